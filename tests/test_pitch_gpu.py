"""GPU: csrc/pitch.hip stage by stage and end to end against the fp64 restatement tests/pyin_ref.py, its invariances, and the
two validators' pitch results.

Limits of the two numeric stages are measured inside the test from an fp32 evaluation of the same stage on the CPU (torch
for d', NumPy for the observation probabilities) against fp64: the kernel may err at most twice as much (the convention of
DESIGN.md section 8a).  The Viterbi stage and the invariances are exact.  End to end, voiced_flag or pitch bin may differ
from the all-fp64 restatement on at most 1 % of a test's frames (twice what tests/test_pitch_cpu.py allows the restatement
against itself with an fp32 d'), by one bin at most where both are voiced."""
import numpy as np
import pytest
import torch

import pyin_ref as R
from test_pitch_cpu import FMIN, FMAX, all_signals, check_ground_truth, ground_truth_signals, ref_run

pytestmark = pytest.mark.gpu

SETTINGS = {"reference": dict(fmin=80.0, fmax=400.0), "odd": dict(fmin=100.0, fmax=500.0, frame_length=600, hop_length=100)}


def batch_of(N, L, seed):
    """N speech-like clips of L samples -> fp32 [N, L]: L consecutive samples of a 1.5 s clip, starting at its loudest sample
    (the generator gates its source on and off, and a short excerpt taken blindly can be digital silence)"""
    out = np.zeros((N, L), np.float32)
    for i in range(N):
        y = R.speech_like(seed + i, dur=max(1.5, L / 16000.0 + 0.5))[0]
        o = min(int(np.argmax(np.abs(y))), len(y) - L)
        out[i] = y[o:o + L]
        assert np.abs(out[i]).max() > 0.05
    return out


def cases(setting):
    s = R.Setting(**setting)
    hop, fl = s.hop_length, s.frame_length
    # (N, L, lengths): frame-aligned, not aligned, shorter than a frame, ragged
    return [(1, 8 * hop, None), (3, 8 * hop, None), (1, 7 * hop + hop // 3 + 1, None), (3, 7 * hop + hop // 3 + 1, None),
            (1, fl // 2 - 7, None), (3, fl // 2 - 7, None), (3, 9 * hop + 5, [9 * hop + 5, 3 * hop - 1, fl // 3])]


def dprime_fp32_torch(y, s):
    """the d' chain in fp32 torch on the CPU: [L] -> [T, P]"""
    fr = torch.from_numpy(R.frames_of(y, s)).float()
    W = s.win_length
    d = torch.stack([((fr[:, :W] - fr[:, tau:tau + W]) ** 2).sum(1) for tau in range(s.max_period + 1)], dim=1)
    d = torch.where(d < 1e-6, torch.zeros_like(d), d)
    mean = torch.cumsum(d[:, 1:], dim=1) / torch.arange(1, s.max_period + 1, dtype=torch.float32)
    dp = d[:, 1:] / (mean + torch.finfo(torch.float32).tiny)
    return dp[:, s.min_period - 1:].numpy()


def frame_rel_err(got, ref):
    """largest error relative to the fp64 peak of the frame; frames whose fp64 d' is all zero must be all zero"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    peak = np.abs(ref).max(axis=1)
    live = peak > 0
    assert np.all(got[~live] == 0.0)
    if not live.any():
        return 0.0
    return float((np.abs(got - ref)[live].max(axis=1) / peak[live]).max())


def within(record_err, tag, err, yard):
    """err < 2 * yard, recorded; where the fp32 evaluation itself is exact (yard == 0) so must the kernel be"""
    if yard == 0.0:
        assert err == 0.0, (tag, err)
    else:
        record_err(tag, err, 2 * yard)


def device_bins(f0, s):
    f0 = np.asarray(f0, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(f0), -1, np.rint(12 * s.nbps * np.log2(f0 / s.fmin))).astype(np.int64)


def stages(y, setting, lengths=None, **kw):
    from nppc_audio.pitch import pyin_stages
    return pyin_stages(torch.from_numpy(np.ascontiguousarray(y)).cuda(), lengths=lengths, **setting, **kw)


# ---- 1. d' ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETTINGS))
def test_cmnd_against_the_fp64_restatement(name, record_err):
    setting = SETTINGS[name]
    s = R.Setting(**setting)
    for ci, (N, L, lengths) in enumerate(cases(setting)):
        y = batch_of(N, L, 10 * ci + 1)
        got = stages(y, setting, lengths)["dprime"].cpu().numpy()
        assert got.shape == (N, s.n_frames(L), s.P)
        for i in range(N):
            Li = L if lengths is None else lengths[i]
            Ti = s.n_frames(Li)
            ref = R.cmnd(y[i, :Li], s)
            f32 = dprime_fp32_torch(y[i, :Li], s)
            err, yard = frame_rel_err(got[i, :Ti], ref), frame_rel_err(f32, ref)
            print(f"cmnd {name} N={N} L={L} item {i} (len {Li}): kernel {err:.3e}  torch fp32 {yard:.3e}")
            within(record_err, f"{name}/N{N}/L{L}/i{i}", err, yard)
            assert np.all(got[i, Ti:] == 0.0)


# ---- 2. observation probabilities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETTINGS))
def test_observe_against_the_restatement_on_the_device_dprime(name, record_err):
    setting = SETTINGS[name]
    s = R.Setting(**setting)
    for ci, (N, L, lengths) in enumerate(cases(setting)):
        y = batch_of(N, L, 10 * ci + 1)
        st = stages(y, setting, lengths)
        dp, obs, vp = (st[k].cpu().numpy() for k in ("dprime", "obs", "voiced_prob"))
        for i in range(N):
            Ti = s.n_frames(L if lengths is None else lengths[i])
            ref_o, ref_v = R.observe(dp[i, :Ti], s)                          # fp64 on the very same fp32 d'
            f32_o, f32_v = R.observe(dp[i, :Ti], s, dtype=np.float32)
            assert np.array_equal(obs[i, :Ti, :s.n_pitch_bins] != 0, ref_o[:, :s.n_pitch_bins] != 0)   # the same bins are hit
            err_o, yard_o = np.abs(obs[i, :Ti] - ref_o).max(), np.abs(f32_o.astype(np.float64) - ref_o).max()
            err_v, yard_v = np.abs(vp[i, :Ti] - ref_v).max(), np.abs(f32_v.astype(np.float64) - ref_v).max()
            print(f"observe {name} N={N} L={L} item {i}: obs kernel {err_o:.3e} numpy fp32 {yard_o:.3e}; "
                  f"voiced_prob kernel {err_v:.3e} numpy fp32 {yard_v:.3e}")
            within(record_err, f"{name}/N{N}/L{L}/i{i}/obs", err_o, yard_o)
            within(record_err, f"{name}/N{N}/L{L}/i{i}/voiced_prob", err_v, yard_v)
            assert np.all(obs[i, Ti:] == 0.0) and np.all(vp[i, Ti:] == 0.0)


# ---- 3. Viterbi ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETTINGS))
def test_viterbi_decodes_the_restatements_path_from_the_device_observations(name):
    setting = SETTINGS[name]
    s = R.Setting(**setting)
    for ci, (N, L, lengths) in enumerate(cases(setting)):
        y = batch_of(N, L, 10 * ci + 1)
        st = stages(y, setting, lengths)
        obs, f0, flag = (st[k].cpu().numpy() for k in ("obs", "f0", "voiced_flag"))
        for i in range(N):
            Ti = s.n_frames(L if lengths is None else lengths[i])
            _, ref_flag, ref_bin = R.decode(R.viterbi(obs[i, :Ti], s), s)
            assert np.array_equal(flag[i, :Ti], ref_flag), (name, N, L, i)
            v = ref_flag.astype(bool)
            assert np.array_equal(device_bins(f0[i, :Ti], s)[v], ref_bin[v]), (name, N, L, i)
            assert np.all(np.isnan(f0[i, :Ti][~v]))


def test_viterbi_on_long_voiced_chains():
    """the 2 s signals: 63 frames, mostly voiced"""
    setting = SETTINGS["reference"]
    s = R.Setting(**setting)
    sig = ground_truth_signals()
    y = np.stack([v[0] for v in sig.values()])
    st = stages(y, setting)
    obs, f0, flag = (st[k].cpu().numpy() for k in ("obs", "f0", "voiced_flag"))
    for i in range(len(y)):
        _, ref_flag, ref_bin = R.decode(R.viterbi(obs[i], s), s)
        assert np.array_equal(flag[i], ref_flag)
        v = ref_flag.astype(bool)
        assert v.sum() > 50 and np.array_equal(device_bins(f0[i], s)[v], ref_bin[v])


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_all_fp64_restatement():
    from nppc_audio.pitch import pyin
    s = R.Setting(FMIN, FMAX)
    sig = all_signals()
    names = list(sig)
    L = max(len(v) for v in sig.values())
    y = np.zeros((len(names), L), np.float32)
    lengths = [len(sig[n]) for n in names]
    for i, n in enumerate(names):
        y[i, :lengths[i]] = sig[n]
    f0, flag, vp = (t.cpu().numpy() for t in pyin(torch.from_numpy(y).cuda(), FMIN, FMAX, lengths=lengths))
    total = differ = 0
    gt = ground_truth_signals()
    for i, n in enumerate(names):
        ref = ref_run(n, sig[n])
        Ti = s.n_frames(lengths[i])
        b = device_bins(f0[i, :Ti], s)
        both = (flag[i, :Ti] == 1) & (ref["voiced_flag"] == 1)
        d = (flag[i, :Ti] != ref["voiced_flag"]) | (both & (b != ref["bin"]))
        print(f"end to end {n}: {int(d.sum())} of {Ti} frames differ; largest voiced_prob difference "
              f"{np.abs(vp[i, :Ti] - ref['voiced_prob']).max():.2e}")
        assert np.all(np.abs(b - ref["bin"])[both] <= 1), n
        total, differ = total + Ti, differ + int(d.sum())
        if n in gt:
            check_ground_truth(n, sig[n], gt[n][1], f0[i, :Ti], flag[i, :Ti])
        if n == "zeros":
            assert not flag[i, :Ti].any() and np.all(vp[i, :Ti] == 0.0)
        if n == "noise":
            assert not flag[i, :Ti].any()
    assert differ <= 0.01 * total, (differ, total)


# ---- 5. invariances ------------------------------------------------------------------------------------------------------
def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_batch_independence_repeatability_and_ragged_items(name):
    from nppc_audio.pitch import pyin
    setting = SETTINGS[name]
    s = R.Setting(**setting)
    hop = s.hop_length
    L = 23 * hop + 17
    y = torch.from_numpy(batch_of(4, L, 77)).cuda()
    a = pyin(y, **setting)
    assert a[0].shape == (4, s.n_frames(L)) and a[1].dtype == torch.uint8 and a[2].dtype == torch.float32
    assert same(a, pyin(y, **setting))                                       # two runs
    for i in range(4):
        assert same([t[i:i + 1] for t in a], pyin(y[i:i + 1], **setting))    # alone == in the batch
    one = pyin(y[2], **setting)                                              # [L] keeps its shape
    assert one[0].shape == (s.n_frames(L),) and same(one, [t[2] for t in a])
    lead = pyin(y.view(2, 2, L), **setting)                                  # any leading shape
    assert lead[0].shape == (2, 2, s.n_frames(L)) and same([t.reshape(4, -1) for t in lead], a)
    lengths = [L, 5 * hop + 3, hop - 1, 11 * hop]
    junk = y.clone()
    for i, n in enumerate(lengths):
        junk[i, n:] = 1e30                                                   # what lies past an item's end is never read
    r = pyin(junk, lengths=lengths, **setting)
    for i, n in enumerate(lengths):
        Ti = s.n_frames(n)
        alone = pyin(y[i, :n].contiguous(), **setting)
        assert same([t[i, :Ti] for t in r], alone), (name, i)                # the clip run alone at its own length
        assert bool(torch.isnan(r[0][i, Ti:]).all()) and not bool(r[1][i, Ti:].any()) and bool((r[2][i, Ti:] == 0).all())
    dev_len = pyin(junk, lengths=torch.tensor(lengths).cuda(), **setting)    # lengths may live on the device
    assert same(dev_len, r)


# ---- 6. validators -------------------------------------------------------------------------------------------------------
def test_inpainting_validator_pitch(tmp_path):
    from nppc_audio import pitch as PT
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    from test_inpaint_gpu import build_trainer, load
    from test_inpaint_validator_gpu import held_out
    z, meta = load("inp_tiny")
    c = meta["config"]
    tr, _, _ = build_trainer(meta, "fp32", tmp_path, z)
    ck = str(tmp_path / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    val = V.NPPCModelValidator(V.NPPCModelValidatorConfig(checkpoint_path=ck, save_dir=str(tmp_path / "val"),
                                                          model_configuration=tr.config.nppc_model_configuration.model_dump()))
    b = held_out(z, 3)
    net = val.model.pretrained_restoration_model.net
    kw = dict(n_mc_samples=8, n_components=c["K"], alphas=V.default_alphas(), n_fft=c["nfft"], hop_length=c["hop"])
    net.dropout_pass = 0
    plain = val.validate_batch(*b, **kw)
    net.dropout_pass = 0
    off = val.validate_batch(*b, pitch=False, **kw)
    net.dropout_pass = 0
    on = val.validate_batch(*b, pitch=True, **kw)
    assert set(plain) == set(off) == set(on) - {"pitch"}
    assert set(plain) == {"pc_directions", "pred_spec_mag_norm", "clean_spec_mag_norm", "mask", "mean", "std", "mc_dropout",
                          "metrics", "audio_variations", "clean_audio"}          # the keys before this option existed

    def equal(u, v):
        if isinstance(u, torch.Tensor):
            return torch.equal(u, v)
        if isinstance(u, dict):
            return set(u) == set(v) and all(equal(u[k], v[k]) for k in u)
        if isinstance(u, (list, tuple)):
            return len(u) == len(v) and all(equal(p, q) for p, q in zip(u, v))
        return bool(np.all(np.asarray(u) == np.asarray(v)))
    for k in plain:
        assert equal(plain[k], off[k]) and equal(plain[k], on[k]), k
    B, K, A, L = on["audio_variations"].shape
    T = 1 + L // 512
    p = on["pitch"]
    assert set(p) == {"f0_clean", "voiced_flag_clean", "voiced_prob_clean", "f0", "voiced_flag", "voiced_prob", "summary"}
    assert p["f0_clean"].shape == (B, T) and p["f0"].shape == (B, K, A, T) and p["voiced_flag"].shape == (B, K, A, T)
    assert p["voiced_prob"].shape == (B, K, A, T) and p["voiced_flag_clean"].dtype == torch.uint8
    assert all(v.shape == (B, K, A) for v in p["summary"].values())
    direct = PT.pyin(on["audio_variations"], 80, 400, sr=16000)
    assert same([p["f0"], p["voiced_flag"], p["voiced_prob"]], direct)
    direct_c = PT.pyin(on["clean_audio"], 80, 400, sr=16000)
    assert same([p["f0_clean"], p["voiced_flag_clean"], p["voiced_prob_clean"]], direct_c)
    with pytest.raises(ValueError, match="alphas"):
        val.validate_batch(*b, pitch=True, n_mc_samples=8, n_components=c["K"])


def test_speech_enhancement_pc_pitch(tmp_path):
    from nppc_audio import ops
    from nppc_audio import pitch as PT
    from nppc_audio.pc_pitch import pc_direction_pitch
    from nppc_validation_ref import build_model
    from oracle import weights as W
    c = dict(F=257, nfft=512, hop=256, sbn=15, sbh=384, K=2, G_rest=1, G_pc=1, seed=3)
    model, _ = build_model(c, "fp32", tmp_path)
    model.eval()
    noisy = torch.from_numpy(W.synth_batch(2, 8192)[0]).cuda()
    alphas = [-2.0, 0.0, 1.5]
    out = pc_direction_pitch(model, noisy, alphas)
    with torch.no_grad():                                                    # the waveforms are the existing op's, bit for bit
        w = model(noisy)
        f = model._front(noisy)
        enh, var = ops.pc_direction_waveforms(f["pred_crm"], w, alphas, f["re"], f["im"], 8192, 512, 256)
    assert torch.equal(out["enhanced"], enh) and torch.equal(out["variations"], var)
    T = 1 + 8192 // 512
    assert out["f0_clean"].shape == (2, T) and out["f0"].shape == (2, 2, 3, T)
    assert all(v.shape == (2, 2, 3) for v in out["summary"].values())
    assert same([out["f0"], out["voiced_flag"], out["voiced_prob"]], PT.pyin(var, 80, 400, sr=16000))
    assert same([out["f0_clean"], out["voiced_flag_clean"], out["voiced_prob_clean"]], PT.pyin(enh, 80, 400, sr=16000))
