"""GPU: whole-recording restoration (csrc/restore_rec.hip, nppc_audio/inpainting/restore.py) against the fp64 restatement
(tests/restore_ref.py) and against the same launch sequence composed by hand from the public functions.

Shapes: a 24000-sample recording, windows of 8192 samples at n_fft 255 / hop 128, three 1024-sample gaps whose windows clamp at
the start, sit in the middle and clamp at the end; 4 Griffin-Lim iterations; the small U-Net / NPPC pair of
tests/test_inpaint_validator_gpu.py (oracle weights, K = 3).

Tolerances
  gain     1e-12 relative: an fp64 sum of fewer than 2^15 terms per thread and one pow / log10.
  windows  exact: each sample is one fp64 product rounded to fp32, computed here with the kernel's own gain.
  splice   bit-identical outside [s - xf, e + xf); inside, 4 fp32 ulps of max(|recording|, |window output| / gain): what a
           blend of three rounded fp32 operations (divide, subtract, multiply-add) could err by.  The kernel blends in fp64 and
           rounds once, so it sits well inside; the measured worst case is printed.
"""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

import restore_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
L, WIN, XF, NFFT, HOP, K = 24000, 8192, 64, 255, 128, 3
GAPS = [(500, 1524), (11500, 12524), (22000, 23024)]
STARTS = [0, 12012 - WIN // 2, L - WIN]
ALPHAS = [-1.0, 0.5]


def recording(n=L, seed=0):
    t = np.arange(n) / 16000.0
    rng = np.random.default_rng(seed)
    x = 0.05 * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 330 * t + 1)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    return (x + 0.005 * rng.standard_normal(n)).astype(np.float32)


def with_gaps(x, gaps, fill=None):
    y = x.copy()
    rng = np.random.default_rng(99)
    for s, e in gaps:
        y[s:e] = 0.0 if fill is None else fill * rng.standard_normal(e - s)
    return y


def dev_plan(gaps, starts):
    return (torch.tensor(gaps, dtype=torch.int64).cuda(), torch.tensor(starts, dtype=torch.int64).cuda())


def bits(t):
    return t.contiguous().view(torch.int32)


def ulp_limit(rec, y, n_ulps=4):
    return n_ulps * np.spacing(np.maximum(np.abs(rec), np.abs(y)).astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def restorer(tmp_path_factory):
    from nppc_audio.inpainting import restore as RS
    tmp = tmp_path_factory.mktemp("restore")
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(K), 41).items()}
    pre = "pretrained_restoration_model.net."
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, tmp / "restorer.pt")
    torch.save({"model_state_dict": wts}, tmp / "nppc.pt")
    mc = dict(pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
              pretrained_restoration_model_path=str(tmp / "restorer.pt"),
              audio_pc_wrapper_configuration=dict(n_dirs=K, model_configuration=dict(in_channels=2, out_channels=K,
                                                                                     precision="fp32")),
              device="cuda")
    return RS.RecordingRestorer(RS.RecordingRestorerConfig(checkpoint_path=str(tmp / "nppc.pt"), model_configuration=mc,
                                                           window_samples=WIN, n_fft=NFFT, hop_length=HOP, gl_iters=4,
                                                           crossfade_samples=XF))


@pytest.fixture(scope="module")
def restored(restorer):
    """one restore() of the damaged recording with variations, shared (read-only) by the end-to-end tests"""
    x = torch.from_numpy(with_gaps(recording(), GAPS))
    return x, restorer.restore(x, GAPS, alphas=ALPHAS)


# ---- 1. gain, windows, masks -------------------------------------------------------------------------------------------
def test_gain_windows_and_masks_against_the_restatement(record_err):
    from nppc_audio.inpainting import restore as RS
    for fill in (None, 3.0):                                          # zeros in the gaps, then garbage: the same result
        x = with_gaps(recording(), GAPS, fill)
        xd = torch.from_numpy(x).cuda()
        gaps_d, starts_d = dev_plan(GAPS, STARTS)
        gain = RS.recording_gain(xd, gaps_d, -25.0)
        want = R.gain(x, GAPS, -25.0)
        g = float(gain.cpu()[0])
        print(f"gain {g!r} restatement {want!r}")
        record_err(f"gain_fill_{fill}", abs(g - want) / want, 1e-12)
        xw, mt = RS.gather_windows(xd, gaps_d, starts_d, WIN, gain)
        ref_w, ref_m = R.windows(x, GAPS, STARTS, WIN, g)
        assert np.array_equal(mt.cpu().numpy(), ref_m)
        assert np.array_equal(xw.cpu().numpy(), ref_w.astype(np.float32))
        assert float(xw[mt == 0].abs().max()) == 0.0 and int((mt == 0).sum()) == 3 * 1024
        if fill is None:
            first = (g, xw.clone(), mt.clone())
    assert first[0] == g and torch.equal(first[1], xw) and torch.equal(first[2], mt)
    # every sample known (G = 0), a length that is no multiple of four, an unaligned base
    y = torch.from_numpy(recording(1003, 5)).cuda()
    for view in (y, y[1:]):
        got = float(RS.recording_gain(view, torch.empty(0, 2, dtype=torch.int64, device="cuda"))[0])
        want = R.gain(view.cpu().numpy(), [])
        record_err("gain_no_gaps", abs(got - want) / want, 1e-12)


# ---- 2. splice -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [L, L - 1], ids=["vector_path", "scalar_path"])
def test_splice_against_the_restatement(n, record_err):
    """V = 1 and V = K A + 1 = 7 from one launch each; a gap whose ramp is clipped at sample 0 (s < xf) and one clipped at L"""
    from nppc_audio.inpainting import restore as RS
    gaps = [(10, 700), (11500, 12524), (22000, n - 10)]
    starts = [0, 7916, n - WIN]
    x = recording(n, 2)
    rng = np.random.default_rng(4)
    g = 1.7320508
    for V in (1, 7):
        wout = (0.1 * rng.standard_normal((3, V, WIN))).astype(np.float32)
        xd, gain = torch.from_numpy(x).cuda(), torch.tensor([g], dtype=torch.float64).cuda()
        gaps_d, starts_d = dev_plan(gaps, starts)
        got = RS.splice_windows(xd, gaps_d, starts_d, torch.from_numpy(wout).cuda(), gain, XF)
        assert got.shape == (V, n)
        want = R.splice(x, gaps, starts, wout, g, XF)
        region = R.spliced_region(n, gaps, XF)
        assert region.sum() == (700 + XF) + (1024 + 2 * XF) + (XF + n - 10 - 22000 + 10)     # clipped at 0 and at n
        keep = ~torch.from_numpy(region).cuda()
        assert torch.equal(bits(got[:, keep]), bits(xd[keep].expand(V, -1)))
        y = np.zeros((V, n))
        for i, ((s, e), ws) in enumerate(zip(gaps, starts)):
            a, b = max(s - XF, 0), min(e + XF, n)
            y[:, a:b] = wout[i, :, a - ws:b - ws].astype(np.float64) / g
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)[:, region]
        lim = ulp_limit(np.broadcast_to(x, (V, n))[:, region], y[:, region])
        worst = float((err / lim).max())
        print(f"splice n={n} V={V}: worst error {worst * 4:.3f} ulps of max(|recording|, |output| / gain)")
        record_err(f"splice_V{V}", worst, 1.0)
        for i, ((s, e), ws) in enumerate(zip(gaps, starts)):           # on the gap itself: one fp64 division, rounded once
            q = (wout[i, :, s - ws:e - ws].astype(np.float64) / g).astype(np.float32)
            assert np.array_equal(got[:, s:e].cpu().numpy(), q)
        assert torch.equal(got, RS.splice_windows(xd, gaps_d, starts_d, torch.from_numpy(wout).cuda(), gain, XF))
    # strided window outputs (views of a wider buffer) are read in place
    wide = torch.from_numpy((0.1 * rng.standard_normal((3, 9, WIN))).astype(np.float32)).cuda()
    assert torch.equal(RS.splice_windows(xd, gaps_d, starts_d, wide[:, 8], gain, XF)[0],
                       RS.splice_windows(xd, gaps_d, starts_d, wide[:, 8].contiguous(), gain, XF)[0])


# ---- 3. zero runs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ZERO_RUN_CASES))
def test_zero_runs_against_the_restatement(name):
    from nppc_audio.inpainting import restore as RS
    x, min_len = R.ZERO_RUN_CASES[name]
    want = R.zero_runs(x, min_len)
    runs, count = RS.zero_runs(torch.from_numpy(x).cuda(), min_len, 1024)
    n = int(count[0])
    assert n == len(want) and [tuple(r) for r in runs[:n].cpu().tolist()] == want
    runs2, count2 = RS.zero_runs(torch.from_numpy(x).cuda(), min_len, 1024)
    assert torch.equal(count, count2) and torch.equal(runs[:n], runs2[:n])


def test_zero_runs_reports_an_overflow_and_stays_inside_the_buffer():
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import restore as RS
    x, min_len = R.ZERO_RUN_CASES["many_short_runs"]
    want = R.zero_runs(x, min_len)
    assert len(want) > 500
    xd = torch.from_numpy(x).cuda()
    for cap in (0, 2, len(want) - 1, len(want)):
        nchunks = -(-x.size // RS.ZERO_RUN_CHUNK)
        work = torch.empty(nchunks * (4 + 2 * (RS.ZERO_RUN_CHUNK // (min_len + 1) + 1)), dtype=torch.int64, device="cuda")
        buf = torch.full((cap + 8, 2), -7, dtype=torch.int64, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        H.call("nppc_zero_runs", xd, x.size, min_len, work, work.numel(), buf, cap, count, H.stream())
        assert int(count[0]) == len(want)
        assert [tuple(r) for r in buf[:cap].cpu().tolist()] == want[:cap] and bool((buf[cap:] == -7).all())
    with pytest.raises(RuntimeError, match="bad argument"):               # a workspace one element short is refused
        H.call("nppc_zero_runs", xd, x.size, min_len, work, work.numel() - 1, buf, cap, count, H.stream())


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
def by_hand(restorer, x, alphas):
    """restore()'s launch sequence from the public functions and the new kernels"""
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import phase as PH
    from nppc_audio.inpainting import restore as RS
    from nppc_audio.inpainting.data import time_to_spec_mask
    from nppc_audio.inpainting.utils import preprocess_data
    xd = x.cuda()
    gaps_d, starts_d = dev_plan(GAPS, STARTS)
    T, F = 1 + WIN // HOP, NFFT // 2 + 1
    with torch.no_grad():
        gain = RS.recording_gain(xd, gaps_d, -25.0)
        xw, mt = RS.gather_windows(xd, gaps_d, starts_d, WIN, gain)
        mf = time_to_spec_mask(mt, T, WIN, NFFT, HOP, True)
        spec, masked = torch.empty(3, 2, F, T, device="cuda"), torch.empty(3, 2, F, T, device="cuda")
        H.call("nppc_stft_pair", xw, mf, spec, masked, 3, WIN, NFFT, HOP, H.stream())
        _, mask4, mn, mean, std = preprocess_data(masked, masked, mf, plot_mean_std=True)
        mask4 = mask4.contiguous()
        pc = restorer.model(mn, mask4)
        pred = restorer.model.get_pred_spec_mag_norm(mn, mask4)
        var, rest, info = PH.pc_audio_variations_blind(pred, pc, masked, mf, alphas, mean, std, n_iter=4, momentum=0.0,
                                                       n_fft=NFFT, hop_length=HOP, length=WIN)
        out = RS.splice_windows(xd, gaps_d, starts_d, rest, gain, XF)[0]
    return out, var / gain.float(), info, gain, mf


def test_restore_equals_the_hand_composed_sequence_and_repeats(restorer, restored):
    x, out = restored
    assert [p["start"] for p in out["windows"]] == STARTS and [p["gap"] for p in out["windows"]] == GAPS
    hand, hand_vw, info, gain, mf = by_hand(restorer, x, ALPHAS)
    assert int((mf == 0).sum()) > 0 and bool(torch.isfinite(out["restored"]).all())
    assert out["restored"].shape == (L,) and out["variation_windows"].shape == (3, K, len(ALPHAS), WIN)
    assert torch.equal(bits(out["restored"]), bits(hand))
    assert torch.equal(bits(out["variation_windows"]), bits(hand_vw))
    assert torch.equal(out["gain"], gain) and torch.equal(out["status"], info["status"]) and int(out["status"].sum()) == 0
    assert out["inconsistency"].shape == (3, K * len(ALPHAS) + 1, 4) and torch.equal(out["inconsistency"], info["inconsistency"])
    assert out["target_norm"].shape == (3, K * len(ALPHAS) + 1) and float(out["target_norm"].min()) > 0
    again = restorer.restore(x, GAPS, alphas=ALPHAS)                       # two calls: identical bits
    assert torch.equal(bits(again["restored"]), bits(out["restored"]))
    assert torch.equal(bits(again["variation_windows"]), bits(out["variation_windows"]))
    # the known samples are the input's bits; the gaps are filled
    region = torch.from_numpy(R.spliced_region(L, GAPS, XF))
    assert torch.equal(bits(out["restored"].cpu()[~region]), bits(x[~region]))
    for s, e in GAPS:
        assert float(out["restored"][s:e].abs().max()) > 0
    # without alphas: the prediction alone, through griffin_lim_gap
    plain = restorer.restore(x, GAPS)
    assert set(plain) == {"restored", "windows", "gain", "inconsistency", "target_norm", "status"}
    assert plain["inconsistency"].shape == (3, 1, 4) and bool(torch.isfinite(plain["restored"]).all())
    assert torch.equal(bits(plain["restored"].cpu()[~region]), bits(x[~region]))
    assert torch.equal(plain["target_norm"][:, 0] > 0, torch.ones(3, dtype=torch.bool, device="cuda"))


def test_full_variations_equal_the_spliced_variation_windows(restorer, restored, record_err):
    x, out = restored
    full = restorer.restore(x, GAPS, alphas=ALPHAS, variations="full")
    A = len(ALPHAS)
    assert full["variations"].shape == (K, A, L) and "variation_windows" not in full
    assert torch.equal(bits(full["restored"]), bits(out["restored"]))      # row K A of the same launch
    vw = out["variation_windows"].reshape(3, K * A, WIN).cpu().numpy()     # already divided by the gain
    want = R.splice(x.numpy(), GAPS, STARTS, vw, 1.0, XF)
    region = R.spliced_region(L, GAPS, XF)
    got = full["variations"].reshape(K * A, L).cpu().numpy()
    assert np.array_equal(got[:, ~region].view(np.int32), np.broadcast_to(x.numpy(), (K * A, L))[:, ~region].view(np.int32))
    y = np.zeros((K * A, L))
    for i, ((s, e), ws) in enumerate(zip(GAPS, STARTS)):
        y[:, s - XF:e + XF] = vw[i][:, s - XF - ws:e + XF - ws]
    err = np.abs(got.astype(np.float64) - want)[:, region]
    lim = ulp_limit(np.broadcast_to(x.numpy(), (K * A, L))[:, region], y[:, region])
    record_err("full_variations", float((err / lim).max()), 1.0)


# ---- 5. what the gaps hold does not matter ---------------------------------------------------------------------------------
def test_garbage_in_the_gaps_changes_nothing(restorer, restored):
    x, out = restored
    noisy = torch.from_numpy(with_gaps(recording(), GAPS, fill=3.0))
    assert float(noisy[GAPS[0][0]:GAPS[0][1]].abs().max()) > 1 and not torch.equal(noisy, x)
    got = restorer.restore(noisy, GAPS, alphas=ALPHAS)
    assert torch.equal(bits(got["restored"]), bits(out["restored"]))
    assert torch.equal(bits(got["variation_windows"]), bits(out["variation_windows"]))
    assert torch.equal(got["gain"], out["gain"])


# ---- 6. files --------------------------------------------------------------------------------------------------------------
def test_restore_file_round_trip_with_detected_gaps(restorer, tmp_path):
    pcm = np.rint(recording(seed=7).astype(np.float64) * 32768).astype(np.int16)
    for s, e in GAPS:
        pcm[s:e] = 0
    wavfile.write(str(tmp_path / "in.wav"), 16000, pcm)
    from nppc_audio.data import _decode_wav
    assert restorer.detect_gaps(_decode_wav(tmp_path / "in.wav", 16000)) == GAPS
    out = restorer.restore_file(tmp_path / "in.wav", tmp_path / "out.wav")
    assert [p["gap"] for p in out["windows"]] == GAPS
    sr, back = wavfile.read(str(tmp_path / "out.wav"))
    assert sr == 16000 and back.dtype == np.int16 and back.shape == pcm.shape
    region = R.spliced_region(L, GAPS, XF)
    wrong = int((back[~region] != pcm[~region]).sum())
    print(f"restore_file: {wrong} known samples differ from the input's int16 values")
    assert wrong == 0                                                      # known samples never pass through the gain
    for s, e in GAPS:
        assert np.abs(back[s:e]).max() > 0
    # given gaps are taken as they are (no detection)
    out2 = restorer.restore_file(tmp_path / "in.wav", tmp_path / "out2.wav", gaps=GAPS[:1])
    assert [p["gap"] for p in out2["windows"]] == GAPS[:1]
    back2 = wavfile.read(str(tmp_path / "out2.wav"))[1]
    assert np.array_equal(back2[GAPS[1][0]:GAPS[1][1]], np.zeros(1024, np.int16))
