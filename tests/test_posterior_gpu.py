"""GPU: the fused posterior sampler (csrc/posterior.hip, nppc_audio/posterior.py) at the smallest shapes where it can go wrong.

Shapes: (n_fft, hop) in {(64,8) (11 frames in LDS, the most), (64,16), (64,32), (512,256)}; K in {1, 5, 16}; S in {1, 3,
TILE + 1}; B in {1, 3}; three output blocks and a bit, L no multiple of hop; ragged lengths with an item 3 samples over
n_fft / 2 (whole blocks past its end), one a little over one block, one full.  pred uniform in [-3, 3], w at scale 0.5.

1. parity: the fused launch and the composed existing path (masks by torch fp32 ops in the stated order, then
   ops.cirm_decompress_apply + ops.istft; decompressed domain: the decompress of ops.cirm_decompress_apply_conj, the
   combination and product by torch, ops.istft) are both measured against the fp64 restatement; the fused errors (max-abs
   and RMS over the peak) are at most 4x the composed ones: both are fp32 evaluations of one formula.
2. z = 0, S = 1 is ops.model_outputs_to_waveforms bit for bit.
3. the reference's validator fixture in the decompressed domain.
4. batch, run and S independence, bit for bit.
5. statistics against the fp64 two-pass result of what the same launch returned (mean 1.2e-7 peak: one fp32 rounding; std
   1e-6 peak: the one-pass fp64 cancellation bound sqrt(S 2^-52) peak at S = 4096 plus one fp32 rounding).  The launch
   returns no spectra, so the spectrum statistics are checked against the |X_s| planes of the composed path.
6. ragged tails are exactly 0.
7. PosteriorSampler and NPPCAudioValidator.save_posterior_samples on a tiny random-weight model."""
import json
import os

import numpy as np
import pytest
import torch

import posterior_ref as PR
from golden_util import GOLD, load
from oracle import weights as W

pytestmark = pytest.mark.gpu
CONFIGS = [(64, 8), (64, 16), (64, 32), (512, 256)]
STAT_KEYS = ("mean", "std", "mag_mean", "mag_std")
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    """NPPC_POSTERIOR_PARITY_OUT=<file>: the errors of both paths and whether they were bit-equal, per case, as JSON
    (profiles/posterior_parity_errors.json is such a run)"""
    yield
    path = os.environ.get("NPPC_POSTERIOR_PARITY_OUT")
    if _RECORD and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(_RECORD, open(path, "w"), indent=1, sort_keys=True)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def length_of(hop):
    return 3 * 4 * hop + hop // 2 + 3


def ragged_of(B, nfft, hop):
    return [nfft // 2 + 3] if B == 1 else [length_of(hop), nfft // 2 + 3, 4 * hop + hop // 2 + 1][:B]


def fused(case, L, nfft, hop, **kw):
    from nppc_audio import posterior as P
    pred, w, re, im, z = case
    return P.sample_waveforms(dev(pred), dev(w), dev(re), dev(im), dev(z), L, nfft, hop, **kw)


def composed(case, L, nfft, hop, lengths=None, domain="compressed"):
    """the existing ops around masks built by torch fp32 operations in the stated order -> (waves [B,S,L], |X| [B,S,F,T])"""
    from nppc_audio import ops
    pred, w, re, im, z = (dev(a) for a in case)
    B, S, K = z.shape[:3]
    F, T = re.shape[1:]
    if domain == "compressed":
        pr, pi, wr, wi = pred[:, 0], pred[:, 1], w[:, :, 0], w[:, :, 1]
    else:
        dec = ops.cirm_decompress_apply_conj(torch.cat((pred, w.reshape(B * K, 2, F, T))), re.repeat(1 + K, 1, 1),
                                             im.repeat(1 + K, 1, 1), want_dec=True)[0]
        pr, pi = dec[:B, ..., 0], dec[:B, ..., 1]
        wr, wi = dec[B:, ..., 0].reshape(B, K, F, T), dec[B:, ..., 1].reshape(B, K, F, T)
    mr, mi = pr[:, None].repeat(1, S, 1, 1), pi[:, None].repeat(1, S, 1, 1)
    for k in range(K):
        zr, zi = z[:, :, k, 0, None, None], z[:, :, k, 1, None, None]
        a, c = wr[:, None, k], wi[:, None, k]
        mr = mr + (zr * a - zi * c)
        mi = mi + (zr * c + zi * a)
    n_re = re[:, None].expand(B, S, F, T).reshape(B * S, F, T)
    n_im = im[:, None].expand(B, S, F, T).reshape(B * S, F, T)
    if domain == "compressed":
        mag, xr, xi = ops.cirm_decompress_apply(torch.stack((mr, mi), dim=2).reshape(B * S, 2, F, T), n_re, n_im)
    else:
        mr, mi = mr.reshape(B * S, F, T), mi.reshape(B * S, F, T)
        xr, xi = mr * n_re - mi * n_im, mi * n_re + mr * n_im
        mag = torch.sqrt(xr * xr + xi * xi)
    rows = None if lengths is None else [n for n in lengths for _ in range(S)]
    waves = ops.istft(xr.contiguous(), xi.contiguous(), nfft, hop, L, lengths=rows)
    return waves.view(B, S, L), mag.view(B, S, F, T)


def errors(got, want):
    """(max-abs, RMS) error over the peak of the reference"""
    got, want = got.double().cpu().numpy(), np.asarray(want)
    peak = np.abs(want).max()
    return float(np.abs(got - want).max() / peak), float(np.sqrt(((got - want) ** 2).mean()) / peak)


def check_parity(tag, case, L, nfft, hop, lengths, domain):
    want = PR.sample_waveforms(*case, L, nfft, hop, lengths=lengths, domain=domain)["samples"]
    f = fused(case, L, nfft, hop, lengths=lengths, domain=domain)["samples"]
    c, _ = composed(case, L, nfft, hop, lengths, domain)
    fe, ce = errors(f, want), errors(c, want)
    _RECORD[tag] = dict(fused_maxabs=fe[0], fused_rms=fe[1], composed_maxabs=ce[0], composed_rms=ce[1],
                        bit_equal=bool(torch.equal(f, c)))
    print(f"{tag}: fused {fe[0]:.3e} / {fe[1]:.3e}, composed {ce[0]:.3e} / {ce[1]:.3e}, bit-equal {_RECORD[tag]['bit_equal']}")
    assert fe[0] <= 4 * ce[0] and fe[1] <= 4 * ce[1], (tag, fe, ce)
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert not f[b, :, n:].any(), (tag, b)


@pytest.mark.parametrize("S", [1, 3, 9])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("nfft,hop", CONFIGS)
def test_fused_launch_is_as_close_to_fp64_as_the_composed_path(nfft, hop, K, B, S):
    from nppc_audio import posterior as P
    assert S in (1, 3, P.TILE + 1)
    L = length_of(hop)
    for kind, cplx in (("real", False), ("complex", True)):
        case = PR.case(B, S, K, nfft, hop, L, seed=1000 * K + 10 * S + B, complex_coeffs=cplx)
        for lengths in (None, ragged_of(B, nfft, hop)):
            for domain in ("compressed", "decompressed"):
                tag = f"n{nfft}_h{hop}_K{K}_B{B}_S{S}_{kind}_{'ragged' if lengths else 'uniform'}_{domain}"
                check_parity(tag, case, L, nfft, hop, lengths, domain)


@pytest.mark.parametrize("nfft,hop", [(64, 16), (512, 256)])
def test_coefficients_of_40_put_most_bins_on_the_clamp(nfft, hop):
    L = length_of(hop)
    case = PR.case(3, 3, 5, nfft, hop, L, seed=77, zscale=40.0, complex_coeffs=True)
    mr, _ = PR.masks(case[0], case[1], case[4])
    assert (np.abs(mr) == PR.decompress(9.9)).mean() > 0.5
    check_parity(f"clamp_n{nfft}_h{hop}", case, L, nfft, hop, ragged_of(3, nfft, hop), "compressed")


@pytest.mark.parametrize("domain", ["compressed", "decompressed"])
@pytest.mark.parametrize("nfft,hop", CONFIGS)
def test_zero_coefficients_are_the_enhanced_waveform_bit_for_bit(nfft, hop, domain):
    from nppc_audio import ops
    L = length_of(hop)
    pred, w, re, im, z = PR.case(3, 1, 5, nfft, hop, L, seed=5)
    for lengths in (None, ragged_of(3, nfft, hop)):
        got = fused((pred, w, re, im, 0 * z), L, nfft, hop, lengths=lengths, domain=domain)["samples"][:, 0]
        want = ops.model_outputs_to_waveforms(dev(pred), dev(re)[:, None], dev(im)[:, None], L, nfft, hop, lengths=lengths)
        assert torch.equal(got, want), (lengths, float((got - want).abs().max()))


def test_reference_validator_fixture_in_the_decompressed_domain():
    """coeffs[b, k A + a] = alpha_a e_k reproduces the reference validator's `enhanced + alpha PC_k` waveforms"""
    from nppc_audio import posterior as P
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-30))
    v = np.load(os.path.join(GOLD, "validator_f1.npz"))
    z, _ = load("g1_c1")
    n_re, n_im, pred = dev(z["noisy_real"][:, 0]), dev(z["noisy_imag"][:, 0]), dev(z["pred_crm_full"])
    L = z["noisy"].shape[1]
    alphas = [float(a) for a in v["alphas"]]
    A = len(alphas)
    for tag, w in (("w", z["log.w_mat"]), ("wbig", v["w_big"])):
        B, K = w.shape[:2]
        coeffs = torch.zeros(B, K * A + 1, K)
        for k in range(K):
            coeffs[:, k * A:(k + 1) * A, k] = torch.tensor(alphas)
        out = P.sample_waveforms(pred, dev(w), n_re, n_im, coeffs.cuda(), L, 512, 256, domain="decompressed")["samples"].cpu().numpy()
        assert rel(out[:, :-1].reshape(B, K, A, L), v[f"{tag}_waves"]) < 2e-5
        assert rel(out[:, -1], v["enhanced_wave"]) < 1e-5


@pytest.mark.parametrize("nfft,hop", [(64, 8), (512, 256)])
def test_item_run_and_sample_independence(nfft, hop):
    L, B, S, K = length_of(hop), 3, 9, 5
    case = PR.case(B, S, K, nfft, hop, L, seed=21, complex_coeffs=True)
    lengths = ragged_of(B, nfft, hop)
    kw = dict(lengths=lengths, stats=True, spec_stats=True)
    a, b2 = fused(case, L, nfft, hop, **kw), fused(case, L, nfft, hop, **kw)
    for key in ("samples",) + STAT_KEYS:
        assert torch.equal(a[key], b2[key]), key                    # run to run
    for b in range(B):                                              # an item alone, at the batch's padded length
        alone = fused(tuple(x[b:b + 1] for x in case), L, nfft, hop, lengths=lengths[b:b + 1], stats=True, spec_stats=True)
        for key in ("samples",) + STAT_KEYS:
            assert torch.equal(alone[key][0], a[key][b]), (b, key)
    for s in (3, 8):                                                # a sample alone; row 8 lies behind the tile boundary
        one = fused(case[:4] + (case[4][:, s:s + 1],), L, nfft, hop, lengths=lengths)["samples"]
        assert torch.equal(one[:, 0], a["samples"][:, s]), s
    uni = fused(case, L, nfft, hop)["samples"]
    assert torch.equal(uni[0], a["samples"][0])                     # the full-length item: ragged == uniform


@pytest.mark.parametrize("nfft,hop,S", [(64, 8, 9), (64, 16, 40), (64, 32, 2), (512, 256, 9)])
def test_statistics_match_the_two_pass_fp64_result_of_the_returned_samples(nfft, hop, S):
    L, B, K = length_of(hop), 3, 5
    case = PR.case(B, S, K, nfft, hop, L, seed=31 + S)
    for lengths in (None, ragged_of(B, nfft, hop)):
        full = fused(case, L, nfft, hop, lengths=lengths, stats=True, spec_stats=True)
        only = fused(case, L, nfft, hop, lengths=lengths, samples=False, stats=True, spec_stats=True)
        assert "samples" not in only
        for key in STAT_KEYS:
            assert torch.equal(full[key], only[key]), key           # stats-only == stats of a call that returns samples
        y = full["samples"].double().cpu().numpy()
        mag = composed(case, L, nfft, hop, lengths)[1].double().cpu().numpy()
        for b, n in enumerate(lengths or []):
            mag[b, :, :, 1 + n // hop:] = 0.0
        for x, mkey, skey in ((y, "mean", "std"), (mag, "mag_mean", "mag_std")):
            m, sd = PR.stats(x)
            peak = np.abs(x).max()
            em = np.abs(full[mkey].double().cpu().numpy() - m).max() / peak
            es = np.abs(full[skey].double().cpu().numpy() - sd).max() / peak
            print(f"n{nfft} h{hop} S{S} {'ragged' if lengths else 'uniform'} {mkey}: {em:.3e}, {skey}: {es:.3e}")
            assert em <= 1.2e-7 and es <= 1e-6, (mkey, em, es)
        for b, n in enumerate(lengths or []):                       # ragged tails: exactly 0
            assert not full["samples"][b, :, n:].any() and not full["mean"][b, n:].any() and not full["std"][b, n:].any()
            assert not full["mag_mean"][b, :, 1 + n // hop:].any() and not full["mag_std"][b, :, 1 + n // hop:].any()
            assert full["mag_mean"][b, :, :1 + n // hop].all()


def test_refusals_come_before_any_launch():
    from nppc_audio import posterior as P
    case = tuple(dev(a) for a in PR.case(2, 3, 5, 64, 16, 100, seed=1))
    with pytest.raises(ValueError, match="n_fft"):
        P.sample_waveforms(*case, 100, 64, 4)
    with pytest.raises(ValueError, match="statistics need"):
        P.sample_waveforms(*case[:4], case[4][:, :1], 100, 64, 16, stats=True)
    with pytest.raises(ValueError, match="too short"):
        P.sample_waveforms(*case, 100, 64, 16, lengths=[100, 32])
    with pytest.raises(ValueError, match="exceeds"):
        P.sample_waveforms(*case, 100, 64, 16, lengths=[100, 101])


# ---- the sampler around a model ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audio_validator(tmp_path_factory):
    from nppc_audio.validator import NPPCAudioValidator, NPPCAudioValidatorConfig
    tmp = tmp_path_factory.mktemp("posterior")
    _, meta = load("g1_c1")
    c = meta["config"]
    spec = W.nppc_spec(c["K"], num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    wts = {k: torch.from_numpy(v) for k, v in W.make_weights(spec, c["seed"]).items()}
    pre = "pretrained_restoration_model."
    ck = os.path.join(str(tmp), "restorer.tar")
    torch.save({"model": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    common = dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"], precision="fp32")
    model_cfg = dict(
        pretrained_restoration_model_configuration=dict(common, num_groups_in_drop_band=c["G_rest"]),
        pretrained_restoration_model_path=ck,
        audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(common, num_groups_in_drop_band=c["G_pc"],
                                                                               n_directions=c["K"])),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda")
    nppc = os.path.join(str(tmp), "nppc.pt")
    torch.save({"model_state_dict": wts, "step": 0}, nppc)
    val = NPPCAudioValidator(NPPCAudioValidatorConfig(nppc_audio_model_configuration=model_cfg, checkpoint_path=nppc))
    return val, model_cfg, nppc, c, tmp


def test_posterior_sampler_on_two_ragged_clips(audio_validator):
    from nppc_audio import metrics as M
    from nppc_audio import posterior as P
    val, model_cfg, nppc, c, tmp = audio_validator
    sampler = P.PosteriorSampler(P.PosteriorSamplerConfig(nppc_audio_model_configuration=model_cfg, checkpoint_path=nppc))
    L, lengths, S = 16000, [16000, 12003], 3
    noisy, clean = (torch.from_numpy(a) for a in W.synth_batch(2, L))
    for b, n in enumerate(lengths):
        noisy[b, n:] = 0
        clean[b, n:] = 0
    F, T, K = c["F"], 1 + L // c["hop"], c["K"]
    r = sampler.sample(noisy, n_samples=S, seed=4, lengths=lengths, stats=True, spec_stats=True)
    assert r["samples"].shape == (2, S, L) and r["coeffs"].shape == (2, S, K, 2) and r["enhanced"].shape == (2, L)
    assert r["mean"].shape == r["std"].shape == (2, L) and r["mag_mean"].shape == r["mag_std"].shape == (2, F, T)
    assert torch.equal(r["coeffs"], P.draw_coefficients(2, S, K, seed=4))
    assert bool(torch.isfinite(r["samples"]).all()) and not r["samples"][1, :, lengths[1]:].any()
    assert float(r["std"][0].max()) > 0                             # the samples differ
    again = sampler.sample(noisy, coeffs=r["coeffs"], lengths=lengths)
    assert torch.equal(again["samples"], r["samples"])
    # z = 0: the samples are the enhanced clip, and so are their scores
    zero = torch.zeros(2, 2, K)
    assert torch.equal(sampler.sample(noisy, coeffs=zero, lengths=lengths)["samples"][:, 1], r["enhanced"])
    sp = sampler.score_spread(noisy, clean, metrics=("STOI", "SI_SDR"), coeffs=zero, lengths=lengths)
    want = {"STOI": M.stoi(clean.cuda(), r["enhanced"], lengths=lengths).cpu().tolist(),
            "SI_SDR": M.si_sdr(clean.cuda(), r["enhanced"], lengths=lengths).cpu().tolist()}
    for m in ("STOI", "SI_SDR"):
        assert set(sp[m]) == {"enhanced", "mean", "std", "min", "max"} and all(len(v) == 2 for v in sp[m].values())
        # the same rows in one call: the same scores; against a call of its own: fp64 sums that may be grouped differently
        assert sp[m]["min"] == sp[m]["enhanced"] and sp[m]["max"] == sp[m]["enhanced"] and sp[m]["std"] == [0.0, 0.0]
        assert np.allclose(sp[m]["mean"], sp[m]["enhanced"], rtol=1e-15, atol=0)
        assert np.allclose(sp[m]["enhanced"], want[m], rtol=1e-9, atol=0), (m, sp[m]["enhanced"], want[m])
    drawn = sampler.score_spread(noisy, clean, n_samples=4, seed=1, lengths=lengths)
    for m in ("STOI", "SI_SDR"):
        for b in range(2):
            assert drawn[m]["min"][b] <= drawn[m]["mean"][b] <= drawn[m]["max"][b] and drawn[m]["std"][b] >= 0
        assert np.allclose(drawn[m]["enhanced"], want[m], rtol=1e-9, atol=0)
    assert min(drawn["SI_SDR"]["std"]) > 0
    with pytest.raises(ValueError, match="registered"):
        sampler.score_spread(noisy, clean, metrics=("PESQ",), lengths=lengths)


def test_validator_writes_posterior_samples_that_read_back(audio_validator):
    from PIL import Image
    from nppc_audio import flac as FL
    val, _, _, c, tmp = audio_validator
    L, S = 8000, 3
    noisy, _ = W.synth_batch(2, L)
    paths = val.save_posterior_samples(torch.from_numpy(noisy), tmp / "post", n_samples=S, seed=2)
    want = [tmp / "post" / f"item_{b}" / "posterior" / f"sample_{s}.flac" for b in range(2) for s in range(S)]
    want += [tmp / "post" / f"item_{b}" / "posterior" / "std_spec.png" for b in range(2)]
    assert [str(p) for p in paths] == [str(p) for p in want] and all(p.exists() for p in want)
    waves, infos = FL.decode_files([str(p) for p in want[:2 * S]])
    assert all(w.shape == (L,) for w in waves) and all(float(w.abs().max()) > 0.99 for w in waves)
    assert not torch.equal(waves[0], waves[1])
    for p in want[2 * S:]:
        im = Image.open(p)
        assert im.mode == "P" and im.size == (1 + L // c["hop"], c["F"]) and np.asarray(im).max() == 253
    one = val.save_posterior_samples(torch.from_numpy(noisy[:1]), tmp / "one", n_samples=2, fmt="wav")
    assert [p.name for p in one] == ["sample_0.wav", "sample_1.wav", "std_spec.png"] and one[0].parent == tmp / "one" / "posterior"
