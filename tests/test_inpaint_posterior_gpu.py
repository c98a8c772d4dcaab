"""GPU: posterior samples of inpainted gaps (csrc/inpaint_posterior.hip, the third magnitude source of gl_gap_common.h and
nppc_audio.inpainting.posterior) against the restatement tests/inpaint_posterior_ref.py.

The yardstick of every numeric comparison is the restatement run in fp32 on the same input: the kernel may be at most twice
as far from the fp64 restatement as that.  Bit-for-bit anchors: one-hot coefficients against pc_audio_variations /
pc_audio_variations_blind."""
import functools

import numpy as np
import pytest
import torch

import gl_gap_ref as GR
import inpaint_posterior_ref as PR
import inpaint_validator_ref as VR

pytestmark = pytest.mark.gpu

ANCHOR_CONFIGS = [(255, 128, 37), (254, 127, 9), (512, 256, 9), (100, 25, 41)]
ANCHOR_K = [1, 5, 16]
B = 2


def IP():
    from nppc_audio.inpainting import posterior
    return posterior


@functools.lru_cache(maxsize=None)
def inputs(n_fft, T, K):
    """built like test_pc_variations_against_the_oracle_chain: |pred| <= 2, |pc| <= 0.6, clean_spec with exact +0 / -0 bins"""
    F = n_fft // 2 + 1
    g = torch.Generator().manual_seed(100 * K + T)
    pred = (torch.rand(B, 1, F, T, generator=g) * 2 - 1) * 2.0
    pc = (torch.rand(B, K, F, T, generator=g) * 2 - 1) * 0.6
    clean_norm = (torch.rand(B, 1, F, T, generator=g) * 2 - 1) * 4.0
    clean_spec = torch.randn(B, 2, F, T, generator=g)
    zero = torch.rand(B, 1, F, T, generator=g) < 0.05
    clean_spec = clean_spec * (~zero)
    re = clean_spec[:, 0]
    assert bool(((re == 0) & ~torch.signbit(re)).any()) and bool(((re == 0) & torch.signbit(re)).any())
    return {"pred": pred, "pc": pc, "clean_norm": clean_norm, "clean_spec": clean_spec, "mean": torch.tensor(-1.0),
            "std": torch.tensor(2.5)}


def coefficients(S, K, seed):
    """randn clamped to +-3, scaled by 1 / K"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, K, generator=g).clamp(-3.0, 3.0) / K


def check_bounded(d, z):
    """|pred| + sum_k |z_k| |w_k| <= 4 for every drawn z: the fp32 chain stays finite.  Checked before any launch."""
    worst = d["pred"].abs()[:, :, None] + (z.abs()[:, :, :, None, None] * d["pc"].abs()[:, None]).sum(2)[:, None]
    assert float(worst.max()) <= 4.0


def device_samples(d, z, n_fft, hop, **kw):
    c = lambda t: t.cuda()
    return IP().sample_waveforms(c(d["pred"]), c(d["pc"]), c(d["clean_spec"]), c(z), c(d["mean"]), c(d["std"]), n_fft=n_fft,
                                 hop_length=hop, **kw)


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, T, K, S, seed, fp32):
    d = inputs(n_fft, T, K)
    return PR.sample_waveforms(d["pred"], d["pc"], d["clean_spec"], coefficients(S, K, seed), d["mean"], d["std"], n_fft, hop,
                               torch.float32 if fp32 else torch.float64)


def worst(x, ref):
    """per waveform (last axis), relative to its own peak"""
    return float(((x.double() - ref.double()).abs().amax(-1) / ref.double().abs().amax(-1)).max())


# ---- 1: anchor --------------------------------------------------------------------------------------------------------------
def test_the_anchor_grid_takes_both_paths():
    paths = {(n_fft, K): IP().sample_shape(B, K * 13, K, T, n_fft, hop)["staged"] for n_fft, hop, T in ANCHOR_CONFIGS for K in ANCHOR_K}
    assert any(paths.values()) and not all(paths.values()), paths
    assert paths[(255, 16)] and not paths[(512, 16)] and not paths[(100, 16)]


@pytest.mark.parametrize("K", ANCHOR_K)
@pytest.mark.parametrize("n_fft,hop,T", ANCHOR_CONFIGS)
def test_one_hot_coefficients_give_the_pc_variations_bit_for_bit(n_fft, hop, T, K):
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas, pc_audio_variations
    d = inputs(n_fft, T, K)
    alphas = default_alphas()
    z = PR.one_hot_coefficients(B, K, alphas)
    check_bounded(d, z)
    c = lambda t: t.cuda()
    want, _ = pc_audio_variations(c(d["clean_norm"]), c(d["pred"]), c(d["pc"]), c(d["clean_spec"]), alphas, c(d["mean"]),
                                  c(d["std"]), n_fft=n_fft, hop_length=hop)
    L = VR.natural_length(n_fft, hop, T)
    staged = IP().sample_shape(B, K * 13, K, T, n_fft, hop)["staged"]
    got = device_samples(d, z, n_fft, hop)["samples"]
    assert got.shape == (B, K * 13, L) and bool(torch.isfinite(got).all())
    assert torch.equal(got.view(B, K, 13, L), want), f"staged={staged}"
    forced = device_samples(d, z, n_fft, hop, no_stage=True)["samples"]               # the other path, whatever the shape
    assert torch.equal(forced, got)


# ---- 2: random coefficients -------------------------------------------------------------------------------------------------
RANDOM = [(255, 128, 37, 5), (512, 256, 9, 16), (100, 25, 41, 1)]


@pytest.mark.parametrize("S", [1, 3, 9, 17])
@pytest.mark.parametrize("n_fft,hop,T,K", RANDOM)
def test_random_coefficients_against_the_restatement(n_fft, hop, T, K, S, record_err):
    d = inputs(n_fft, T, K)
    z = coefficients(S, K, 7)
    check_bounded(d, z)
    ref, f32 = reference(n_fft, hop, T, K, S, 7, False), reference(n_fft, hop, T, K, S, 7, True)
    assert bool(torch.isfinite(f32).all()) and bool(torch.isfinite(ref).all())
    got = device_samples(d, z, n_fft, hop)["samples"].cpu()
    assert got.shape == ref.shape
    err, yard = worst(got, ref), worst(f32, ref)
    print(f"samples {n_fft}/{hop} K={K} S={S}: kernel {err:.3e}, fp32 restatement {yard:.3e}")
    record_err("samples", err, 2 * yard)


# ---- 3: determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,T,K", RANDOM[:2])
def test_samples_are_repeatable_and_independent_of_batch_count_and_statistics(n_fft, hop, T, K):
    d = inputs(n_fft, T, K)
    z = coefficients(17, K, 7)
    check_bounded(d, z)
    a = device_samples(d, z, n_fft, hop)["samples"]
    assert torch.equal(a, device_samples(d, z, n_fft, hop)["samples"])                              # two runs
    one = {k: (v[1:] if v.dim() else v) for k, v in d.items()}
    assert torch.equal(device_samples(one, z[1:], n_fft, hop)["samples"][0], a[1])                  # alone == in the batch
    assert torch.equal(device_samples(d, z[:, :3].contiguous(), n_fft, hop)["samples"], a[:, :3])    # sample s does not depend on S
    full = device_samples(d, z, n_fft, hop, stats=True, spec_stats=True)                            # the statistics kernels
    assert torch.equal(full["samples"], a)
    # a length past the overlap-add is zero-filled, a shorter one is the head of the natural one
    L = VR.natural_length(n_fft, hop, T)
    longer = device_samples(d, z, n_fft, hop, length=L + 700)["samples"]
    assert torch.equal(longer[..., :L], a) and bool((longer[..., L + n_fft // 2:] == 0).all())
    assert torch.equal(device_samples(d, z, n_fft, hop, length=L - 300)["samples"], a[..., :L - 300])


# ---- 4: statistics ----------------------------------------------------------------------------------------------------------
def formula_bounds(y):
    """|device - host| bounds of mean and std by the stated formula, both evaluated from the same fp32 samples y [B,S,L].
    u = 2^-53.  A sum of S fp64 terms is within (S - 1) u sum|terms| of exact whatever its order, y^2 is exact in fp64, so with
    s1 = sum y, s2 = sum y^2 (device and host each carry their own error, hence the factors 2):
      mean:  2 (S u sum|y|) / S, then ONE fp32 rounding of the device's result: 2^-24 |mean| (+ 2^-149 where it is subnormal);
      var = (s2 - s1^2 / S) / (S - 1):  s2 is off by < S u s2, s1^2 / S by < 2 S u s1^2 / S, the subtraction and the division by
             u each: |dvar| < 2 (2 S u (s2 + s1^2 / S)) / (S - 1);
      std = sqrt(max(0, var)):  |sqrt a - sqrt b| <= min(sqrt|a - b|, |a - b| / sqrt(max(a, b))), then one fp32 rounding."""
    y = y.double()
    S = y.shape[1]
    u = 2.0 ** -53
    s1, s2, sa = y.sum(1), (y * y).sum(1), y.abs().sum(1)
    mean = s1 / S
    var = ((s2 - s1 * s1 / S) / (S - 1)).clamp_min(0.0)
    sd = var.sqrt()
    b_mean = 2 * S * u * sa / S + 2.0 ** -24 * mean.abs() * (1 + 2.0 ** -20) + 2.0 ** -149
    dvar = 4 * S * u * (s2 + s1 * s1 / S) / (S - 1)
    b_sd = torch.minimum(dvar.sqrt(), dvar / sd.clamp_min(1e-300)) + 2.0 ** -24 * sd * (1 + 2.0 ** -20) + 2.0 ** -149
    return mean, sd, b_mean, b_sd


@pytest.mark.parametrize("S", [2, 17])
@pytest.mark.parametrize("n_fft,hop,T,K", RANDOM[:2])
def test_statistics_against_the_restatement_and_the_stated_formula(n_fft, hop, T, K, S, record_err):
    d = inputs(n_fft, T, K)
    z = coefficients(S, K, 7)
    check_bounded(d, z)
    sh = IP().sample_shape(B, S, K, T, n_fft, hop, stats=3)
    assert sh["tiles"] == (1 if S == 2 else 3) and sh["work_bytes"] > 0                # S = 2 and more than one tile are covered
    out = device_samples(d, z, n_fft, hop, stats=True, spec_stats=True)
    only = device_samples(d, z, n_fft, hop, samples=False, stats=True, spec_stats=True)
    assert "samples" not in only and set(only) == {"mean", "std", "mag_mean", "mag_std"}
    for k in only:
        assert torch.equal(only[k], out[k]), k
    single = device_samples(d, z, n_fft, hop, samples=False, spec_stats=True)          # the magnitude kernel alone
    assert set(single) == {"mag_mean", "mag_std"} and torch.equal(single["mag_std"], out["mag_std"])
    # against the restatement
    ref, f32 = reference(n_fft, hop, T, K, S, 7, False), reference(n_fft, hop, T, K, S, 7, True)
    m64, s64 = PR.stats(ref)
    m32, s32 = PR.stats(f32)
    g64 = PR.sample_magnitudes(d["pred"], d["pc"], z, d["mean"], d["std"], torch.float64)
    g32 = PR.sample_magnitudes(d["pred"], d["pc"], z, d["mean"], d["std"], torch.float32)
    gm64, gs64 = PR.stats(g64)
    gm32, gs32 = PR.stats(g32)
    rel = lambda x, r: float(((x.double() - r).abs().flatten(1).amax(1) / r.abs().flatten(1).amax(1)).max())   # per item, to its peak
    for tag, got, want, yard in (("mean", out["mean"], m64, m32), ("std", out["std"], s64, s32),
                                 ("mag_mean", out["mag_mean"], gm64, gm32), ("mag_std", out["mag_std"], gs64, gs32)):
        e, y = rel(got.cpu(), want), rel(yard, want)
        print(f"{tag} {n_fft}/{hop} K={K} S={S}: kernel {e:.3e}, fp32 restatement {y:.3e}")
        record_err(tag, e, 2 * y)
    # against the stated formula on the device's own samples
    mean, sd, b_mean, b_sd = formula_bounds(out["samples"].cpu())
    assert bool(((out["mean"].cpu().double() - mean).abs() <= b_mean).all())
    assert bool(((out["std"].cpu().double() - sd).abs() <= b_sd).all())


# ---- 5: the Griffin-Lim route -----------------------------------------------------------------------------------------------
GK = 3
IDS = [GR.case_id(c) for c in GR.CASES]


@functools.lru_cache(maxsize=None)
def gl_inputs(i):
    z = GR.make_case(GR.CASES[i], B=B, V=1, seed=0)
    rng = np.random.default_rng(7)
    mag = z["spec"].abs().float().clamp_min(1e-6)
    mean, std = mag.log().mean(), mag.log().std()
    z["pred"] = ((mag.log() - mean) / std)[:, None].contiguous()
    z["pc"] = torch.from_numpy(rng.standard_normal((B, GK, z["F"], z["T"])) * 0.1).float()
    z["mean"], z["std"] = mean, std
    z["ph0"] = z["init_phase"][:, 0].contiguous()
    return z


def blind(z, coeffs, n_iter, **kw):
    c = lambda t: t.cuda()
    return IP().sample_waveforms_blind(c(z["pred"]), c(z["pc"]), c(z["known"]), c(z["mask"]), c(coeffs), c(z["mean"]), c(z["std"]),
                                       n_iter=n_iter, init_phase=c(z["ph0"]), n_fft=z["n_fft"], hop_length=z["hop"], **kw)


@pytest.mark.parametrize("i", range(len(GR.CASES)), ids=IDS)
def test_blind_one_hot_coefficients_give_the_blind_pc_variations_bit_for_bit(i):
    from nppc_audio.inpainting.phase import pc_audio_variations_blind
    z = gl_inputs(i)
    alphas = torch.tensor([-1.5, 0.0, 2.0])
    c = lambda t: t.cuda()
    var, rest, info = pc_audio_variations_blind(c(z["pred"]), c(z["pc"]), c(z["known"]), c(z["mask"]), alphas, c(z["mean"]),
                                                c(z["std"]), n_iter=8, init_phase=c(z["ph0"]), n_fft=z["n_fft"],
                                                hop_length=z["hop"])
    smp, rest2, info2 = blind(z, PR.one_hot_coefficients(B, GK, alphas), 8)
    assert smp.shape == (B, GK * 3, z["L"]) and bool(torch.isfinite(smp).all())
    assert torch.equal(smp, var.reshape(B, GK * 3, -1)) and torch.equal(rest2, rest)
    assert torch.equal(info2["status"], info["status"]) and int(info2["status"].abs().sum()) == 0
    assert torch.equal(info2["inconsistency"], info["inconsistency"]) and torch.equal(info2["target_norm"], info["target_norm"])
    tiled, trest, tinfo = blind(z, PR.one_hot_coefficients(B, GK, alphas), 8, long_spans="always")
    assert torch.equal(tiled, smp) and torch.equal(trest, rest) and int(tinfo["status"].abs().sum()) == 0


@pytest.mark.parametrize("n_iter", [1, 8])
@pytest.mark.parametrize("i", range(len(GR.CASES)), ids=IDS)
def test_blind_random_coefficients_against_the_restatement(i, n_iter, record_err):
    z = gl_inputs(i)
    S = 3
    coeffs = coefficients(S, GK, 11)
    args = (z["pred"], z["pc"], z["known"], z["mask"], coeffs, z["mean"], z["std"], z["ph0"], n_iter, 0.0, z["n_fft"], z["hop"], z["L"])
    W64, D64, N64 = PR.sample_waveforms_blind(*args, torch.float64)
    W32, D32, _ = PR.sample_waveforms_blind(*args, torch.float32)
    smp, rest, info = blind(z, coeffs, n_iter)
    got = torch.cat([smp, rest[:, None]], 1).cpu()
    assert got.shape == W64.shape and int(info["status"].abs().sum()) == 0
    d_err = lambda dd, ref: float(((dd.double().cpu() - ref).abs() / N64[..., None]).max())
    ew, yw = GR.rel_l2(got, W64), GR.rel_l2(W32, W64)
    ed, yd = d_err(info["inconsistency"], D64), d_err(D32, D64)
    print(f"{IDS[i]} n_iter {n_iter}: wave {ew:.3e} (fp32 restatement {yw:.3e}), d {ed:.3e} ({yd:.3e})")
    record_err("wave", ew, 2 * yw)
    record_err("d", ed, 2 * yd)
    zero, rest0, _ = blind(z, torch.zeros(B, 2, GK), n_iter)                           # z = 0 is the prediction
    assert torch.equal(zero[:, 0], rest0) and torch.equal(zero[:, 1], rest0) and torch.equal(rest0, rest)


def test_blind_item_over_the_span_cap_is_flagged_as_before():
    from nppc_audio.inpainting import phase as PH
    z = dict(gl_inputs(0))
    mask = z["mask"].clone()
    mask[1] = 1
    mask[1, 2:2 + PH.GL_MAX_SPAN_FRAMES - 1] = 0                                       # one frame over the cap
    z["mask"] = mask
    z["known"] = torch.stack([z["spec"].real, z["spec"].imag], 1).float() * mask[:, None, None, :]
    coeffs = coefficients(3, GK, 11)
    smp, rest, info = blind(z, coeffs, 2)
    assert info["status"].tolist() == [0, 1]
    assert bool(torch.isnan(smp[1]).all()) and bool(torch.isnan(rest[1]).all()) and bool(torch.isfinite(smp[0]).all())
    smp2, rest2, info2 = blind(z, coeffs, 2, long_spans=True)                          # the tiled path takes it
    assert info2["status"].tolist() == [0, 0] and bool(torch.isfinite(smp2).all()) and torch.equal(smp2[0], smp[0])


# ---- 6: end to end ----------------------------------------------------------------------------------------------------------
from test_restore_gpu import GAPS, HOP, K as RK, L as RL, NFFT, STARTS, WIN, XF, bits, dev_plan, recording, restorer, with_gaps  # noqa: E402,F401
from test_validator_png_gpu import FQ, KDIR, T64, inpainting_validator  # noqa: E402,F401
from test_validator_png_gpu import HOP as VHOP, NFFT as VNFFT  # noqa: E402


def window_tensors(restorer, xd):
    """restore()'s launch sequence up to the two nets, from the public functions (as test_restore_gpu.by_hand)"""
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import restore as RS
    from nppc_audio.inpainting.data import time_to_spec_mask
    from nppc_audio.inpainting.utils import preprocess_data
    gaps_d, starts_d = dev_plan(GAPS, STARTS)
    T, F = 1 + WIN // HOP, NFFT // 2 + 1
    gain = RS.recording_gain(xd, gaps_d, -25.0)
    xw, mt = RS.gather_windows(xd, gaps_d, starts_d, WIN, gain)
    mf = time_to_spec_mask(mt, T, WIN, NFFT, HOP, True)
    spec, masked = torch.empty(3, 2, F, T, device="cuda"), torch.empty(3, 2, F, T, device="cuda")
    H.call("nppc_stft_pair", xw, mf, spec, masked, 3, WIN, NFFT, HOP, H.stream())
    _, mask4, mn, mean, std = preprocess_data(masked, masked, mf, plot_mean_std=True)
    mask4 = mask4.contiguous()
    pc = restorer.model(mn, mask4)
    pred = restorer.model.get_pred_spec_mag_norm(mn, mask4)
    return dict(pred=pred, pc=pc, masked=masked, mf=mf, mean=mean, std=std, gain=gain, gaps_d=gaps_d, starts_d=starts_d)


def test_restore_with_samples_equals_the_hand_composed_sequence(restorer):
    import restore_ref as RR
    from nppc_audio.inpainting import restore as RS
    P = IP()
    x = torch.from_numpy(with_gaps(recording(), GAPS))
    plain = restorer.restore(x, GAPS)
    out = restorer.restore(x, GAPS, samples=3, seed=1, variations="full")
    assert set(out) - set(plain) == {"coeffs", "samples", "sample_windows", "sample_status"}
    assert out["samples"].shape == (3, RL) and out["sample_windows"].shape == (3, 3, WIN) and out["coeffs"].shape == (3, 3, RK)
    for k in plain:                                                           # 'restored' and the rest: the call without samples
        if torch.is_tensor(plain[k]):
            assert torch.equal(bits(out[k]) if plain[k].dtype == torch.float32 else out[k], bits(plain[k]) if plain[k].dtype == torch.float32 else plain[k]), k
    with torch.no_grad():
        w = window_tensors(restorer, x.cuda())
        z = P.draw_coefficients(3, 3, RK, seed=1, device="cuda")
        smp, _, info = P.sample_waveforms_blind(w["pred"], w["pc"], w["masked"], w["mf"], z, w["mean"], w["std"], n_iter=4,
                                                momentum=0.0, n_fft=NFFT, hop_length=HOP, length=WIN)
        hand = RS.splice_windows(x.cuda(), w["gaps_d"], w["starts_d"], smp, w["gain"], XF)
    assert torch.equal(out["coeffs"], z) and torch.equal(bits(out["samples"]), bits(hand))
    assert torch.equal(bits(out["sample_windows"]), bits(smp / w["gain"].float())) and int(out["sample_status"].sum()) == 0
    assert bool(torch.isfinite(out["samples"]).all())
    # samples outside the crossfaded gaps are the input's bits; inside, the samples differ from each other
    region = torch.from_numpy(RR.spliced_region(RL, GAPS, XF))
    for s in range(3):
        assert torch.equal(bits(out["samples"][s].cpu()[~region]), bits(x[~region]))
    assert not torch.equal(out["samples"][0], out["samples"][1])
    # coeffs = 0: every sample equals 'restored' where 'restored' is the prediction row of the same expression, i.e. in a
    # call with `alphas`.  Without `alphas` 'restored' has always come from torch's fp32 exp fed to griffin_lim_gap as a
    # target, and it has to stay that (checked above), so there the two differ in the last bits: measured 1.25e-8 at a
    # peak of 0.083 on this recording.
    zero = restorer.restore(x, GAPS, coeffs=torch.zeros(3, 2, RK), alphas=[0.5], variations="full")
    assert zero["variations"].shape == (RK, 1, RL) and zero["samples"].shape == (2, RL)
    for s in range(2):
        assert torch.equal(bits(zero["samples"][s]), bits(zero["restored"]))
    # windows only: no 'samples'; save_variations writes posterior/sample_<s> when the dict holds them
    win_only = restorer.restore(x, GAPS, samples=3, seed=1)
    assert "samples" not in win_only and torch.equal(bits(win_only["sample_windows"]), bits(out["sample_windows"]))


def test_restore_with_samples_at_another_rate_equals_down_sample_up(restorer, tmp_path):
    from nppc_audio import _hip as H
    from nppc_audio import flac as FL
    from nppc_audio import resample as RSM
    rate, n = 44100, 66150
    t = np.arange(n) / rate
    x = (0.05 * np.sin(2 * np.pi * 220 * t) + 0.02 * np.sin(2 * np.pi * 5000 * t)).astype(np.float32)
    gaps = [(30000, 32800)]
    x[gaps[0][0]:gaps[0][1]] = 0
    x = torch.from_numpy(x)
    out = restorer.restore(x, gaps, samples=2, seed=5, variations="full", sample_rate=rate)
    plain = restorer.restore(x, gaps, sample_rate=rate)
    assert out["samples"].shape == (2, n) and torch.equal(bits(out["restored"]), bits(plain["restored"]))
    inner = restorer.restore(RSM.resample(x.cuda(), rate, 16000, backend="hip"), out["gaps_model_rate"], samples=2, seed=5,
                             variations="full")
    assert torch.equal(out["coeffs"], inner["coeffs"])
    up = RSM.resample(inner["samples"], 16000, rate, backend="hip")
    merged = out["gaps_merged"]
    from nppc_audio.inpainting.restore import native_crossfade
    xf = native_crossfade(XF, rate, 16000)
    full = torch.empty(2, n, device="cuda")
    H.call("nppc_rec_splice", x.cuda(), n, torch.tensor(merged, dtype=torch.int64).cuda(), torch.zeros(len(merged), dtype=torch.int64).cuda(),
           len(merged), up, 0, up.stride(0), n, 2, xf, torch.ones(1, dtype=torch.float64).cuda(), full, H.stream())
    assert torch.equal(bits(out["samples"]), bits(full))
    outside = torch.ones(n, dtype=torch.bool)
    for s, e in merged:
        outside[s - xf:e + xf] = False
    assert torch.equal(bits(out["samples"][1].cpu()[outside]), bits(x[outside]))
    paths = restorer.save_variations(out, tmp_path / "rec")
    assert [str(p) for p in paths] == [str(tmp_path / "rec" / n_) for n_ in ("restored.flac", "posterior/sample_0.flac", "posterior/sample_1.flac")]
    back, infos = FL.decode_files(paths)
    want = FL.quantize_waves_host(torch.cat([out["restored"][None], out["samples"]]).cpu().numpy(), 16)
    for i in range(3):
        assert int(infos[i].sample_rate) == rate and np.array_equal(np.rint(back[i].cpu().numpy() * 32768).astype(np.int64), want[i])


def test_validate_batch_with_posterior_samples_and_its_files(inpainting_validator):
    from PIL import Image
    from nppc_audio import flac as FL
    from nppc_audio.spectrogram_png import Cell, Sheet, render_indices, windows_from_mask
    V, val, batch, tmp = inpainting_validator
    kw = dict(n_mc_samples=4, n_components=KDIR, ragged_gaps=True, n_fft=VNFFT, hop_length=VHOP)
    net = val.model.pretrained_restoration_model.net
    net.dropout_pass = 0
    plain = val.validate_batch(*batch, **kw)
    net.dropout_pass = 0
    out = val.validate_batch(*batch, posterior_samples=4, posterior_seed=3, **kw)
    assert set(out) - set(plain) == {"posterior"} and set(out["posterior"]) == {"coeffs", "samples", "std", "mag_std"}
    for k in ("pc_directions", "pred_spec_mag_norm", "clean_spec_mag_norm", "mask", "mean", "std"):
        assert torch.equal(out[k], plain[k]), k
    assert out["metrics"] == plain["metrics"]
    Lc = VR.natural_length(VNFFT, VHOP, T64)
    post = out["posterior"]
    assert post["coeffs"].shape == (2, 4, KDIR) and post["samples"].shape == (2, 4, Lc) and post["std"].shape == (2, Lc)
    assert post["mag_std"].shape == (2, FQ, T64) and bool(torch.isfinite(post["samples"]).all())
    assert torch.equal(post["coeffs"], IP().draw_coefficients(2, 4, KDIR, seed=3, device="cuda"))
    gap = (batch[1] == 0).cuda()
    # the directions are zero on known frames: all S magnitudes m are equal there, and the sum formula leaves at most its own
    # rounding, |var| <= 4 S u (s2 + s1^2 / S) / (S - 1) = 8 S^2 u m^2 / (S - 1) with u = 2^-53 (formula_bounds above)
    m = torch.exp(out["pred_spec_mag_norm"][:, 0].double() * out["std"].double() + out["mean"].double())
    lim = (8 * 4 * 4 * 2.0 ** -53 / 3) ** 0.5 * m * (1 + 1e-6)
    known = ~gap[:, None, :].expand(2, FQ, T64)
    assert bool((post["mag_std"].double() <= lim)[known].all()) and bool((post["mag_std"].double() > 100 * lim)[~known].any())
    net.dropout_pass = 0
    both = val.validate_batch(*batch, posterior_samples=4, posterior_seed=3, phase="griffin_lim", gl_iters=2, **kw)
    assert set(both["posterior"]) == {"coeffs", "samples", "std", "mag_std", "samples_blind", "phase_info"}
    assert both["posterior"]["samples_blind"].shape == (2, 4, Lc) and torch.equal(both["posterior"]["samples"], post["samples"])
    for bad in (1, 0, 4097, 2.5, True):
        with pytest.raises(ValueError, match="posterior_samples"):
            val.validate_batch(*batch, posterior_samples=bad, **kw)
    with pytest.raises(ValueError, match="posterior_samples=S"):
        V.save_posterior_samples(plain, tmp / "none")
    # the files
    paths = V.save_posterior_samples(both, tmp / "post", first_index=2)
    names = [f"sample_{s}.flac" for s in range(4)] + [f"sample_{s}_blind.flac" for s in range(4)]
    want = [tmp / "post" / f"sample_{2 + b}" / "posterior" / f"sample_{s}.flac" for b in range(2) for s in range(4)]
    want += [tmp / "post" / f"sample_{2 + b}" / "posterior" / f"sample_{s}_blind.flac" for b in range(2) for s in range(4)]
    want += [tmp / "post" / f"sample_{2 + b}" / "posterior" / "std_spec.png" for b in range(2)]
    assert [str(p) for p in paths] == [str(p) for p in want] and all(p.exists() for p in want) and len(names) == 8
    back, _ = FL.decode_files(paths[:16])
    written = torch.cat([both["posterior"]["samples"].reshape(8, Lc), both["posterior"]["samples_blind"].reshape(8, Lc)])
    q = FL.quantize_waves_host(written.cpu().numpy(), 16)
    for i in range(16):
        assert np.array_equal(np.rint(back[i].cpu().numpy() * 32768).astype(np.int64), q[i]), i
    planes = V.posterior_std_planes(both)
    win = windows_from_mask(both["mask"][:, 0, 0, :])
    idx = render_indices(planes, [Sheet(b, [[Cell(p=0, g="db", markers=True)]], sx=2, sy=2) for b in range(2)], win)
    for b in range(2):
        im = Image.open(paths[16 + b])
        t0, t1 = int(win[b, 0]), int(win[b, 1])
        assert im.mode == "P" and im.size == ((t1 - t0) * 2, FQ * 2)
        assert np.array_equal(np.asarray(im), np.asarray(idx[b].cpu() if torch.is_tensor(idx[b]) else idx[b])[:FQ * 2, :(t1 - t0) * 2])


def test_sampler_runs_both_routes_on_a_loaded_model(inpainting_validator):
    V, val, batch, tmp = inpainting_validator
    masked, mask, clean = batch
    s = IP().InpaintingPosteriorSampler(model=val.model)
    cfg = dict(n_fft=VNFFT, hop_length=VHOP)
    out = s.sample(masked, mask, clean, n_samples=4, seed=3, stats=True, spec_stats=True, **cfg)
    assert set(out) == {"coeffs", "samples", "mean", "std", "mag_mean", "mag_std"}
    val.model.pretrained_restoration_model.net.dropout_pass = 0
    ref = val.validate_batch(masked, mask, clean, n_mc_samples=4, n_components=KDIR, ragged_gaps=True, posterior_samples=4,
                             posterior_seed=3, **cfg)["posterior"]
    for k in ("coeffs", "samples", "std", "mag_std"):                       # the same launches on the same tensors
        assert torch.equal(out[k], ref[k]), k
    given = s.sample(masked, mask, clean, coeffs=out["coeffs"].cpu(), **cfg)
    assert set(given) == {"coeffs", "samples"} and torch.equal(given["samples"], out["samples"])
    blind = s.sample(masked, mask, n_samples=3, seed=3, phase="griffin_lim", gl_iters=2, stats=True, spec_stats=True, **cfg)
    assert set(blind) == {"coeffs", "samples", "restored", "phase_info", "mean", "std", "mag_mean", "mag_std"}
    Lc = VR.natural_length(VNFFT, VHOP, T64)
    assert blind["samples"].shape == (2, 3, Lc) and blind["restored"].shape == (2, Lc) and bool(torch.isfinite(blind["samples"]).all())
    assert torch.equal(blind["std"], blind["samples"].std(1)) and int(blind["phase_info"]["status"].abs().sum()) == 0
    zero = s.sample(masked, mask, coeffs=torch.zeros(2, 2, KDIR), phase="griffin_lim", gl_iters=2, **cfg)
    assert torch.equal(zero["samples"][:, 0], zero["restored"]) and torch.equal(zero["restored"], blind["restored"])
    with pytest.raises(ValueError, match="at least 2"):
        s.sample(masked, mask, n_samples=1, phase="griffin_lim", stats=True, **cfg)
