"""GPU: gap-constrained Griffin-Lim (csrc/gl_gap.hip through nppc_audio.inpainting.phase) against the fp64 restatement of its
contract (tests/gl_gap_ref.py).  The yardstick of every numeric comparison is the SAME restatement run in fp32 on the same
input: the kernel may be at most twice as far from fp64 as that, never a bound taken from the kernel's own output.
Error measures: relative L2 of the waveforms of a case; |d - d_ref| / target_norm, worst over the case."""
import functools

import numpy as np
import pytest
import torch

import gl_gap_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]
B, V = 3, 3


def PH():
    from nppc_audio.inpainting import phase
    return phase


@functools.lru_cache(maxsize=None)
def case_data(i, seed=0):
    return R.make_case(R.CASES[i], B=B, V=V, seed=seed)


@functools.lru_cache(maxsize=None)
def reference(i, n_iter, mu, fp32, seed=0):
    return R.run_case(case_data(i, seed), n_iter, mu, torch.float32 if fp32 else torch.float64)


def device_run(z, n_iter, mu, target_mag=None, init_phase=None, items=None, **kw):
    sel = slice(None) if items is None else items
    tm = (z["target_mag"] if target_mag is None else target_mag)[sel]
    ph = (z["init_phase"] if init_phase is None else init_phase)[sel]
    w, info = PH().griffin_lim_gap(tm.cuda(), z["known"][sel].cuda(), z["mask"][sel].cuda(), n_iter=n_iter, momentum=mu,
                                   init_phase=ph.cuda(), n_fft=z["n_fft"], hop_length=z["hop"], **kw)
    return w, info


def d_err(d, d_ref, tn):
    return float(((d.double().cpu() - d_ref).abs() / tn[..., None]).max()) if d_ref.numel() else 0.0


# ---- 1, 2: one step; eight steps; two steps with momentum -------------------------------------------------------------------
@pytest.mark.parametrize("n_iter,mu", [(1, 0.0), (8, 0.0), (2, 0.99)])
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_steps_against_the_restatement(i, n_iter, mu, record_err):
    z = case_data(i)
    W64, D64, N64 = reference(i, n_iter, mu, False)
    W32, D32, _ = reference(i, n_iter, mu, True)
    w, info = device_run(z, n_iter, mu)
    assert w.shape == (B, V, z["L"]) and info["inconsistency"].shape == (B, V, n_iter)
    assert int(info["status"].abs().sum()) == 0
    ew, yw = R.rel_l2(w.cpu(), W64), R.rel_l2(W32, W64)
    ed, yd = d_err(info["inconsistency"], D64, N64), d_err(D32, D64, N64)
    en = float(((info["target_norm"].cpu() - N64).abs() / N64).max())
    print(f"{IDS[i]} n_iter {n_iter} mu {mu}: wave {ew:.3e} (fp32 restatement {yw:.3e}), d {ed:.3e} ({yd:.3e}), norm {en:.3e}")
    record_err("wave", ew, 2 * yw)                             # kept with the session's other parity figures
    record_err("d", ed, 2 * yd)
    assert en <= 2 ** -23                                      # one fp32 rounding of each magnitude at most, summed in fp64


# ---- 3: fixed point -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_clean_phase_and_magnitude_are_a_fixed_point(i, record_err):
    z = case_data(i)
    tm = z["spec"].abs().float()[:, None].contiguous()
    ph = torch.angle(z["spec"]).float()[:, None].contiguous()
    W32, D32, N32 = R.run_case(z, 8, 0.0, torch.float32, tm, ph)
    w, info = device_run(z, 8, 0.0, tm, ph)
    clean = z["clean"][:, None].double()
    ew, yw = R.rel_l2(w.cpu(), clean), R.rel_l2(W32, clean)
    ed = float((info["inconsistency"].cpu() / info["target_norm"].cpu()[..., None]).max())
    yd = float((D32 / N32[..., None]).max())
    print(f"{IDS[i]} fixed point: wave {ew:.3e} (fp32 restatement {yw:.3e}), d / norm {ed:.3e} ({yd:.3e})")
    record_err("wave", ew, 2 * yw)
    record_err("d", ed, 2 * yd)


# ---- 4: the distance never grows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_distance_is_non_increasing(i):
    z = case_data(i, R.MONOTONE_SEED)
    _, D64, _ = reference(i, 16, 0.0, False, R.MONOTONE_SEED)
    assert bool((D64[..., 1:] <= D64[..., :-1] * (1 + 1e-9)).all())             # the input is one the restatement is monotone on
    _, info = device_run(z, 16, 0.0)
    d = info["inconsistency"].cpu()
    worst = float((d[..., 1:] / d[..., :-1]).max())
    print(f"{IDS[i]}: largest d[n+1] / d[n] = 1 {worst - 1:+.3e}")
    assert worst <= 1 + 1e-5 and bool((d[..., -1] < d[..., 0]).all())


# ---- 5: exact invariances -------------------------------------------------------------------------------------------------------
def same(a, b):
    wa, ia = a
    wb, ib = b
    return torch.equal(wa, wb) and torch.equal(ia["inconsistency"], ib["inconsistency"]) and \
        torch.equal(ia["target_norm"], ib["target_norm"])


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_exact_invariances(i):
    from nppc_audio import ops
    z = case_data(i)
    mu = 0.99 if i % 2 else 0.0
    full = device_run(z, 4, mu)
    assert same(full, device_run(z, 4, mu))                                                          # two runs
    for b in range(B):                                                                              # alone == in the batch
        w1, i1 = device_run(z, 4, mu, items=slice(b, b + 1))
        assert torch.equal(w1[0], full[0][b]) and torch.equal(i1["inconsistency"][0], full[1]["inconsistency"][b])
    perm = [2, 0, 1]
    wp, ip = device_run(z, 4, mu, items=perm)                                                       # a permuted batch
    assert torch.equal(wp, full[0][perm]) and torch.equal(ip["inconsistency"], full[1]["inconsistency"][perm])
    # NaN wherever the contract says nothing is read
    gap = (z["mask"] == 0)
    tm = z["target_mag"].clone()
    tm[(~gap)[:, None, None, :].expand_as(tm)] = float("nan")
    ph = z["init_phase"].clone()
    ph[(~gap)[:, None, None, :].expand_as(ph)] = float("nan")
    zz = dict(z)
    zz["known"] = z["known"].clone()
    zz["known"][gap[:, None, None, :].expand_as(zz["known"])] = float("nan")
    assert same(full, device_run(zz, 4, mu, tm, ph))
    # samples outside the gap's reach are ops.istft_any of the known spectrum, bit for bit
    known = ops.istft_any(z["known"][:, 0].contiguous().cuda(), z["known"][:, 1].contiguous().cuda(), z["n_fft"], z["hop"])
    for b in range(B):
        out = torch.from_numpy(~R.reach(z["mask"][b], z["n_fft"], z["hop"], z["L"])).cuda()
        assert bool(out.any())
        for v in range(V):
            assert torch.equal(full[0][b, v][out], known[b][out])
    assert not bool(torch.isnan(full[0]).any())


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_pc_route_against_the_general_route(i, record_err):
    z = case_data(i)
    K, A = 2, 3
    rng = np.random.default_rng(7)
    mag = z["spec"].abs().float().clamp_min(1e-6)
    mean, std = mag.log().mean(), mag.log().std()
    pred = ((mag.log() - mean) / std)[:, None].contiguous()
    pc = torch.from_numpy(rng.standard_normal((B, K, z["F"], z["T"])) * 0.1).float()
    alphas = torch.tensor([-1.5, 0.0, 2.0])
    ph0 = z["init_phase"][:, 0].contiguous()
    var, rest, info = PH().pc_audio_variations_blind(pred.cuda(), pc.cuda(), z["known"].cuda(), z["mask"].cuda(), alphas, mean.cuda(),
                                                     std.cuda(), n_iter=8, init_phase=ph0.cuda(), n_fft=z["n_fft"],
                                                     hop_length=z["hop"])
    assert var.shape == (B, K, A, z["L"]) and rest.shape == (B, z["L"]) and info["inconsistency"].shape == (B, K * A + 1, 8)
    # the expression in fp64, as the kernel forms it, rounded once: in fp32 the argument of exp alone is off by some 1e-6
    p64, d64 = pred.double(), pc.double()
    stack = torch.cat([(p64[:, :, None] + alphas.double()[None, None, :, None, None] * d64[:, :, None])
                       .reshape(B, K * A, z["F"], z["T"]), p64], 1)
    tm = torch.exp(stack * std.double() + mean.double()).float().contiguous()
    w, winfo = device_run(z, 8, 0.0, tm, ph0)
    W64, D64, N64 = R.run_case(z, 8, 0.0, torch.float64, tm, ph0)
    W32, D32, _ = R.run_case(z, 8, 0.0, torch.float32, tm, ph0)
    got = torch.cat([var.reshape(B, K * A, -1), rest[:, None]], 1)
    ew, yw = R.rel_l2(got.cpu(), w.cpu()), R.rel_l2(W32, W64)
    ed, yd = d_err(info["inconsistency"], winfo["inconsistency"].cpu(), N64), d_err(D32, D64, N64)
    print(f"{IDS[i]} pc route vs general route: wave {ew:.3e} (fp32 restatement vs fp64 {yw:.3e}), d {ed:.3e} ({yd:.3e})")
    record_err("wave", ew, 2 * yw)
    record_err("d", ed, 2 * yd)
    assert torch.equal(var[:, :, 1], rest[:, None].expand(B, K, -1))              # alpha = 0 of every direction is the prediction


# ---- 6: envelope ----------------------------------------------------------------------------------------------------------------
def test_item_over_the_span_cap_is_flagged_and_alone():
    from nppc_audio import ops
    P = PH()
    z = dict(case_data(0))
    mask = z["mask"].clone()
    mask[1] = 1
    mask[1, 2:2 + P.GL_MAX_SPAN_FRAMES - 1] = 0                                  # 31 gap frames + 2 neighbours: one over the cap
    z["mask"] = mask
    z["known"] = torch.stack([z["spec"].real, z["spec"].imag], 1).float() * mask[:, None, None, :]
    w, info = device_run(z, 4, 0.0)
    assert info["status"].cpu().tolist() == [0, 1, 0]
    assert bool(torch.isnan(w[1]).all()) and bool(torch.isnan(info["inconsistency"][1]).all())
    assert bool(torch.isnan(info["target_norm"][1]).all())
    w2, info2 = device_run(z, 4, 0.0, items=[0, 2])
    assert torch.equal(w[[0, 2]], w2) and torch.equal(info["inconsistency"][[0, 2]], info2["inconsistency"])
    assert info2["status"].cpu().tolist() == [0, 0] and not bool(torch.isnan(w2).any())
    mask[1] = 1
    mask[1, 2:2 + P.GL_MAX_SPAN_FRAMES - 2] = 0                                  # exactly at the cap
    z["known"] = torch.stack([z["spec"].real, z["spec"].imag], 1).float() * mask[:, None, None, :]
    w3, info3 = device_run(z, 1, 0.0)
    assert info3["status"].cpu().tolist() == [0, 0, 0] and bool(torch.isfinite(w3).all())
    # a lower cap of the caller's: the 17-frame gaps of this case need 19
    _, info4 = device_run(case_data(0), 1, 0.0, max_span=18)
    assert info4["status"].cpu().tolist() == [1, 1, 1]
    w5, info5 = device_run(case_data(0), 4, 0.0, max_span=19)
    w6, _ = device_run(case_data(0), 4, 0.0)
    assert info5["status"].cpu().tolist() == [0, 0, 0] and torch.equal(w5, w6)


def test_item_without_a_gap_and_zero_iterations():
    from nppc_audio import ops
    z = dict(case_data(3))
    mask = z["mask"].clone()
    mask[1] = 1
    z["mask"] = mask
    z["known"] = torch.stack([z["spec"].real, z["spec"].imag], 1).float() * mask[:, None, None, :]
    w, info = device_run(z, 4, 0.0)
    known = ops.istft_any(z["known"][:, 0].contiguous().cuda(), z["known"][:, 1].contiguous().cuda(), z["n_fft"], z["hop"])
    assert torch.equal(w[1], known[1][None].expand(V, -1))
    assert float(info["inconsistency"][1].abs().max()) == 0.0 and float(info["target_norm"][1].abs().max()) == 0.0
    assert info["status"].cpu().tolist() == [0, 0, 0] and float(info["target_norm"][0].min()) > 0
    for i in (1, 5, 9):
        zc = case_data(i)
        w0, info0 = device_run(zc, 0, 0.0)
        W64, _, N64 = reference(i, 0, 0.0, False)
        W32, _, _ = reference(i, 0, 0.0, True)
        assert info0["inconsistency"].shape == (B, V, 0)
        assert R.rel_l2(w0.cpu(), W64) <= 2 * R.rel_l2(W32, W64)
    # [B,F,T] magnitudes and a shared initial phase: V = 1
    zc = case_data(0)
    w1, _ = PH().griffin_lim_gap(zc["target_mag"][:, 0].cuda(), zc["known"].cuda(), zc["mask"].cuda(), n_iter=2,
                                 init_phase=zc["init_phase"][:, 0].cuda())
    w2, _ = device_run(zc, 2, 0.0)
    assert w1.shape == (B, 1, zc["L"]) and torch.equal(w1[:, 0], w2[:, 0])


def test_phase_advance_init_on_the_device():
    for i in (0, 1, 4, 6, 8, 9):
        z = case_data(i)
        got = PH().phase_advance_init(z["known"].cuda(), z["mask"].cuda(), z["n_fft"], z["hop"]).cpu().double()
        Kn = torch.complex(z["known"][:, 0].double(), z["known"][:, 1].double())
        for b in range(B):
            want = R.phase_advance_init(Kn[b], z["mask"][b], z["n_fft"], z["hop"])
            err = torch.angle(torch.polar(torch.ones_like(want), got[b] - want)).abs()
            # the phase leaves the device as fp32 in [-pi, pi]: half an ulp of pi is 1.2e-7, the fp64 sums add 1e-15
            assert float(err.max()) <= 2.5e-7, (i, b, float(err.max()))
            assert float(got[b][:, z["mask"][b] != 0].abs().max()) == 0.0 and float(got[b].abs().max()) <= 3.1415928


def deep_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(deep_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(deep_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


# ---- 7: validator ---------------------------------------------------------------------------------------------------------------
def test_validator_blind_phase(tmp_path, record_err):
    from nppc_audio.inpainting.validator import validator_nppc_model as Vm
    from test_inpaint_gpu import build_trainer, load
    from test_inpaint_validator_gpu import held_out
    zf, meta = load("inp_tiny")
    c = meta["config"]
    tr, _, _ = build_trainer(meta, "fp32", tmp_path, zf)
    ck = str(tmp_path / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    cfg = Vm.NPPCModelValidatorConfig(checkpoint_path=ck, save_dir=str(tmp_path / "val"),
                                      model_configuration=tr.config.nppc_model_configuration.model_dump())
    val = Vm.NPPCModelValidator(cfg)
    batch = held_out(zf, 3)
    net = val.model.pretrained_restoration_model.net
    kw = dict(n_mc_samples=8, n_components=c["K"], alphas=Vm.default_alphas(), n_fft=c["nfft"], hop_length=c["hop"])
    net.dropout_pass = 0
    base = val.validate_batch(*batch, **kw)
    net.dropout_pass = 0
    blind = val.validate_batch(*batch, phase="griffin_lim", gl_iters=8, **kw)
    assert set(base) == {"pc_directions", "pred_spec_mag_norm", "clean_spec_mag_norm", "mask", "mean", "std", "mc_dropout", "metrics",
                         "audio_variations", "clean_audio"}
    assert set(blind) - set(base) == {"audio_variations_blind", "restored_audio_blind", "phase_info"} and set(base) <= set(blind)
    for k, v in base.items():                                                    # everything else bit for bit
        assert deep_equal(v, blind[k]), k
    Bv, K, T = 3, c["K"], c["T"]
    L = R.natural_length(c["nfft"], c["hop"], T)
    assert blind["audio_variations_blind"].shape == (Bv, K, 13, L) and blind["restored_audio_blind"].shape == (Bv, L)
    assert bool(torch.isfinite(blind["audio_variations_blind"]).all()) and int(blind["phase_info"]["status"].sum()) == 0
    # the restored clip against the restatement on the validator's own tensors and the device's own initial phase
    masked, mask = batch[0], batch[1]
    ph0 = PH().phase_advance_init(masked.cuda(), mask.cuda(), c["nfft"], c["hop"]).cpu()
    M = torch.exp(blind["pred_spec_mag_norm"].cpu().double() * blind["std"].cpu().double() + blind["mean"].cpu().double())
    z = {"known": masked.float(), "mask": mask, "n_fft": c["nfft"], "hop": c["hop"], "L": L}
    W64, D64, N64 = R.run_case(z, 8, 0.0, torch.float64, M.float(), ph0[:, None])
    W32, D32, _ = R.run_case(z, 8, 0.0, torch.float32, M.float(), ph0[:, None])
    ew, yw = R.rel_l2(blind["restored_audio_blind"].cpu()[:, None], W64), R.rel_l2(W32, W64)
    print(f"validator restored_audio_blind: wave {ew:.3e} (fp32 restatement {yw:.3e})")
    record_err("wave", ew, 2 * yw)
