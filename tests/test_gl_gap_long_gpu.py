"""GPU: Griffin-Lim's tiled long-span path (csrc/gl_gap_long.hip through nppc_audio.inpainting.phase)
against the fp64 restatement of the contract (tests/gl_gap_ref.py, which has no span cap) and, bit for bit, against the
resident path.  Yardstick and error measures are those of tests/test_gl_gap_gpu.py: the kernel may be at most twice as far
from fp64 as the restatement run in fp32 on the same input."""
import functools

import numpy as np
import pytest
import torch

import gl_gap_ref as R

pytestmark = pytest.mark.gpu

B, V = 3, 3
LONG_CASES = [
    (255, 128, 64, [(10, 42)]),             # the reference yaml's 0.256 s: 33 frames
    (255, 128, 64, [(0, 40)]),              # clip edges
    (255, 128, 64, [(23, 63)]),
    (255, 128, 96, [(3, 6), (80, 85)]),     # few gap frames, a long bounding range
    (64, 16, 80, [(20, 60)]),               # r = 3, six neighbour frames, an odd number of live frames
    (512, 256, 48, [(6, 40)]),
    (510, 256, 48, [(6, 40)]),              # even n_fft: a Nyquist bin
]
LONG_IDS = [R.case_id(c) for c in LONG_CASES]
IDS = [R.case_id(c) for c in R.CASES]


def PH():
    from nppc_audio.inpainting import phase
    return phase


@functools.lru_cache(maxsize=None)
def long_case(i):
    return R.make_case(LONG_CASES[i], B=B, V=V)


@functools.lru_cache(maxsize=None)
def short_case(i):
    return R.make_case(R.CASES[i], B=B, V=V)


@functools.lru_cache(maxsize=None)
def reference(i, n_iter, mu, fp32):
    return R.run_case(long_case(i), n_iter, mu, torch.float32 if fp32 else torch.float64)


def device_run(z, n_iter, mu, target_mag=None, init_phase=None, items=None, **kw):
    sel = slice(None) if items is None else items
    tm = (z["target_mag"] if target_mag is None else target_mag)[sel]
    ph = (z["init_phase"] if init_phase is None else init_phase)[sel]
    return PH().griffin_lim_gap(tm.cuda(), z["known"][sel].cuda(), z["mask"][sel].cuda(), n_iter=n_iter, momentum=mu,
                                init_phase=ph.cuda(), n_fft=z["n_fft"], hop_length=z["hop"], **kw)


def d_err(d, d_ref, tn):
    return float(((d.double().cpu() - d_ref).abs() / tn[..., None]).max()) if d_ref.numel() else 0.0


def spans(z):
    """bounding range of each item's gap frames + the 2 r neighbour frames, as the span cap counts it"""
    r = -(-z["n_fft"] // z["hop"]) - 1
    out = []
    for m in z["mask"]:
        gap = np.flatnonzero(m.numpy() == 0)
        out.append(int(gap[-1] - gap[0] + 1 + 2 * r))
    return out


def resident_cap(z, n_iter, mu):
    return PH().gl_gap_shape(B, V, z["F"], z["T"], z["n_fft"], z["hop"], n_iter=n_iter, momentum=mu)["span_cap"]


def same(a, b):
    (wa, ia), (wb, ib) = a, b
    return torch.equal(wa, wb) and torch.equal(ia["inconsistency"], ib["inconsistency"]) and \
        torch.equal(ia["target_norm"], ib["target_norm"])


# ---- 1: against the fp64 restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter,mu", [(1, 0.0), (8, 0.0), (2, 0.99)])
@pytest.mark.parametrize("i", range(len(LONG_CASES)), ids=LONG_IDS)
def test_long_spans_against_the_restatement(i, n_iter, mu, record_err):
    z = long_case(i)
    cap = resident_cap(z, n_iter, mu)
    assert min(spans(z)) > cap, (spans(z), cap)                  # every item is one the default call flags
    W64, D64, N64 = reference(i, n_iter, mu, False)
    W32, D32, _ = reference(i, n_iter, mu, True)
    w, info = device_run(z, n_iter, mu, long_spans=True)
    assert w.shape == (B, V, z["L"]) and info["inconsistency"].shape == (B, V, n_iter)
    assert info["status"].cpu().tolist() == [0] * B
    ew, yw = R.rel_l2(w.cpu(), W64), R.rel_l2(W32, W64)
    ed, yd = d_err(info["inconsistency"], D64, N64), d_err(D32, D64, N64)
    en = float(((info["target_norm"].cpu() - N64).abs() / N64).max())
    print(f"{LONG_IDS[i]} n_iter {n_iter} mu {mu}: wave {ew:.3e} (fp32 restatement {yw:.3e}), d {ed:.3e} ({yd:.3e}), norm {en:.3e}")
    record_err("wave", ew, 2 * yw)
    record_err("d", ed, 2 * yd)
    assert en <= 2 ** -23


# ---- 2: the same bits as the resident path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_tiled_path_gives_the_resident_path_its_bits(i):
    z = short_case(i)
    for mu in (0.0, 0.99):                                        # every case through the shared momentum branch and without it
        w0, i0 = device_run(z, 4, mu)
        w1, i1 = device_run(z, 4, mu, long_spans="always")
        assert i0["status"].cpu().tolist() == [0] * B and i1["status"].cpu().tolist() == [0] * B
        diff = (w0 != w1)
        assert torch.equal(w0, w1), (mu, int(diff.sum()), float((w0 - w1).abs().max()))
        # folded across workgroups in another order: fewer than 2^17 non-negative fp64 terms, reordering error <= about 1.5e-11
        for k in ("inconsistency", "target_norm"):
            rel = float(((i0[k] - i1[k]).abs() / i0[k]).max())
            print(f"{IDS[i]} mu {mu} {k}: tiled vs resident {rel:.3e}")
            assert rel <= 1e-10, (mu, k, rel)
        # and through the router nothing here is long: the resident kernel's own results, info included
        assert same((w0, i0), device_run(z, 4, mu, long_spans=True)), mu


# ---- 3: one batch, both paths -------------------------------------------------------------------------------------------------
def test_mixed_batch_routes_by_item():
    z = dict(long_case(0))
    mask = torch.ones(B, z["T"])
    mask[0, 12:29] = 0                                             # 17 frames: within the cap
    mask[1, 10:43] = 0                                             # 33 frames: over it
    z["mask"] = mask                                               # item 2: no gap
    z["known"] = torch.stack([z["spec"].real, z["spec"].imag], 1).float() * mask[:, None, None, :]
    cap = resident_cap(z, 4, 0.99)
    assert 17 + 2 <= cap < 33 + 2
    for mu in (0.0, 0.99):
        w, info = device_run(z, 4, mu, long_spans=True)
        assert info["status"].cpu().tolist() == [0, 0, 0]
        w0, i0 = device_run(z, 4, mu, items=slice(0, 1))
        assert torch.equal(w[0], w0[0]) and torch.equal(info["inconsistency"][0], i0["inconsistency"][0])
        assert torch.equal(info["target_norm"][0], i0["target_norm"][0])
        w1, i1 = device_run(z, 4, mu, items=slice(1, 2), long_spans="always")
        assert torch.equal(w[1], w1[0]) and torch.equal(info["inconsistency"][1], i1["inconsistency"][0])
        assert torch.equal(info["target_norm"][1], i1["target_norm"][0])
        assert bool(torch.isfinite(w[1]).all()) and float(info["target_norm"][1].min()) > 0
        from nppc_audio import ops
        known = ops.istft_any(z["known"][:, 0].contiguous().cuda(), z["known"][:, 1].contiguous().cuda(), z["n_fft"], z["hop"])
        assert torch.equal(w[2], known[2][None].expand(V, -1))
        assert float(info["inconsistency"][2].abs().max()) == 0.0 and float(info["target_norm"][2].abs().max()) == 0.0
        wa, ia = device_run(z, 4, mu, long_spans="always")       # every item tiled: the same waveforms, item 2 included
        assert torch.equal(wa, w) and ia["status"].cpu().tolist() == [0, 0, 0]
        assert float(ia["inconsistency"][2].abs().max()) == 0.0 and float(ia["target_norm"][2].abs().max()) == 0.0
        # the default call on the same batch is what it was
        wd, idf = device_run(z, 4, mu)
        assert idf["status"].cpu().tolist() == [0, 1, 0]
        assert bool(torch.isnan(wd[1]).all()) and bool(torch.isnan(idf["inconsistency"][1]).all())
        assert bool(torch.isnan(idf["target_norm"][1]).all())
        assert torch.equal(wd[[0, 2]], w[[0, 2]]) and torch.equal(idf["inconsistency"][[0, 2]], info["inconsistency"][[0, 2]])
    # a cap of the caller's on the tiled path: an item over it is refused as the resident path refuses
    wl, il = device_run(z, 2, 0.0, long_spans=True, long_max_span=34)
    assert il["status"].cpu().tolist() == [0, 1, 0] and bool(torch.isnan(wl[1]).all()) and bool(torch.isfinite(wl[0]).all())
    wl, il = device_run(z, 2, 0.0, long_spans="always", long_max_span=35)
    assert il["status"].cpu().tolist() == [0, 0, 0] and torch.equal(wl, device_run(z, 2, 0.0, long_spans=True)[0])


# ---- 4: exact invariances on spans over the cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i,mu", [(0, 0.99), (1, 0.0), (3, 0.0), (4, 0.99)], ids=lambda x: LONG_IDS[x] if isinstance(x, int) else str(x))
def test_exact_invariances_over_the_cap(i, mu):
    z = long_case(i)
    full = device_run(z, 4, mu, long_spans=True)
    assert same(full, device_run(z, 4, mu, long_spans=True))                                        # two runs
    for b in range(B):                                                                              # alone == in the batch
        w1, i1 = device_run(z, 4, mu, items=slice(b, b + 1), long_spans=True)
        assert torch.equal(w1[0], full[0][b]) and torch.equal(i1["inconsistency"][0], full[1]["inconsistency"][b])
        assert torch.equal(i1["target_norm"][0], full[1]["target_norm"][b])
    perm = [2, 0, 1]
    wp, ip = device_run(z, 4, mu, items=perm, long_spans=True)                                      # a permuted batch
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
    assert same(full, device_run(zz, 4, mu, tm, ph, long_spans=True))
    # samples outside the gap's reach are ops.istft_any of the known spectrum, bit for bit
    from nppc_audio import ops
    known = ops.istft_any(z["known"][:, 0].contiguous().cuda(), z["known"][:, 1].contiguous().cuda(), z["n_fft"], z["hop"])
    for b in range(B):
        out = torch.from_numpy(~R.reach(z["mask"][b], z["n_fft"], z["hop"], z["L"])).cuda()
        assert bool(out.any())
        for v in range(V):
            assert torch.equal(full[0][b, v][out], known[b][out])
    assert not bool(torch.isnan(full[0]).any())


# ---- 5: fixed point -------------------------------------------------------------------------------------------------------------
def test_clean_phase_and_magnitude_are_a_fixed_point_on_a_40_frame_gap(record_err):
    z = R.make_case((255, 128, 64, [(10, 49)]), B=B, V=V)
    assert min(spans(z)) == 42 > resident_cap(z, 8, 0.0)
    tm = z["spec"].abs().float()[:, None].contiguous()
    ph = torch.angle(z["spec"]).float()[:, None].contiguous()
    W32, D32, N32 = R.run_case(z, 8, 0.0, torch.float32, tm, ph)
    w, info = device_run(z, 8, 0.0, tm, ph, long_spans=True)
    assert info["status"].cpu().tolist() == [0] * B
    clean = z["clean"][:, None].double()
    ew, yw = R.rel_l2(w.cpu(), clean), R.rel_l2(W32, clean)
    ed = float((info["inconsistency"].cpu() / info["target_norm"].cpu()[..., None]).max())
    yd = float((D32 / N32[..., None]).max())
    print(f"40-frame gap fixed point: wave {ew:.3e} (fp32 restatement {yw:.3e}), d / norm {ed:.3e} ({yd:.3e})")
    record_err("wave", ew, 2 * yw)
    record_err("d", ed, 2 * yd)


# ---- 6: the PC route --------------------------------------------------------------------------------------------------------------
def test_pc_route_equals_the_general_route_on_a_36_frame_gap():
    z = R.make_case((255, 128, 64, [(10, 45)]), B=B, V=V)
    assert min(spans(z)) == 38 > resident_cap(z, 4, 0.0)
    K, A = 2, 3
    rng = np.random.default_rng(7)
    mag = z["spec"].abs().float().clamp_min(1e-6)
    mean, std = mag.log().mean(), mag.log().std()
    pred = ((mag.log() - mean) / std)[:, None].contiguous()
    pc = torch.from_numpy(rng.standard_normal((B, K, z["F"], z["T"])) * 0.1).float()
    alphas = torch.tensor([-1.5, 0.0, 2.0])
    ph0 = z["init_phase"][:, 0].contiguous()
    kw = dict(n_iter=4, init_phase=ph0.cuda(), n_fft=z["n_fft"], hop_length=z["hop"])
    args = (pred.cuda(), pc.cuda(), z["known"].cuda(), z["mask"].cuda(), alphas, mean.cuda(), std.cuda())
    var, rest, info = PH().pc_audio_variations_blind(*args, long_spans=True, **kw)
    assert var.shape == (B, K, A, z["L"]) and rest.shape == (B, z["L"]) and info["inconsistency"].shape == (B, K * A + 1, 4)
    assert info["status"].cpu().tolist() == [0] * B
    # the expression in fp64, as the kernel forms it, rounded once
    p64, d64 = pred.double(), pc.double()
    stack = torch.cat([(p64[:, :, None] + alphas.double()[None, None, :, None, None] * d64[:, :, None])
                       .reshape(B, K * A, z["F"], z["T"]), p64], 1)
    tm = torch.exp(stack * std.double() + mean.double()).float().contiguous()
    w, winfo = device_run(z, 4, 0.0, tm, ph0, long_spans=True)
    got = torch.cat([var.reshape(B, K * A, -1), rest[:, None]], 1)
    assert torch.equal(got, w), float((got - w).abs().max())
    assert torch.equal(info["inconsistency"], winfo["inconsistency"]) and torch.equal(info["target_norm"], winfo["target_norm"])
    assert torch.equal(var[:, :, 1], rest[:, None].expand(B, K, -1))              # alpha = 0 of every direction is the prediction
    # the default call still refuses the batch
    _, _, dinfo = PH().pc_audio_variations_blind(*args, **kw)
    assert dinfo["status"].cpu().tolist() == [1] * B


# ---- 7: a whole recording ---------------------------------------------------------------------------------------------------------
def test_recording_restorer_with_a_4096_sample_gap(tmp_path):
    from nppc_audio.inpainting import restore as RS
    from oracle import weights as W
    L, WIN, XF, K = 48000, 8192, 64, 3
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(K), 41).items()}
    pre = "pretrained_restoration_model.net."
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, tmp_path / "restorer.pt")
    torch.save({"model_state_dict": wts}, tmp_path / "nppc.pt")
    mc = dict(pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
              pretrained_restoration_model_path=str(tmp_path / "restorer.pt"),
              audio_pc_wrapper_configuration=dict(n_dirs=K, model_configuration=dict(in_channels=2, out_channels=K,
                                                                                     precision="fp32")),
              device="cuda")
    cfg = dict(checkpoint_path=str(tmp_path / "nppc.pt"), model_configuration=mc, window_samples=WIN, n_fft=255, hop_length=128,
               gl_iters=4, crossfade_samples=XF)
    t = np.arange(L) / 16000.0
    x = 0.05 * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 330 * t + 1)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x = (x + 0.005 * np.random.default_rng(0).standard_normal(L)).astype(np.float32)
    s, e = 20000, 20000 + 4096
    x[s:e] = 0.0
    x = torch.from_numpy(x)
    rest = RS.RecordingRestorer(RS.RecordingRestorerConfig(long_gaps=True, **cfg))
    out = rest.restore(x, [(s, e)])
    y = out["restored"]
    assert y.shape == (L,) and bool(torch.isfinite(y).all()) and out["status"].cpu().tolist() == [0]
    lo, hi = out["windows"][0]["frames"]
    assert hi - lo + 1 + 2 > PH().gl_gap_shape(1, 1, 128, 1 + WIN // 128, length=WIN, n_iter=0)["span_cap"]
    assert torch.equal(y[:s - XF].cpu(), x[:s - XF]) and torch.equal(y[e + XF:].cpu(), x[e + XF:])
    assert float(y[s:e].abs().max()) > 0 and bool(torch.isfinite(out["inconsistency"]).all())
    again = rest.restore(x, [(s, e)])
    assert torch.equal(again["restored"], y) and torch.equal(again["inconsistency"], out["inconsistency"])
    va = rest.restore(x, [(s, e)], alphas=[-1.0, 0.5], variations="full")        # the PC route through the same option
    assert va["variations"].shape == (K, 2, L) and bool(torch.isfinite(va["variations"]).all()) and va["status"].cpu().tolist() == [0]
    with pytest.raises(ValueError, match="span cap"):
        RS.RecordingRestorer(RS.RecordingRestorerConfig(**cfg)).restore(x, [(s, e)])
