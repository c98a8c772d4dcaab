"""GPU: the TSSE channel attention of the full-band front (csrc/spec.hip) against fp64 references built from the oracle, and
its ragged entry (nppc_tsse_fwd_maps_ragged, the same kernels with per-item frame counts) against the uniform one bit for bit.

nppc_tsse_fwd_maps: per map, pad the look-ahead with zeros -> laplace_norm -> oracle.nppc_ref.tsse (attention_model.py:78-98),
its scale and saved intermediates, and the scaled map transposed into the TCN input X0 [3][B][Tp][ld] (map j = m*3 + z lands
in branch z at columns [m*C, (m+1)*C)).  nppc_tsse_bwd_maps: the gradients of all attention parameters of the three branches
for a given dX0, against fp64 autograd.  The kernel computes the conv means from row sums minus prefix and suffix sums and
sizes its workgroup as C rounded up to 64 (at most 1024): the shapes below sit at those edges."""
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

from oracle import nppc_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
KS = (3, 5, 10)
CONVS = ("smallConv1d", "middleConv1d", "largeConv1d")


def rel(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def _layout(C):
    """offsets of the attention parameters inside one branch's block (the kernel's flat layout), block stride sW"""
    C2 = C // 2
    shapes = dict(cw0=C * KS[0], cb0=C, cw1=C * KS[1], cb1=C, cw2=C * KS[2], cb2=C, fcw=3, fcb=1, w1=C2 * C, b1=C2, w2=C * C2,
                  b2=C)
    offs, o = {}, 0
    for k, n in shapes.items():
        offs[k] = o
        o += (n + 3) // 4 * 4 + 4                  # a gap after every parameter: never read, never written
    return shapes, offs, o + 16


def _params(flat, z, C, sW, offs):
    """branch z of the flat fp64 buffer as the oracle's parameter dict (prefix "att")"""
    C2 = C // 2
    v = lambda k, n, shp: flat[z * sW + offs[k]: z * sW + offs[k] + n].view(*shp)
    P = {}
    for i, nm in enumerate(CONVS):
        P[f"att.{nm}.0.weight"] = v(f"cw{i}", C * KS[i], (C, 1, KS[i]))
        P[f"att.{nm}.0.bias"] = v(f"cb{i}", C, (C,))
    P["att.feature_concate_fc.weight"] = v("fcw", 3, (1, 3))
    P["att.feature_concate_fc.bias"] = v("fcb", 1, (1,))
    P["att.fc1.weight"] = v("w1", C2 * C, (C2, C))
    P["att.fc1.bias"] = v("b1", C2, (C2,))
    P["att.fc2.weight"] = v("w2", C * C2, (C, C2))
    P["att.fc2.bias"] = v("b2", C, (C,))
    return P


def _tsse_parts(xn, P):
    """the intermediates of oracle tsse (attention_model.py:78-98) on the normalised padded map xn [B,C,Tp]"""
    C = xn.shape[1]
    pre = torch.stack([Fn.conv1d(xn, P[f"att.{nm}.0.weight"], P[f"att.{nm}.0.bias"], groups=C).mean(dim=2) for nm in CONVS], 2)
    sq = Fn.linear(torch.relu(pre), P["att.feature_concate_fc.weight"], P["att.feature_concate_fc.bias"])[..., 0]
    h1 = torch.relu(Fn.linear(sq, P["att.fc1.weight"], P["att.fc1.bias"]))
    sg = torch.sigmoid(Fn.linear(h1, P["att.fc2.weight"], P["att.fc2.bias"]))
    return pre, sq, h1, sg


def _maps(nm, B, C, T, seed, ri_mean):
    """3 * nm maps [B,C,T] (j = m*3 + z): a magnitude-like map with a small mean (1/(mu + 1e-5) is large and sensitive) and
    real / imaginary-like maps of mean +-ri_mean (ri_mean = 1e-3: ~1/500 of their spread)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(3 * nm):
        z = j % 3
        x = torch.randn(B, C, T, generator=g) * (0.3 if z == 0 else 0.5)
        x = x - x.mean(dim=(1, 2), keepdim=True) + (0.02 if z == 0 else (ri_mean if j % 2 else -0.8 * ri_mean))
        out.append(x.contiguous())
    return out


def _setup(nm, B, C, T, seed, ri_mean=1e-3):
    C2 = C // 2
    shapes, offs, sW = _layout(C)
    g = torch.Generator().manual_seed(seed + 1)
    flat = torch.full((3 * sW,), NAN, dtype=torch.float64)
    scl = dict(cw0=0.5 / KS[0], cw1=0.5 / KS[1], cw2=0.5 / KS[2], cb0=0.2, cb1=0.2, cb2=0.2, fcw=0.6, fcb=0.2,
               w1=1.0 / C ** 0.5, b1=0.2, w2=1.0 / max(C2, 1) ** 0.5, b2=0.2)
    for z in range(3):
        for k, n in shapes.items():
            flat[z * sW + offs[k]: z * sW + offs[k] + n] = torch.randn(n, generator=g).double() * scl[k]
    flat = flat.float().double()                                      # the values the kernel sees
    return shapes, offs, sW, flat, _maps(nm, B, C, T, seed, ri_mean)


def _reference(maps, flat, nm, B, C, T, la, sW, offs):
    """per map slot (z, m): ns [B], pre [B,C,3], sq [B,C], h1 [B,C2], sg [B,C], and X0 rows = (x * ns * sg)[..., :T]"""
    out = {}
    for z in range(3):
        P = _params(flat, z, C, sW, offs)
        for m in range(nm):
            xp = Fn.pad(maps[m * 3 + z].double(), [0, la])             # look-ahead zeros (fullsubnet_plus.py:158)
            xn = R.laplace_norm(xp)
            ns = 1.0 / (xp.mean(dim=(1, 2)) + 1e-5)
            pre, sq, h1, sg = _tsse_parts(xn, P)
            y = R.tsse(xn, P, "att")
            out[z, m] = dict(ns=ns, pre=pre, sq=sq, h1=h1, sg=sg, scale=ns[:, None] * sg, y=y[..., :T])
    return out


def _launch_fwd(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs):
    from nppc_audio import _hip as H
    C2 = C // 2
    P = lambda k: flat_d[offs[k]:]
    rs = torch.full((3 * nm, B, C), NAN, dtype=torch.float64, device="cuda")
    scale = torch.full((3, nm, B, C), NAN, device="cuda")
    sv = {k: torch.full((3, nm, B, *shp), NAN, device="cuda")
          for k, shp in (("ns", ()), ("pre", (C, 3)), ("sq", (C,)), ("h1", (C2,)), ("sg", (C,)))}
    X0 = torch.full((3, B, Tp, ld), NAN, dtype=H.dtype_of(prec), device="cuda")
    H.call("nppc_tsse_fwd_maps", prec, H.ptr_array(maps_d), 3 * nm, rs, P("cw0"), P("cb0"), P("cw1"), P("cb1"), P("cw2"), P("cb2"),
           *KS, P("fcw"), P("fcb"), P("w1"), P("b1"), P("w2"), P("b2"), sW, scale, sv["ns"], sv["pre"], sv["sq"], sv["h1"],
           sv["sg"], X0, B * Tp * ld, B, C, T, la, Tp, ld, H.stream())
    return rs, scale, sv, X0


# (prec, nm, B, C, T, la): C around the 64-thread rounding and at TSSE_MAXC; T = the largest kernel size, just above, well above
ATT_CASES = [
    (1, 1, 1, 2, 10, 0),
    (0, 2, 3, 2, 70, 2),
    (1, 2, 3, 63, 11, 2),
    (0, 1, 1, 64, 70, 0),
    (1, 1, 3, 65, 10, 2),
    (0, 2, 3, 65, 70, 2),
    (0, 2, 1, 257, 11, 0),
    (1, 1, 3, 257, 70, 2),
    (0, 1, 3, 1024, 10, 2),
    (1, 2, 1, 1024, 70, 0),
]


@pytest.mark.parametrize("prec,nm,B,C,T,la", ATT_CASES)
def test_tsse_forward_matches_reference(prec, nm, B, C, T, la, record_err):
    from nppc_audio import _hip as H
    _, offs, sW, flat, maps = _setup(nm, B, C, T, seed=C + T + la)
    Tp, ld = T + la + 3, nm * C + 5                                   # padded rows and columns: the kernel leaves them alone
    maps_d = [m.cuda() for m in maps]
    flat_d = flat.float().cuda()
    rs, scale, sv, X0 = _launch_fwd(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs)
    torch.cuda.synchronize()
    ref = _reference(maps, flat, nm, B, C, T, la, sW, offs)
    for z in range(3):
        for m in range(nm):
            assert rel(rs[m * 3 + z], maps[m * 3 + z].double().sum(-1)) < 1e-12
    stack = lambda k: torch.stack([torch.stack([ref[z, m][k] for m in range(nm)]) for z in range(3)])
    for k, tol in (("ns", 1e-6), ("pre", 2e-5), ("sq", 2e-5), ("h1", 1e-4), ("sg", 1e-4)):
        assert bool(torch.isfinite(sv[k]).all()), k
        record_err(k, rel(sv[k], stack(k)), tol)
    record_err("scale", rel(scale, stack("scale")), 1e-4)
    want = torch.full((3, B, Tp, ld), NAN, dtype=torch.float64)
    for z in range(3):
        for m in range(nm):
            want[z, :, :T, m * C:(m + 1) * C] = ref[z, m]["y"].permute(0, 2, 1)
    got = X0.double().cpu()
    valid = ~torch.isnan(want)
    assert torch.equal(torch.isnan(got), ~valid)                       # exactly the valid rows / columns are written
    record_err("X0", rel(got[valid], want[valid]), 1e-4 if prec == 1 else 1e-2)
    # one writer and a fixed order for every sum: a second launch gives the same bits
    rs2, scale2, sv2, X02 = _launch_fwd(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs)
    torch.cuda.synchronize()
    assert torch.equal(rs2, rs) and torch.equal(scale2, scale) and torch.equal(X02.isnan(), X0.isnan())
    assert torch.equal(X02[valid.cuda()], X0[valid.cuda()])
    for k in sv:
        assert torch.equal(sv2[k], sv[k]), k


def test_tsse_forward_argument_guards():
    """the conv means need every kernel size to fit in the unpadded map; one workgroup holds at most 1024 channels"""
    from nppc_audio import _hip as H
    for C, T, msg in ((33, 9, "unsupported"), (1025, 11, "bad argument")):
        _, offs, sW, flat, maps = _setup(1, 1, C, T, seed=3)
        with pytest.raises(RuntimeError, match=msg):
            _launch_fwd(1, [m.cuda() for m in maps], flat.float().cuda(), 1, 1, C, T, 2, T + 2, C, sW, offs)


def _launch_fwd_ragged(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs, frames):
    """nppc_tsse_fwd_maps_ragged into NaN-filled buffers; frames: the items' frame counts (None: a null pointer)"""
    from nppc_audio import _hip as H
    P = lambda k: flat_d[offs[k]:]
    rs = torch.full((3 * nm, B, C), NAN, dtype=torch.float64, device="cuda")
    scale = torch.full((3, nm, B, C), NAN, device="cuda")
    X0 = torch.full((3, B, Tp, ld), NAN, dtype=H.dtype_of(prec), device="cuda")
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
    H.call("nppc_tsse_fwd_maps_ragged", prec, H.ptr_array(maps_d), 3 * nm, rs, P("cw0"), P("cb0"), P("cw1"), P("cb1"), P("cw2"),
           P("cb2"), *KS, P("fcw"), P("fcb"), P("w1"), P("b1"), P("w2"), P("b2"), sW, scale, X0, B * Tp * ld, fr, B, C, T, la, Tp,
           ld, H.stream())
    return rs, scale, X0


# (prec, nm, B, C, T, la, frames): 10 = the largest kernel size is the shortest legal item; C at the 64-thread rounding (2, 65)
# and at TSSE_MAXC
RAGGED_CASES = [
    (0, 2, 3, 65, 70, 2, [70, 10, 37]),
    (1, 2, 3, 65, 70, 2, [70, 10, 37]),
    (1, 1, 3, 2, 11, 0, [11, 10, 10]),
    (0, 1, 3, 1024, 12, 2, [12, 10, 11]),
]


@pytest.mark.parametrize("prec,nm,B,C,T,la,frames", RAGGED_CASES)
def test_tsse_forward_ragged_is_the_uniform_entry_per_item(prec, nm, B, C, T, la, frames):
    """The ragged entry (the RAGGED instantiations of the uniform kernels) against the uniform entry, bit for bit: with every
    item full length it is the uniform call; item b of a ragged batch is the uniform call on that item alone with its maps
    cropped to T_b frames; X0 rows T_b <= t < Tp are written as zero."""
    _, offs, sW, flat, maps = _setup(nm, B, C, T, seed=C + T + la)
    Tp, ld, W = T + la + 3, nm * C + 5, nm * C
    maps_d = [m.cuda() for m in maps]
    flat_d = flat.float().cuda()
    # 1: all frames = T
    rs_u, scale_u, _, X0_u = _launch_fwd(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs)
    rs_f, scale_f, X0_f = _launch_fwd_ragged(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs, [T] * B)
    assert torch.equal(rs_f, rs_u) and torch.equal(scale_f, scale_u)
    assert torch.equal(X0_f[:, :, :T, :W], X0_u[:, :, :T, :W]) and not bool(X0_u[:, :, :T, :W].isnan().any())
    assert float(X0_f[:, :, T:, :W].float().abs().max()) == 0.0
    # 2, 3: a ragged batch, item by item
    rs, scale, X0 = _launch_fwd_ragged(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs, frames)
    assert bool(X0[..., W:].isnan().all())                              # the pad columns are the caller's
    for b, Tb in enumerate(frames):
        alone = [m[b:b + 1, :, :Tb].contiguous() for m in maps_d]
        rs_a, scale_a, _, X0_a = _launch_fwd(prec, alone, flat_d, nm, 1, C, Tb, la, Tp, ld, sW, offs)
        assert torch.equal(rs[:, b], rs_a[:, 0]), b
        assert torch.equal(scale[:, :, b], scale_a[:, :, 0]), b
        assert torch.equal(X0[:, b, :Tb, :W], X0_a[:, 0, :Tb, :W]) and not bool(X0_a[:, 0, :Tb, :W].isnan().any()), b
        assert bool((X0[:, b, Tb:, :W] == 0).all()), b


def test_tsse_forward_ragged_argument_guards():
    """the uniform entry's guards, and a null frames pointer"""
    for C, T, frames, msg in ((33, 9, [9], "unsupported"), (1025, 11, [11], "bad argument"), (33, 11, None, "bad argument")):
        _, offs, sW, flat, maps = _setup(1, 1, C, T, seed=3)
        with pytest.raises(RuntimeError, match=msg):
            _launch_fwd_ragged(1, [m.cuda() for m in maps], flat.float().cuda(), 1, 1, C, T, 2, T + 2, C, sW, offs, frames)


@pytest.mark.parametrize("prec,nm,B,C,T,la", ATT_CASES)
def test_tsse_backward_matches_autograd(prec, nm, B, C, T, la, record_err):
    """the parameter gradients of all three branches for a random dX0 (padding rows and columns NaN: never read), ADDED to
    the gradient buffers; bit-identical over two launches (no atomics, fixed summation order).  The maps have means of 0.02
    here: at ns ~ 1e3 the sigmoid of a whole branch saturates, and its gradient s (1 - s) keeps only the fp32 rounding of
    1 + exp(-a) (~1e-3 relative, as in any fp32 implementation); at ns ~ 50 every branch has channels off saturation"""
    from nppc_audio import _hip as H
    shapes, offs, sW, flat, maps = _setup(nm, B, C, T, seed=7 * C + T + la, ri_mean=0.02)
    Tp, ld = T + la + 3, nm * C + 5
    dt = H.dtype_of(prec)
    maps_d = [m.cuda() for m in maps]
    flat_d = flat.float().cuda()
    rs, _, sv, _ = _launch_fwd(prec, maps_d, flat_d, nm, B, C, T, la, Tp, ld, sW, offs)
    g = torch.Generator().manual_seed(C + 11 * T)
    dX0 = torch.full((3, B, Tp, ld), NAN)
    dX0[:, :, :T, :nm * C] = torch.randn(3, B, T, nm * C, generator=g)
    dX0 = dX0.to(dt)
    dX0_d = dX0.cuda()
    nW = ctypes.c_long()
    H.call("nppc_tsse_bwd_ws_elems", 3 * nm, B, C, *KS, ctypes.byref(nW))
    P = lambda k: flat_d[offs[k]:]

    def grads():
        G = torch.full((3 * sW,), NAN, device="cuda")
        for z in range(3):
            for k, n in shapes.items():
                G[z * sW + offs[k]: z * sW + offs[k] + n] = 0.0
        ws = torch.full((nW.value,), NAN, device="cuda")             # nothing may rely on a cleared workspace
        Gp = lambda k: G[offs[k]:]
        H.call("nppc_tsse_bwd_maps", prec, dX0_d, B * Tp * ld, H.ptr_array(maps_d), 3 * nm, rs, P("cw0"), P("cw1"), P("cw2"), *KS,
               P("fcw"), P("w1"), P("w2"), sW, sv["ns"], sv["pre"], sv["sq"], sv["h1"], sv["sg"], ws, Gp("cw0"), Gp("cb0"),
               Gp("cw1"), Gp("cb1"), Gp("cw2"), Gp("cb2"), Gp("fcw"), Gp("fcb"), Gp("w1"), Gp("b1"), Gp("w2"), Gp("b2"), B, C, T,
               la, Tp, ld, H.stream())
        return G

    G1 = grads()
    G2 = grads()
    torch.cuda.synchronize()
    fr = flat.clone().requires_grad_(True)
    loss = 0.0
    for z in range(3):
        Pz = _params(fr, z, C, sW, offs)
        for m in range(nm):
            xn = R.laplace_norm(Fn.pad(maps[m * 3 + z].double(), [0, la]))
            y = R.tsse(xn, Pz, "att")[..., :T]                         # [B,C,T]
            loss = loss + (y * dX0[z, :, :T, m * C:(m + 1) * C].double().permute(0, 2, 1)).sum()
    loss.backward()
    want = fr.grad
    got = G1.double().cpu()
    tol = 3e-4
    for z in range(3):
        for k, n in shapes.items():
            sl = slice(z * sW + offs[k], z * sW + offs[k] + n)
            assert bool(torch.isfinite(got[sl]).all()), (z, k)
            record_err(f"{k}_{z}", rel(got[sl], want[sl]), tol)
    used = torch.zeros(3 * sW, dtype=torch.bool)
    for z in range(3):
        for k, n in shapes.items():
            used[z * sW + offs[k]: z * sW + offs[k] + n] = True
    assert bool(torch.isnan(got[~used]).all())                        # the gaps between parameters are not written
    assert torch.equal(G1[used.cuda()], G2[used.cuda()])
