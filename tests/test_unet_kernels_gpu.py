"""The support kernels of the inpainting U-Net (csrc/unet.hip: BatchNorm, pooling, upsampling, the thin convolutions, the
boundary maps) and the dropout bits (csrc/mc_pca.hip) through the C ABI against the fp64 references of tests/unet_ref.py,
at the shapes where they take another path: several workgroups with a ragged last one, every channel-group width, the
slice cap of the statistics reduction, tied pooling windows, one-pixel upsampling inputs, the narrow thin convolutions,
non-dense batch strides and the grid-stride second trip of every clamped grid.

Activations are rounded to the storage dtype before staging and the references are evaluated in fp64 on those values.
Every limit is derived (tests/unet_ref.py states how) or is the limit the project already uses for that kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
from unet_halo import Halo
from unet_ref import U24, q
from vad_ref import philox4x32_10

pytestmark = pytest.mark.gpu
PRECS = [("fp32", 1, torch.float32, 2e-5), ("bf16", 0, torch.bfloat16, 3e-2)]
ONE = float(np.nextafter(1.0, 2.0))      # record_err asserts measured < limit: ratio <= 1
SENT = 7.0                               # exactly representable in bf16


def sentinel(h):
    h.view().fill_(SENT)
    return h


def region(h, c0, c1, y0=0, y1=None, x0=0, x1=None):
    """bool mask over h.view(): channels [c0, c1) of the interior pixels [y0, y1) x [x0, x1)"""
    m = torch.zeros(h.B, h.H + 2, h.W + 2, h.ld, dtype=torch.bool)
    m[:, 1 + y0:1 + (h.H if y1 is None else y1), 1 + x0:1 + (h.W if x1 is None else x1), c0:c1] = True
    return m


def keeps_outside(h, written, value=SENT):
    v = h.view().float().cpu()
    return bool((v[~written] == value).all())


def nchw(v):
    """[B,H,W,C] -> [B,C,H,W]"""
    return v.permute(0, 3, 1, 2).contiguous()


# ---- 1. BatchNorm ------------------------------------------------------------------------------------------------------
# (B,H,W,C): 3 workgroups, last one 192 rows, 32 row lanes | 2 workgroups, last one 101 rows (no multiple of 4 * 4 lanes) |
# 2 workgroups, 8 lanes | fewer interior pixels than the 16 row lanes
BN_SHAPES = [(2, 30, 33, 64), (1, 23, 43, 512), (3, 9, 37, 256), (1, 2, 3, 128)]


@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("B,H,W,C", BN_SHAPES)
def test_batchnorm_forward_backward_against_fp64(pname, prec, dtype, tol, B, H, W, C, record_err):
    """nppc_bn_stats / _finalize / _act / _bwd / _bwd_dropout with fp64 atomics across workgroups and a ragged last one."""
    from nppc_audio import _hip as Hh
    bf = dtype == torch.bfloat16
    g = torch.Generator().manual_seed(1000 * C + 10 * H + B)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    x = R.bn_condition(torch.randn(B, C, H, W, generator=g) * 2 + 0.5, gamma, beta, dtype)
    n = float(B * H * W)
    s = Hh.stream()
    X = Halo(B, H, W, C, dtype).put(x)
    P = X.P
    Y = Halo(B, H, W, 2 * C, dtype)                   # written as the upper channel slice of a wider buffer
    st = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    ss = torch.empty(4 * C, dtype=torch.float32, device="cuda")
    rmd, rvd = rm.cuda(), rv.cuda()
    Hh.call("nppc_bn_stats", prec, X.t, C, P, C, st, s)
    Hh.call("nppc_bn_finalize", st, gamma.cuda(), beta.cuda(), rmd, rvd, ss, C, n, 1e-5, 0.1, 1, s)
    Hh.call("nppc_bn_act", prec, X.t, C, Y.t[C:], 2 * C, ss, C, B, H, W, R.SLOPE, s)
    torch.cuda.synchronize()
    # batch sums: fp64 accumulation of exact inputs
    s1, s2, sa = R.bn_stats_ref(x)
    std = st.cpu().numpy()
    record_err("st.sum", R.ratio(std[:C] - s1, 2.0 ** -40 * sa), ONE)
    record_err("st.sumsq", R.ratio(std[C:] - s2, 2.0 ** -40 * s2), ONE)
    # (scale, shift, mean, rstd) and the running buffers
    sc, sh, mean, rstd, rm_new, rv_new = R.bn_finalize_ref(s1, s2, n, gamma, beta, rm, rv)
    ssd = ss.cpu().double().numpy()
    for name, got, ref in (("scale", ssd[:C], sc), ("mean", ssd[2 * C:3 * C], mean), ("rstd", ssd[3 * C:], rstd)):
        record_err("ss." + name, R.ratio(got - ref, 4 * U24 * np.abs(ref)), ONE)
    record_err("ss.shift", R.ratio(ssd[C:2 * C] - sh, 4 * U24 * (np.abs(beta.double().numpy()) + np.abs(mean * sc))), ONE)
    record_err("running_mean", R.rel(rmd.cpu(), rm_new), 1e-5)
    record_err("running_var", R.rel(rvd.cpu(), rv_new), 1e-5)
    # the activation, element by element, from the device's own scale and shift
    assert R.bn_near_zero(x, ssd[:C], ssd[C:2 * C]) == 0          # no LeakyReLU decision within rounding of zero
    y_ref, y_bound = R.bn_act_ref(x, ssd[:C], ssd[C:2 * C], bf)
    record_err("bn_act", R.ratio(Y.get(C, C).double() - y_ref, y_bound), ONE)
    assert float(Y.get(C, 0).abs().max()) == 0.0 and Y.halo_is_zero()

    # backward: fp64 autograd for dx, the closed form from the device's ss for the reduction workspace
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.leaky_relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, float(np.float32(1e-5))), R.SLOPE_F32)
    d1, d2 = q(torch.randn(B, C, H, W, generator=g), dtype), q(torch.randn(B, C, H, W, generator=g), dtype)
    DA, DB = Halo(B, H, W, C, dtype).put(d1), Halo(B, H, W, 3 * C, dtype).put(d2, C)
    p, seed, stream_id = 0.2, 0x1234_5678_9ABC, 6
    cases = [("two", d2, None), ("one", None, None)]
    if C in (512, 256):
        cases.append(("drop", d2, R.keep_nchw(R.dropout_keep_ref(P, C, p, seed, stream_id), B, H, W)))
    for tag, dyb, keep in cases:
        DX = Halo(B, H, W, C, dtype)
        S = torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")      # (the entry point zeroes it)
        dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        args = (prec, DA.t, C, None if dyb is None else DB.t[C:], 0 if dyb is None else 3 * C, Y.t[C:], 2 * C, X.t, C, ss, S,
                DX.t, C, dgam, dbet, C, B, H, W, R.SLOPE)
        if keep is None:
            Hh.call("nppc_bn_bwd", *args, s)
        else:
            Hh.call("nppc_bn_bwd_dropout", *args, p, seed, stream_id, s)
        torch.cuda.synchronize()
        S1, S2, a1, a2, _, _ = R.bn_bwd_sums_ref(x, ssd, d1, dyb, keep, p)
        b1, b2 = R.bn_bwd_sum_bounds(P, C, a1, a2)
        Sd = S.cpu().numpy()
        record_err(tag + ".S.sum_g", R.ratio(Sd[:C] - S1, b1), ONE)
        record_err(tag + ".S.sum_g_xhat", R.ratio(Sd[C:] - S2, b2), ONE)
        assert torch.equal(dbet.cpu(), S[:C].float().cpu()) and torch.equal(dgam.cpu(), S[C:].float().cpu())
        out = yr if keep is None else yr * keep * R.drop_scale_f32(p)
        up = d1.double() if dyb is None else d1.double() + dyb.double()
        gx, gg, gb = torch.autograd.grad(out, (xr, gr, br), up, retain_graph=True)
        record_err(tag + ".dx", R.rel(DX.get(C), gx), tol * 3)
        record_err(tag + ".dgamma", R.rel(dgam.cpu(), gg), tol * 3)
        record_err(tag + ".dbeta", R.rel(dbet.cpu(), gb), tol * 3)
        assert DX.halo_is_zero()
        if keep is None:
            # p = 0: bit for bit the plain backward.  (The workgroups' fp64 atomics land in any order, so the last bit of S is
            # free; it takes a sum within 2^-53 of an fp32 rounding boundary to show in dgamma, dbeta or dx.)
            DX0 = Halo(B, H, W, C, dtype)
            S0 = torch.full_like(S, float("nan"))
            dg0, db0 = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            Hh.call("nppc_bn_bwd_dropout", *args[:10], S0, DX0.t, C, dg0, db0, *args[15:], 0.0, seed, stream_id, s)
            torch.cuda.synchronize()
            assert torch.equal(dg0, dgam) and torch.equal(db0, dbet) and torch.equal(DX0.t, DX.t)


# ---- 2. nppc_bn_stats_from_parts past its cap of 128 slices ------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("B,H,W,Cout", [(1, 126, 127, 64), (2, 126, 127, 64), (1, 126, 127, 100), (1, 260, 62, 64)])
def test_bn_stats_from_parts_past_the_slice_cap(pname, prec, dtype, tol, B, H, W, Cout, record_err):
    """129 tiles -> 2 per slice, 65 slices used (the last holds one tile), 63 empty; 258 tiles -> 3 per slice, 86 used.  In
    those shapes the last tile is all bottom halo (129 zero rows end the matrix), so a walk that lost it would go unseen:
    (1, 260, 62) has 131 tiles, 2 per slice, and the one tile of its last slice holds the last interior image row."""
    from nppc_audio import _hip as Hh
    Cin = 64
    Np, C = (Cout + 63) // 64 * 64, Cout // 8 * 8
    g = torch.Generator().manual_seed(B * 100 + Cout)
    x = q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    wf = torch.empty(Np * 9 * Cin, dtype=dtype, device="cuda")
    s = Hh.stream()
    Hh.call("nppc_conv_pack", prec, w.cuda(), wf, None, Cout, Cin, 3, Np, Cin, Cin, Np, s)
    X = Halo(B, H, W, Cin, dtype).put(x)
    Y = Halo(B, H, W, Np, dtype)
    ntiles = (X.P + 127) // 128
    assert ntiles > 128
    if W == 62:
        assert ntiles == 131 and (ntiles - 1) * 128 < (H * (W + 2) + W)      # (row of the last interior pixel: in the last tile)
    part = torch.full((ntiles * 2 * Np,), float("nan"), dtype=torch.float32, device="cuda")
    Hh.call("nppc_conv_fwd_stats", prec, X.t, Cin, wf, Y.t, Np, b.cuda(), B, H, W, Cin, Cout, Np, 3, part, s)
    st = torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")
    scr = torch.full((2 * C * 128,), float("nan"), dtype=torch.float64, device="cuda")
    Hh.call("nppc_bn_stats_from_parts", part, B, H, W, Np, C, st, scr, s)
    st2 = torch.full_like(st, float("nan"))
    Hh.call("nppc_bn_stats_from_parts", part, B, H, W, Np, C, st2, scr, s)
    torch.cuda.synchronize()
    assert not torch.isnan(st).any() and not torch.isnan(scr).any()
    assert torch.equal(st, st2)                                       # fixed summation order
    y = Y.view()[..., :C].double()                                    # the stored output (halo rows are zero)
    assert Y.halo_is_zero()
    s1, s2, sa = y.sum((0, 1, 2)).cpu().numpy(), (y * y).sum((0, 1, 2)).cpu().numpy(), y.abs().sum((0, 1, 2)).cpu().numpy()
    assert float(sa.min()) > 0
    # 128-row tile sums in fp32 (a chain of at most 128 additions), the rounded square, slack: 136 * 2^-24; then fp64
    std = st.cpu().numpy()
    record_err("st.sum", R.ratio(std[:C] - s1, 136 * U24 * sa), ONE)
    record_err("st.sumsq", R.ratio(std[C:] - s2, 136 * U24 * s2), ONE)


# ---- 3. pooling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("C,H,W,ties", [(C, H, W, True) for C in (64, 512) for H, W in ((7, 9), (2, 2), (6, 5))] + [(64, 7, 9, False)])
def test_maxpool_ties_route_to_the_first_maximum(pname, prec, dtype, tol, C, H, W, ties):
    """windows of exact zeros (the pool follows a Dropout) tie: the first maximum in scan order takes the gradient; the
    backward writes exactly the windows"""
    from nppc_audio import _hip as Hh
    B = 2
    g = torch.Generator().manual_seed(C + H * 31 + W)
    x = R.tie_alphabet((B, C, H, W), g) if ties else q(torch.randn(B, C, H, W, generator=g), dtype)
    assert (R.tie_fraction(x) > 1 / 3) == ties
    Ho, Wo = H // 2, W // 2
    s = Hh.stream()
    X = Halo(B, H, W, C, dtype).put(x)
    Y = Halo(B, Ho, Wo, C, dtype)
    idx = torch.full((Y.P * C,), 255, dtype=torch.uint8, device="cuda")
    Hh.call("nppc_maxpool2", prec, X.t, C, Y.t, C, idx, C, B, H, W, s)
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    y_ref, idx_ref = R.maxpool_first_max_ref(x)
    assert torch.equal(Y.get(C), yr.detach()) and torch.equal(yr.detach(), y_ref) and Y.halo_is_zero()
    iv = nchw(idx.view(B, Ho + 2, Wo + 2, C)[:, 1:-1, 1:-1].cpu().long())
    assert int(iv.min()) >= 0 and int(iv.max()) <= 3
    assert torch.equal(iv, idx_ref)
    dy = q(torch.randn(B, C, Ho, Wo, generator=g), dtype)
    yr.backward(dy)
    DY = Halo(B, Ho, Wo, C, dtype).put(dy)
    DX = sentinel(Halo(B, H, W, C, dtype))
    Hh.call("nppc_maxpool2_bwd", prec, DY.t, C, idx, DX.t, C, C, B, H, W, s)
    torch.cuda.synchronize()
    got = DX.get(C)
    assert torch.equal(got[:, :, :2 * Ho, :2 * Wo], xr.grad[:, :, :2 * Ho, :2 * Wo])
    assert torch.equal(got, R.maxpool_bwd_ref(dy, idx_ref, H, W, fill=SENT))      # the odd last row / column: untouched
    assert keeps_outside(DX, region(DX, 0, C, 0, 2 * Ho, 0, 2 * Wo))


# ---- 4. upsampling ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("Hi,Wi,Ht,Wt", [(1, 1, 2, 2), (1, 1, 3, 3), (1, 4, 3, 9), (3, 5, 7, 10), (4, 6, 8, 12)])
def test_bilinear_upsample_edges_and_adjoint(pname, prec, dtype, tol, C, Hi, Wi, Ht, Wt, record_err):
    """one-pixel inputs (nin - 1 = 0 in the source-index scale), padded and unpadded targets, the adjoint identity"""
    from nppc_audio import _hip as Hh
    B = 2
    fp32 = dtype == torch.float32
    g = torch.Generator().manual_seed(C + 100 * Hi + 10 * Wi + Ht)
    x = q(torch.randn(B, C, Hi, Wi, generator=g), dtype)
    s = Hh.stream()
    X = Halo(B, Hi, Wi, C, dtype).put(x)
    U = sentinel(Halo(B, Ht, Wt, 2 * C, dtype))
    Hh.call("nppc_upsample2", prec, X.t, C, U.t[C:], 2 * C, C, B, Hi, Wi, Ht, Wt, s)
    torch.cuda.synchronize()
    pr = x.clone().requires_grad_(True)
    up, (py, px) = R.upsample_pad_ref(pr, Ht, Wt)            # torch fp32: the definition (fp32 index arithmetic)
    win = (slice(None), slice(None), slice(py, py + 2 * Hi), slice(px, px + 2 * Wi))
    ud = U.get(C, C)
    record_err("forward", R.rel(ud[win], up.detach()[win]), 1e-6 if fp32 else 1e-2)
    assert keeps_outside(U, region(U, C, 2 * C, py, py + 2 * Hi, px, px + 2 * Wi))      # padding ring, other slice, halo
    du = q(torch.randn(B, C, Ht, Wt, generator=g), dtype)
    up.backward(du)
    DU = Halo(B, Ht, Wt, 2 * C, dtype).put(du, C)
    DP = sentinel(Halo(B, Hi, Wi, C, dtype))
    Hh.call("nppc_upsample2_bwd", prec, DU.t[C:], 2 * C, DP.t, C, C, B, Hi, Wi, Ht, Wt, s)
    torch.cuda.synchronize()
    dp = DP.get(C)
    record_err("backward", R.rel(dp, pr.grad), 1e-5 if fp32 else 1e-2)
    assert keeps_outside(DP, region(DP, 0, C))
    if fp32:
        # <up(x), g> = <x, up^T(g)> on the device's own outputs, both sides summed in fp64.  Each side is a sum of products of
        # x, g and two interpolation weights that the two kernels round differently (a handful of fp32 roundings per term):
        # 2^-18 = 64 * 2^-24 of the sum of the terms' magnitudes
        lhs = float((ud[win].double() * du[win].double()).sum())
        rhs = float((x.double() * dp.double()).sum())
        mag = float((R.upsample_pad_ref(x.abs(), Ht, Wt)[0].double() * du.abs().double()).sum())
        record_err("adjoint", abs(lhs - rhs) / (2.0 ** -18 * mag), ONE)


# ---- 5. thin convolutions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("Cout", [8, 32])
@pytest.mark.parametrize("Cin", [1, 2])
@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 9, 13)])
def test_thin_3x3_convolution_narrow_widths(pname, prec, dtype, tol, Cout, Cin, B, H, W, record_err):
    """Cout = 8: one channel chunk, 256 pixel lanes per workgroup, 85 weight-gradient groups and an idle thread 255; P = 63 is
    no multiple of the four rows a thread owns"""
    from nppc_audio import _hip as Hh
    ld = 32
    g = torch.Generator().manual_seed(11 * B + Cin + Cout)
    x = q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 3.0
    b = torch.randn(Cout, generator=g) * 0.1
    s = Hh.stream()
    X = Halo(B, H, W, ld, dtype).put(x)
    Y = Halo(B, H, W, Cout, dtype)
    Hh.call("nppc_conv3x3_thin_fwd", prec, X.t, ld, w.cuda(), b.cuda(), None, None, R.SLOPE, Y.t, Cout, B, H, W, Cin, Cout, s)
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    record_err("forward", R.rel(Y.get(Cout), ref), tol)
    assert Y.halo_is_zero()
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    Y2 = Halo(B, H, W, Cout, dtype)
    Hh.call("nppc_conv3x3_thin_fwd", prec, X.t, ld, w.cuda(), b.cuda(), sc.cuda(), sh.cuda(), R.SLOPE, Y2.t, Cout, B, H, W, Cin,
            Cout, s)
    ref2 = F.leaky_relu(ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], R.SLOPE_F32)
    record_err("folded", R.rel(Y2.get(Cout), ref2), tol)
    assert Y2.halo_is_zero()
    dy = q(torch.randn(B, Cout, H, W, generator=g), dtype)
    DY = Halo(B, H, W, Cout, dtype).put(dy)
    part = torch.empty(Hh.conv_thin_part_elems(), dtype=torch.float32, device="cuda")
    dW = torch.full((Cout, Cin, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
    Hh.call("nppc_conv3x3_thin_wgrad", prec, DY.t, Cout, X.t, ld, part, dW, B, H, W, Cin, Cout, s)
    torch.cuda.synchronize()
    wr = w.double().requires_grad_(True)
    F.conv2d(x.double(), wr, None, padding=1).backward(dy.double())
    record_err("wgrad", R.rel(dW.cpu(), wr.grad), tol if pname == "fp32" else 2e-3)


def dev_rel(a, b):
    """rel() on the device, for tensors too large to compare on the host"""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def test_thin_3x3_grid_stride_second_trip(record_err):
    """P = 527076 haloed rows > the 4096 * 128 rows one trip of the clamped grid covers (bf16, Cin = 1, Cout = 64)"""
    from nppc_audio import _hip as Hh
    _, prec, dtype, tol = PRECS[1]
    B, H, W, Cin, Cout, ld = 1, 724, 724, 1, 64, 8
    assert B * (H + 2) * (W + 2) == 527076 > 4096 * 128
    g = torch.Generator().manual_seed(724)
    x = q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 3.0
    b = torch.randn(Cout, generator=g) * 0.1
    s = Hh.stream()
    X = Halo(B, H, W, ld, dtype).put(x)
    Y = Halo(B, H, W, Cout, dtype)
    Hh.call("nppc_conv3x3_thin_fwd", prec, X.t, ld, w.cuda(), b.cuda(), None, None, R.SLOPE, Y.t, Cout, B, H, W, Cin, Cout, s)
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).cuda()
    record_err("forward", dev_rel(Y.view()[:, 1:-1, 1:-1], ref.permute(0, 2, 3, 1)), tol)
    # the rows of the second trip alone (a skipped trip leaves zeros there)
    y0 = 4096 * 128 // (W + 2)                 # first interior image row wholly behind the first trip
    record_err("forward.second_trip", dev_rel(Y.view()[:, 1 + y0:-1, 1:-1], ref.permute(0, 2, 3, 1)[:, y0:]), tol)
    assert Y.halo_is_zero()


def test_thin_1x1_grid_stride_second_trip(record_err):
    """P = 132496 haloed rows > the 4096 * 32 rows one trip covers: forward and input gradient (bf16, K = 5)"""
    from nppc_audio import _hip as Hh
    _, prec, dtype, tol = PRECS[1]
    B, H, W, Cin, K, ld = 1, 362, 362, 64, 5, 8
    assert B * (H + 2) * (W + 2) == 132496 > 4096 * 32
    g = torch.Generator().manual_seed(362)
    x = q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = torch.randn(K, Cin, 1, 1, generator=g) / 8.0
    b = torch.randn(K, generator=g) * 0.1
    s = Hh.stream()
    X = Halo(B, H, W, Cin, dtype).put(x)
    Y = Halo(B, H, W, ld, dtype)
    Hh.call("nppc_conv1x1_thin_fwd", prec, X.t, Cin, w.cuda(), b.cuda(), Y.t, ld, B, H, W, Cin, K, s)
    torch.cuda.synchronize()
    y0 = 4096 * 32 // (W + 2)                  # first interior image row wholly behind the first trip
    ref = F.conv2d(x.double(), w.double(), b.double())
    got = Y.get(ld)
    record_err("forward", R.rel(got[:, :K], ref), tol)
    record_err("forward.second_trip", R.rel(got[:, :K, y0:], ref[:, :, y0:]), tol)
    assert Y.halo_is_zero() and float(got[:, K:].abs().max()) == 0.0
    dy = q(torch.randn(B, K, H, W, generator=g), dtype)
    DY = Halo(B, H, W, ld, dtype).put(dy)
    DX = Halo(B, H, W, Cin, dtype)
    Hh.call("nppc_conv1x1_thin_bwd_data", prec, DY.t, ld, w.cuda(), DX.t, Cin, B, H, W, Cin, K, s)
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    F.conv2d(xr, w.double(), None).backward(dy.double())
    gotx = DX.get(Cin)
    record_err("bwd_data", R.rel(gotx, xr.grad), tol)
    record_err("bwd_data.second_trip", R.rel(gotx[:, :, y0:], xr.grad[:, :, y0:]), tol)
    assert DX.halo_is_zero()


# ---- 6. boundary maps ------------------------------------------------------------------------------------------------------
# (B,F,T): the toy size, and one past the 1024 x 256 (logmag, standardize) and 4096 x 256 (unet_out) grid caps by no multiple of 256
@pytest.mark.parametrize("B,Fq,T", [(2, 5, 7), (3, 129, 700)])
@pytest.mark.parametrize("with_b", [True, False])
def test_logmag_and_standardize_against_fp64(B, Fq, T, with_b, record_err):
    from nppc_audio import _hip as Hh
    FT = Fq * T
    bs = FT + 5                                           # batch stride of the outputs: a gap of 5 after every item
    assert (B, Fq, T) == (2, 5, 7) or (B * FT > 1024 * 256 and (B * FT) % 256)
    g = torch.Generator().manual_seed(B * 1000 + T)
    spec = torch.randn(B, 2, Fq, T, generator=g)
    spec[0, :, 0, 0] = 0.0                                # |z| = 0: log(1e-6)
    spec[1, :, 1, 2] = torch.tensor([1e-40, -3e-42])      # denormals
    spec[1, :, 2, 3] = torch.tensor([0.0, 2e-39])
    spec[0, :, 3, 1] = torch.tensor([-0.0, 5.0])
    s = Hh.stream()
    out = torch.full((B, bs), SENT, dtype=torch.float32, device="cuda")
    st = torch.zeros(2, dtype=torch.float64, device="cuda")
    Hh.call("nppc_logmag", spec.cuda(), out, bs, B, FT, st, s)
    torch.cuda.synchronize()
    v = out[:, :FT].cpu()
    ref, bound = R.logmag_ref(spec)
    record_err("logmag", R.ratio(v.double() - ref.reshape(B, FT), bound.reshape(B, FT)), ONE)
    assert bool((out[:, FT:] == SENT).all())
    std = st.cpu().numpy()
    vd = v.double()
    record_err("st.sum", R.ratio(std[0] - float(vd.sum()), 2.0 ** -40 * float(vd.abs().sum())), ONE)
    record_err("st.sumsq", R.ratio(std[1] - float((vd * vd).sum()), 2.0 ** -40 * float((vd * vd).sum())), ONE)
    # standardize in place, from the sums the device left
    a2 = torch.full((B, bs), SENT, dtype=torch.float32, device="cuda")
    w = torch.randn(B, FT, generator=g) * 3 - 4
    a2[:, :FT] = w.cuda()
    ms = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
    Hh.call("nppc_standardize", out, a2 if with_b else None, bs, B, FT, st, ms, s)
    torch.cuda.synchronize()
    za, ba, mean, sd = R.standardize_ref(v, float(std[0]), float(std[1]), float(B * FT))
    msd = ms.cpu().double().numpy()
    record_err("mean", abs(msd[0] - mean) / (2.0 ** -23 * abs(mean)), ONE)
    record_err("std", abs(msd[1] - sd) / (2.0 ** -23 * sd), ONE)
    record_err("standardize.a", R.ratio(out[:, :FT].cpu().double() - za, ba), ONE)
    assert bool((out[:, FT:] == SENT).all())
    if with_b:
        zb, bb, _, _ = R.standardize_ref(w, float(std[0]), float(std[1]), float(B * FT))
        record_err("standardize.b", R.ratio(a2[:, :FT].cpu().double() - zb, bb), ONE)
    else:
        assert torch.equal(a2[:, :FT].cpu(), w)
    assert bool((a2[:, FT:] == SENT).all())


@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
def test_stage_map_writes_one_channel(pname, prec, dtype, tol):
    from nppc_audio import _hip as Hh
    B, H, W, ld, c = 2, 5, 7, 32, 3
    sbs = H * W + 4
    g = torch.Generator().manual_seed(9)
    src = torch.randn(B, sbs, generator=g)
    D = sentinel(Halo(B, H, W, ld, dtype))
    Hh.call("nppc_unet_stage_map", prec, src.cuda(), sbs, D.t, ld, c, B, H, W, Hh.stream())
    torch.cuda.synchronize()
    assert torch.equal(D.get(1, c), q(src[:, :H * W].reshape(B, 1, H, W), dtype))       # exact: one rounding to storage
    assert keeps_outside(D, region(D, c, c + 1))


def _mask(B, W, g):
    m = (torch.rand(B, W, generator=g) < 0.5).float()
    m[:, 0], m[:, 1] = 0.0, 1.0
    m[:, W // 2] = 0.3                                    # one fractional column
    return m


@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("B,H,W,K,mode", [(2, 5, 7, 1, 0), (2, 5, 7, 5, 0), (2, 5, 7, 8, 0), (2, 5, 7, 1, 1), (2, 129, 830, 5, 0)])
def test_unet_out_blending_against_fp64(pname, prec, dtype, tol, B, H, W, K, mode, record_err):
    from nppc_audio import _hip as Hh
    ld = 8 if H > 100 else 64
    assert H < 100 or (B * K * H * W > 4096 * 256 and (B * K * H * W) % 256)
    ps, xbs = H * W + 3, H * W + 5
    g = torch.Generator().manual_seed(B * K + W + mode)
    raw = q(torch.randn(B, K, H, W, generator=g), dtype)
    mask = _mask(B, W, g)
    xin = torch.randn(B, xbs, generator=g)
    Rw = Halo(B, H, W, ld, dtype).put(raw)
    out = torch.full((B * K, ps), SENT, dtype=torch.float32, device="cuda")
    Hh.call("nppc_unet_out", prec, Rw.t, ld, mask.cuda(), xin.cuda() if mode else None, xbs, out, ps, K, B, H, W, mode, Hh.stream())
    torch.cuda.synchronize()
    ref, bound = R.unet_out_ref(raw, mask, xin[:, :H * W].reshape(B, H, W) if mode else None)
    got = out[:, :H * W].cpu().double().reshape(B, K, H, W)
    record_err("out", R.ratio(got - ref, bound), ONE)
    assert bool((out[:, H * W:] == SENT).all())


@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("K", [1, 5, 8])
def test_unet_out_backward_writes_only_its_columns(pname, prec, dtype, tol, K, record_err):
    from nppc_audio import _hip as Hh
    B, H, W, ld = 2, 5, 7, 64
    ps = H * W + 3
    g = torch.Generator().manual_seed(K)
    dout = torch.randn(B * K, ps, generator=g)
    mask = _mask(B, W, g)
    D = sentinel(Halo(B, H, W, ld, dtype))
    Hh.call("nppc_unet_out_bwd", prec, dout.cuda(), ps, mask.cuda(), D.t, ld, K, B, H, W, Hh.stream())
    torch.cuda.synchronize()
    ref, bound = R.unet_out_bwd_ref(dout[:, :H * W].reshape(B, K, H, W), mask, dtype == torch.bfloat16)
    record_err("draw", R.ratio(D.get(K).double() - ref, bound), ONE)
    assert keeps_outside(D, region(D, 0, K))              # columns >= K and the halo are the caller's


# ---- 7. dropout bits --------------------------------------------------------------------------------------------------------
_KEEP = {}


def _keep_ref(rows, C, p, seed, stream_id):
    """the keep bits from the scalar generator of tests/vad_ref.py, once per case"""
    key = (rows, C, p, seed, stream_id)
    if key not in _KEEP:
        _KEEP[key] = R.dropout_keep_ref(rows, C, p, seed, stream_id, philox=philox4x32_10)
    return _KEEP[key]


@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("rows,C", [(70, 128), (33, 512)])
def test_dropout_bits_are_philox_words(pname, prec, dtype, tol, p, rows, C):
    """keep[r][4 c4 + i] = (word i of Philox4x32-10(counter (r lo, r hi, c4, stream), key (seed lo, seed hi)) >= p 2^32)"""
    from nppc_audio import _hip as Hh
    seed, stream_id = 0x0000_1234_9ABC_DEF0, 5           # non-zero high word
    assert seed >> 32
    ld = 2 * C
    g = torch.Generator().manual_seed(rows + C)
    x = q(torch.randn(rows, ld, generator=g), dtype)
    X = x.to(dtype).cuda()
    keep = torch.full((rows * C,), 9, dtype=torch.uint8, device="cuda")
    Hh.call("nppc_dropout", prec, X, ld, rows, C, p, seed, stream_id, keep, Hh.stream())
    torch.cuda.synchronize()
    want = _keep_ref(rows, C, p, seed, stream_id)
    kd = keep.cpu().numpy().reshape(rows, C)
    assert np.array_equal(kd, want)
    assert np.array_equal(want, R.dropout_keep_ref(rows, C, p, seed, stream_id))         # (the vectorised reference agrees)
    got = X.float().cpu()
    scaled = (x[:, :C] * torch.tensor(R.drop_scale_f32(p))).to(dtype).float()            # x / (1 - p) in fp32, rounded to storage
    wk = torch.from_numpy(want.astype(bool))
    assert torch.equal(got[:, :C][wk], scaled[wk])
    assert bool((got[:, :C][~wk] == 0).all())
    assert torch.equal(got[:, C:], x[:, C:])                                              # channels C .. 2C-1 untouched


def test_dropout_argument_guards():
    from nppc_audio import _hip as Hh
    X = torch.zeros(8 * 16, device="cuda")
    for ld, C, p in ((16, 6, 0.2), (16, 8, 1.0), (4, 8, 0.2)):        # C % 4, p = 1, ld < C
        with pytest.raises(RuntimeError, match="bad argument"):
            Hh.call("nppc_dropout", Hh.PREC_F32, X, ld, 8, C, p, 1, 0, None, Hh.stream())
    assert float(X.abs().max()) == 0.0
