"""GPU: the MFMA convolutions of csrc/unet.hip and the nine-tap weight gradient of csrc/tcn.hip, element by element against
the fp64 references and the derived bounds of tests/unet_ref.py (conv_bound, conv_wgrad_bound; tests/test_unet_conv_ref_cpu.py
shows that honest fp32 arithmetic stays inside them and wrong arithmetic does not).

Forward / input gradient (nppc_conv_fwd, nppc_conv_fwd_stats): conv_tiled_kernel<bf16 | float, 64 | 128>, conv_kernel<bf16>
and the LDS-DMA ring conv_dma_kernel<64 | 128, 3>, with 1, 2, 3, 9 and 36 K stages around the ring depth of three, ragged and
mostly-halo pixel tiles, Cout below the padded width, the skip-into-concat write (ldc = 2 Np), a channel slice as the input
(lda > Cin), the folded BatchNorm + LeakyReLU epilogue with scales of both signs, and the backward pack.
Weight gradient (nppc_conv_wgrad + nppc_conv_wgrad_reduce): every path of launch_tn with nine taps -- tiled 128 / 64, M == 64
computed as 128, the transposed orientation (shift_a), the rings gemm_tn_dma_kernel<128,64,3> and <192,32,5> at the ksplit the
engine plans (slices wholly behind P, and one image large enough for more stages than ring slots) -- the plain split-K of a
1x1 convolution and the fp32 wgrad_simple_kernel; nppc_gemm_tn_splitk_taps itself slab by slab with rows wider than its operands.

Every buffer a kernel must not write starts as a bf16-exact sentinel, slabs and statistics start as NaN."""
import functools

import numpy as np
import pytest
import torch

import unet_ref as R
from unet_halo import Halo

pytestmark = pytest.mark.gpu
SENT = -1536.0                       # exact in bf16
NAN = float("nan")
BF16, F32 = "bf16", "fp32"


def rup(n, m):
    return (n + m - 1) // m * m


def prec_of(pname):
    from nppc_audio import _hip as Hh
    return (Hh.PREC_BF16, torch.bfloat16) if pname == BF16 else (Hh.PREC_F32, torch.float32)


@pytest.fixture
def dispatch(monkeypatch):
    """select the convolution kernel the way tests/test_inpaint_gpu.py does: "ring" sends every tiled bf16 shape to
    conv_dma_kernel, anything else leaves the default dispatch (the ring only from 256 workgroups on)"""
    def select(kernel):
        if kernel == "ring":
            monkeypatch.setenv("NPPC_CONV_DMA", "1")
            monkeypatch.setenv("NPPC_CONV_DMA_MIN_TILES", "1")
        else:
            monkeypatch.delenv("NPPC_CONV_DMA", raising=False)
            monkeypatch.delenv("NPPC_CONV_DMA_MIN_TILES", raising=False)
    return select


@functools.lru_cache(maxsize=None)
def conv_case(pname, B, H, W, Cin, Cout, ks):
    """operands as the kernels read them and their fp64 references: computed once, shared by the kernels that run the
    shape, never modified"""
    dtype = torch.bfloat16 if pname == BF16 else torch.float32
    g = torch.Generator().manual_seed(1000 * B + 10 * Cin + Cout + ks + H)
    x = R.q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = R.q(torch.randn(Cout, Cin, ks, ks, generator=g) / np.sqrt(Cin * ks * ks), dtype)
    b = torch.randn(Cout, generator=g) * 0.1
    dy = R.q(torch.randn(B, Cout, H, W, generator=g), dtype)
    fold = (torch.where(torch.arange(Cout) % 2 == 0, 1.0, -1.0) * (torch.rand(Cout, generator=g) + 0.5),
            torch.randn(Cout, generator=g) * 0.1)
    junk = R.q(torch.randn(B, 64, H, W, generator=g) * 50, dtype)
    return dict(x=x, w=w, b=b, dy=dy, fold=fold, junk=junk, cr=R.conv_ref(x, w, b, ks), crf=R.conv_ref(x, w, b, ks, fold),
                dx=R.conv_dx_ref(dy, w, ks))


def out_buf(B, H, W, ld, dtype):
    """an output matrix: zero halo and guard rows, the sentinel in every column of the interior rows"""
    Y = Halo(B, H, W, ld, dtype, guard_after=512)
    Y.view()[:, 1:-1, 1:-1, :] = SENT
    return Y


def untouched_outside(Y, C, coff):
    """the kernel wrote nothing but columns [coff, coff + C) of the interior rows: halo and guard rows are still zero, the
    other columns still hold the sentinel"""
    c = Y.store.clone()
    c[Y.gb * Y.ld: (Y.gb + Y.P) * Y.ld].view(Y.B, Y.H + 2, Y.W + 2, Y.ld)[:, 1:-1, 1:-1, coff:coff + C] = SENT
    return torch.equal(c, out_buf(Y.B, Y.H, Y.W, Y.ld, Y.store.dtype).store) and Y.halo_is_zero()


# kernel, precision, B, H, W, Cin, Cout, ks.  P = 330 (2, 9, 13): a partly filled last 128- and 256-row tile and grid padding
# tiles with m0 >= P; (1, 6, 37): one 256-row tile, mostly halo.  K stages: ks^2 * Cin / 64 (bf16) or / 32 (fp32).
BF16_TILED = [(2, 9, 13, 64, 64, 1),        # 1 stage, 64-column tile
              (1, 6, 37, 64, 128, 1),       # 1 stage, 128-column tile
              (2, 9, 13, 128, 128, 1),      # 2 stages
              (1, 6, 37, 192, 64, 1),       # 3 stages
              (2, 9, 13, 64, 5, 3),         # 9 stages, 5 of 64 columns
              (2, 9, 13, 64, 100, 3),       # 9 stages, 100 of 128 columns
              (1, 6, 37, 256, 128, 3)]      # 36 stages
F32_TILED = [(2, 9, 13, 32, 64, 1), (2, 9, 13, 64, 128, 1), (1, 6, 37, 96, 5, 1), (2, 9, 13, 32, 100, 3), (1, 6, 37, 128, 64, 3)]
BF16_REG = [(2, 9, 13, 32, 64, 1), (2, 9, 13, 96, 100, 3), (1, 6, 37, 32, 5, 3)]       # Cin % 64 == 32: conv_kernel<bf16>
FWD_CASES = ([("tiled", BF16) + s for s in BF16_TILED] + [("ring", BF16) + s for s in BF16_TILED]
             + [("tiled", F32) + s for s in F32_TILED] + [("reg", BF16) + s for s in BF16_REG])


def case_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("kernel,pname,B,H,W,Cin,Cout,ks", FWD_CASES, ids=[case_id(c) for c in FWD_CASES])
def test_convolution_forward_and_input_gradient_match_fp64(kernel, pname, B, H, W, Cin, Cout, ks, dispatch, record_err):
    from nppc_audio import _hip as Hh
    prec, dtype = prec_of(pname)
    bf16 = pname == BF16
    c = conv_case(pname, B, H, W, Cin, Cout, ks)
    cr, crf, dxr, fold = c["cr"], c["crf"], c["dx"], c["fold"]
    Np, Mb, nt = rup(Cout, 64), rup(Cin, 64), ks * ks
    K = nt * Cin
    tiled_shape = Cin % (64 if bf16 else 32) == 0
    assert tiled_shape == (kernel != "reg")
    P = B * (H + 2) * (W + 2)
    assert (P + 255) // 256 * (Np // 64) < 256              # below the ring's default threshold: "tiled" is the tiled kernel
    dispatch(kernel)
    s = Hh.stream()
    wf = torch.empty(Np * nt * Cin, dtype=dtype, device="cuda")
    wb = torch.empty(Mb * nt * Np, dtype=dtype, device="cuda")
    Hh.call("nppc_conv_pack", prec, c["w"].cuda(), wf, wb, Cout, Cin, ks, Np, Cin, Mb, Np, s)
    bias, sc, sh = c["b"].cuda(), fold[0].cuda(), fold[1].cuda()
    X = Halo(B, H, W, Cin, dtype).put(c["x"])

    def fwd(Xt, lda, Yt, ldc, folded=False):
        Hh.call("nppc_conv_fwd", prec, Xt, lda, wf, Yt, ldc, bias, sc if folded else None, sh if folded else None, 0.2,
                B, H, W, Cin, Cout, Np, ks, s)
        torch.cuda.synchronize()

    def check(tag, Y, C, coff, ref, bound):
        assert untouched_outside(Y, C, coff), tag
        record_err(tag, R.ratio(Y.get(C, coff).double() - ref.ref, bound), 1.0)

    # dense rows: ldc == Np, columns [Cout, Np) keep the sentinel
    Y = out_buf(B, H, W, Np, dtype)
    fwd(X.t, Cin, Y.t, Np)
    check("fwd", Y, Cout, 0, cr, R.conv_bound(cr, K, bf16))
    # the engine's skip-into-concat write: channels [0, Cout) of rows twice as wide, the other half belongs to nppc_upsample2
    Yc = out_buf(B, H, W, 2 * Np, dtype)
    fwd(X.t, Cin, Yc.t, 2 * Np)
    check("fwd_concat", Yc, Cout, 0, cr, R.conv_bound(cr, K, bf16))
    assert torch.equal(Yc.get(Cout), Y.get(Cout))
    # folded BatchNorm + LeakyReLU, scales of both signs
    Yf = out_buf(B, H, W, Np, dtype)
    fwd(X.t, Cin, Yf.t, Np, folded=True)
    check("fwd_fold", Yf, Cout, 0, crf, R.conv_bound(crf, K, bf16, fold))
    # the input as a channel slice: offset 64 of rows 64 wider (lda > Cin); the other channels hold large values
    Xs = Halo(B, H, W, Cin + 64, dtype).put(c["junk"], 0).put(c["x"], 64)
    Ys = out_buf(B, H, W, Np, dtype)
    fwd(Xs.t[64:], Cin + 64, Ys.t, Np)
    check("fwd_lda", Ys, Cout, 0, cr, R.conv_bound(cr, K, bf16))
    assert torch.equal(Ys.get(Cout), Y.get(Cout))          # the same products in the same order
    # the same convolution leaving the per-tile statistics (tiled and ring kernels only)
    if tiled_shape:
        Yt = out_buf(B, H, W, Np, dtype)
        part = torch.full(((P + 127) // 128 * 2 * Np,), NAN, dtype=torch.float32, device="cuda")
        Hh.call("nppc_conv_fwd_stats", prec, X.t, Cin, wf, Yt.t, Np, bias, B, H, W, Cin, Cout, Np, ks, part, s)
        torch.cuda.synchronize()
        assert torch.equal(Yt.store, Y.store) and not bool(torch.isnan(part).any())
    # input gradient through the backward pack, as UNetEngine._conv_bwd_data calls it: Cin and Np swap roles, written into the
    # upper half of a concat-wide row
    DY = Halo(B, H, W, Np, dtype).put(c["dy"])
    DX = out_buf(B, H, W, 2 * Mb, dtype)
    Hh.call("nppc_conv_fwd", prec, DY.t, Np, wb, DX.t[Mb:], 2 * Mb, None, None, None, 0.2, B, H, W, Np, Cin, Mb, ks, s)
    torch.cuda.synchronize()
    check("dx", DX, Cin, Mb, dxr, R.conv_bound(dxr, nt * Np, bf16))


def test_default_dispatch_takes_the_ring_from_256_workgroups(dispatch, record_err):
    """no environment switch: Np % 128 == 0 and ceil(P / 256) * Np / 128 = 256 workgroups -> conv_dma_kernel<128, 3> (the
    XCD-aware tile order over a grid of more than one round)"""
    from nppc_audio import _hip as Hh
    B, H, W, Cin, Cout, ks = 4, 126, 126, 64, 128, 3
    prec, dtype = prec_of(BF16)
    P = B * (H + 2) * (W + 2)
    assert Cout % 128 == 0 and (P + 255) // 256 * (Cout // 128) >= 256
    dispatch("default")
    g = torch.Generator().manual_seed(77)
    x = R.q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = R.q(torch.randn(Cout, Cin, ks, ks, generator=g) / np.sqrt(Cin * ks * ks), dtype)
    b = torch.randn(Cout, generator=g) * 0.1
    cr = R.conv_ref(x, w, b, ks)
    s = Hh.stream()
    wf = torch.empty(Cout * 9 * Cin, dtype=dtype, device="cuda")
    Hh.call("nppc_conv_pack", prec, w.cuda(), wf, None, Cout, Cin, ks, Cout, Cin, Cin, Cout, s)
    X = Halo(B, H, W, Cin, dtype).put(x)
    Y = out_buf(B, H, W, 2 * Cout, dtype)
    Hh.call("nppc_conv_fwd", prec, X.t, Cin, wf, Y.t, 2 * Cout, b.cuda(), None, None, 0.2, B, H, W, Cin, Cout, Cout, ks, s)
    torch.cuda.synchronize()
    assert untouched_outside(Y, Cout, 0)
    record_err("fwd_concat", R.ratio(Y.get(Cout).double() - cr.ref, R.conv_bound(cr, 9 * Cin, True)), 1.0)


# ------------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=None)
def wgrad_case(pname, B, H, W, Cout, Cin, ks):
    dtype = torch.bfloat16 if pname == BF16 else torch.float32
    g = torch.Generator().manual_seed(100 * B + Cin + 3 * Cout + ks)
    x = R.q(torch.randn(B, Cin, H, W, generator=g), dtype)
    dy = R.q(torch.randn(B, Cout, H, W, generator=g), dtype)
    return x, dy, R.conv_wgrad_ref(dy, x, ks)


# precision, B, H, W, Cout, Cin, ks, ksplit  (P = 330 for 9 x 13, P = 1984 for 30 x 29)
WGRAD_CASES = [
    (BF16, 2, 9, 13, 128, 128, 3, 1), (BF16, 2, 9, 13, 128, 128, 3, 3),      # gemm_tn_tiled_kernel<128>, nine taps
    (BF16, 2, 9, 13, 64, 64, 3, 3),                                          # M == 64 computed as 128, upper half discarded
    (BF16, 2, 9, 13, 64, 128, 3, 3), (BF16, 2, 9, 13, 64, 128, 3, 8),        # transposed (shift_a), tiled 64: up4's first convolution
    (BF16, 2, 30, 29, 256, 128, 3, 32),                                      # ring <128,64,3>: R = 2048, the last slice wholly behind P
    (BF16, 2, 30, 29, 256, 128, 3, 64),                                      # R = 4096 (the engine's cap): half the slices behind P
    (BF16, 2, 30, 29, 256, 192, 3, 32),                                      # ring <192,32,5>
    (BF16, 2, 30, 29, 192, 256, 3, 32),                                      # ring with shift_a
    (BF16, 2, 62, 61, 256, 128, 3, 32),                                      # ring <128,64,3>, P = 8064: four stages per slice
    (BF16, 2, 9, 13, 12, 64, 1, 3),                                          # 1x1: plain split-K (the tiled head, out_ch > 8), M = 64
    (F32, 2, 9, 13, 64, 64, 3, 3), (F32, 2, 9, 13, 64, 64, 3, 24),           # wgrad_simple_kernel; ksplit 24: slices starting
    (F32, 2, 9, 13, 128, 64, 3, 3), (F32, 2, 9, 13, 128, 64, 3, 24)]         # behind P write zero slabs


def test_the_weight_gradient_cases_reach_the_paths_they_name():
    """the dispatch conditions of launch_tn / nppc_conv_wgrad, restated for the bf16 nine-tap cases above"""
    from nppc_audio import _hip as Hh
    paths = []
    for pname, B, H, W, Cout, Cin, ks, ksplit in WGRAD_CASES:
        if pname != BF16 or ks != 3:
            continue
        M, N = rup(Cout, 64), Cin
        tr = Hh.lib().nppc_conv_wgrad_transposed(M, N)
        gm, gn = (N, M) if tr else (rup(M, 128), N)
        bn = 192 if gn % 192 == 0 else (128 if gn % 128 == 0 else 0)
        ring = gm % 256 == 0 and bn and (gm // 256) * (gn // bn) * ksplit * 9 >= 256
        paths.append((("ring%d" % bn) if ring else ("tiled%d" % (128 if gn % 128 == 0 else 64))) + ("T" if tr else ""))
        P = B * (H + 2) * (W + 2)
        if ring and P == 1984:
            assert rup(P, 64 * ksplit) - P >= 64                     # at least the last slice lies wholly behind P
    assert paths == ["tiled128", "tiled128", "tiled64", "tiled64T", "tiled64T", "ring128", "ring128", "ring192", "ring192T", "ring128"]


@pytest.mark.parametrize("pname,B,H,W,Cout,Cin,ks,ksplit", WGRAD_CASES, ids=[case_id(c) for c in WGRAD_CASES])
def test_convolution_weight_gradient_matches_fp64(pname, B, H, W, Cout, Cin, ks, ksplit, record_err):
    from nppc_audio import _hip as Hh
    prec, dtype = prec_of(pname)
    bf16 = pname == BF16
    x, dy, (ref, mag) = wgrad_case(pname, B, H, W, Cout, Cin, ks)
    M, N, nt = rup(Cout, 64), Cin, ks * ks
    guard = 64 * ksplit + 128 + W + 4                               # as UNetEngine.buf sizes the rows behind P
    DY = Halo(B, H, W, M, dtype, guard_after=guard).put(dy)         # (columns [Cout, M) and every row behind P: zero)
    X = Halo(B, H, W, N, dtype, guard_after=guard).put(x)
    P = X.P
    n = Cout * Cin * nt
    s = Hh.stream()

    def run(Xh):
        slabs = torch.full((nt * ksplit * rup(M, 128) * N,), NAN, dtype=torch.float32, device="cuda")
        dW = torch.full((n + 64,), SENT, dtype=torch.float32, device="cuda")
        Hh.call("nppc_conv_wgrad", prec, DY.t, M, Xh.t, N, slabs, M, N, B, H, W, ks, ksplit, s)
        Hh.call("nppc_conv_wgrad_reduce", prec, slabs, ksplit, M, N, dW, Cout, Cin, ks, s)
        torch.cuda.synchronize()
        return dW.cpu()

    got = run(X)
    assert bool((got[n:] == SENT).all())                            # nothing behind [Cout][Cin][ks * ks]
    Rz = R.wgrad_rows_per_slab(P, ksplit, bf16)
    record_err("dW", R.ratio(got[:n].view(Cout, Cin, ks, ks).double() - ref, R.conv_wgrad_bound(ref, mag, Rz, bf16)), 1.0)
    assert torch.equal(run(X), got)                                 # fixed summation order
    if bf16:
        # the rows of X behind P hold a finite sentinel, dY stays zero there: bit-identical, so "dY is zero beyond P" is all
        # that the padded slices rely on
        X2 = Halo(B, H, W, N, dtype, guard_after=guard).put(x)
        X2.t[P * N:] = 3.0
        assert torch.equal(run(X2), got)


# path, M, N, Rz, ksplit, shift_a: the nine-tap launch itself, slab by slab, with rows wider than the operands
TAPS_CASES = [("tiled128", 128, 128, 64, 2, 0), ("tiled64", 128, 64, 128, 3, 1),
              ("ring128", 256, 128, 256, 32, 0), ("ring192", 256, 192, 192, 32, 1)]       # 4 / 6 stages in rings of 3 / 5 slots


@pytest.mark.parametrize("path,M,N,Rz,ksplit,shift_a", TAPS_CASES, ids=[case_id(c) for c in TAPS_CASES])
def test_nine_tap_tn_gemm_matches_fp64_slab_by_slab(path, M, N, Rz, ksplit, shift_a, record_err):
    """nppc_gemm_tn_splitk_taps: C[t * ksplit + z][m][n] = sum_{r in slice z} A[r][m] B[r + off_t][n] (shift_a: the offset on
    A's rows), off_t = (t/3 - 1) Wp + (t%3 - 1).  lda > M, ldb > N, ldc > N: the columns behind N keep the sentinel.  Each slab
    is an fp32 sum of Rz exact products: 2 sqrt(Rz) 2^-24 sum |a||b| + 2^-24 |ref| (tests/test_wgrad_reduce_gpu.py)."""
    from nppc_audio import _hip as Hh
    bn = 192 if N % 192 == 0 else (128 if N % 128 == 0 else 0)
    ring = M % 256 == 0 and bn and (M // 256) * (N // bn) * ksplit * 9 >= 256                # launch_tn's condition
    assert bool(ring) == path.startswith("ring")
    Wp, Rr = 15, Rz * ksplit
    G = Wp + 1                                                       # rows the shifted operand reads on either side
    lda, ldb, ldc = M + 8, N + 24, N + 16
    g = torch.Generator().manual_seed(M + N + ksplit)
    a = torch.randn(Rr + 2 * G, lda, generator=g).bfloat16()
    b = torch.randn(Rr + 2 * G, ldb, generator=g).bfloat16()
    C = torch.full((9 * ksplit * M * ldc,), SENT, device="cuda")
    Hh.call("nppc_gemm_tn_splitk_taps", a.cuda().view(-1)[G * lda:], lda, b.cuda().view(-1)[G * ldb:], ldb, C, ldc, M, N, Rr,
            ksplit, Wp, shift_a, Hh.stream())
    torch.cuda.synchronize()
    C = C.cpu().view(9, ksplit, M, ldc)
    assert bool((C[..., N:] == SENT).all())
    a64, b64 = a.double()[:, :M], b.double()[:, :N]
    worst = 0.0
    for t in range(9):
        off = (t // 3 - 1) * Wp + (t % 3 - 1)
        at = a64[G + (off if shift_a else 0):][:Rr].view(ksplit, Rz, M).transpose(1, 2)
        bt = b64[G + (0 if shift_a else off):][:Rr].view(ksplit, Rz, N)
        ref, mag = torch.bmm(at, bt), torch.bmm(at.abs(), bt.abs())
        worst = max(worst, R.ratio(C[t, :, :, :N].double() - ref, 2 * np.sqrt(Rz) * R.U24 * mag + R.U24 * ref.abs()))
    record_err("slabs", worst, 1.0)


# ------------------------------------------------------------------------------------------------ argument guards
def test_entry_points_refuse_what_they_cannot_compute():
    from nppc_audio import _hip as Hh
    prec, dtype = prec_of(BF16)
    B, H, W = 1, 4, 6
    s = Hh.stream()
    X = Halo(B, H, W, 128, dtype)
    Y = out_buf(B, H, W, 128, dtype)
    wf = torch.zeros(128 * 9 * 128, dtype=dtype, device="cuda")
    v = torch.zeros(128, device="cuda")
    part = torch.full((2 * 2 * 128,), NAN, device="cuda")

    def fwd(Cin, Cout, Np, ks, scale=None, shift=None):
        Hh.call("nppc_conv_fwd", prec, X.t, 128, wf, Y.t, 128, v, scale, shift, 0.2, B, H, W, Cin, Cout, Np, ks, s)

    refused = "unsupported|bad argument"
    with pytest.raises(RuntimeError, match=refused):
        fwd(48, 64, 64, 3)                                          # Cin % 32 != 0
    with pytest.raises(RuntimeError, match=refused):
        fwd(64, 96, 96, 3)                                          # Np % 64 != 0
    with pytest.raises(RuntimeError, match=refused):
        fwd(64, 64, 64, 2)                                          # ksize 2
    with pytest.raises(RuntimeError, match=refused):
        fwd(64, 64, 64, 3, scale=v)                                 # scale without shift
    with pytest.raises(RuntimeError, match=refused):
        fwd(64, 128, 64, 3)                                         # Cout > Np
    with pytest.raises(RuntimeError, match=refused):                # a register-path shape leaves no statistics
        Hh.call("nppc_conv_fwd_stats", prec, X.t, 32, wf, Y.t, 128, v, B, H, W, 32, 64, 64, 3, part, s)
    slabs = torch.full((9 * 128 * 128,), NAN, device="cuda")
    dW = torch.full((128 * 128 * 9,), SENT, device="cuda")
    with pytest.raises(RuntimeError, match=refused):
        Hh.call("nppc_conv_wgrad", prec, Y.t, 96, X.t, 128, slabs, 96, 128, B, H, W, 3, 1, s)         # M % 64 != 0
    with pytest.raises(RuntimeError, match=refused):
        Hh.call("nppc_conv_wgrad", prec, Y.t, 128, X.t, 128, slabs, 128, 128, B, H, W, 3, 0, s)       # ksplit 0
    with pytest.raises(RuntimeError, match=refused):
        Hh.call("nppc_conv_wgrad_reduce", prec, slabs, 1, 64, 128, dW, 128, 128, 3, s)                # Cout > M
    torch.cuda.synchronize()
    # refused, not computed: nothing was written
    assert untouched_outside(Y, 0, 0) and bool(torch.isnan(part).all()) and bool(torch.isnan(slabs).all())
    assert bool((dW == SENT).all())
