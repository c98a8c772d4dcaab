"""The convolution references and bounds of tests/unet_ref.py (conv_ref, conv_dx_ref, conv_wgrad_ref, conv_bound,
conv_wgrad_bound), checked without a GPU: honest fp32 arithmetic stays inside the bounds, subtly wrong arithmetic falls
outside, and the row-shifted products over the haloed matrix (unet_halo.Halo) that the kernels compute are the convolution
and its weight gradient.  tests/test_unet_conv_gpu.py compares the kernels of csrc/unet.hip with exactly these."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
from unet_halo import Halo

# (B, H, W, Cin, Cout, ks): one K slice per tap / several, one tap / nine, a 256-row tile mostly halo / several tiles
SHAPES = [pytest.param(2, 9, 13, 64, 64, 3, id="9x13-64to64-3x3"), pytest.param(2, 9, 13, 256, 128, 3, id="9x13-256to128-3x3"),
          pytest.param(2, 4, 6, 64, 64, 1, id="4x6-64to64-1x1"), pytest.param(2, 30, 29, 128, 256, 3, id="30x29-128to256-3x3")]
STORAGE = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float32, id="fp32")]


@functools.lru_cache(maxsize=None)
def operands(B, H, W, Cin, Cout, ks, dtype):
    """operands rounded to the storage dtype, and their fp64 references (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(1000 * B + 10 * Cin + Cout + ks + H)
    x = R.q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = R.q(torch.randn(Cout, Cin, ks, ks, generator=g) / np.sqrt(Cin * ks * ks), dtype)
    b = torch.randn(Cout, generator=g) * 0.1
    dy = R.q(torch.randn(B, Cout, H, W, generator=g), dtype)
    fold = (torch.where(torch.arange(Cout) % 2 == 0, 1.0, -1.0) * (torch.rand(Cout, generator=g) + 0.5),
            torch.randn(Cout, generator=g) * 0.1)
    return x, w, b, dy, fold, R.conv_ref(x, w, b, ks), R.conv_ref(x, w, b, ks, fold), R.conv_wgrad_ref(dy, x, ks)


def rowshift_conv(x, w, b, ks, dtype, drop=None, bad_tap=None):
    """raw[p][co] = bias[co] + sum_t X[p + off(t)] W_t^T over the haloed rows, interior pixels kept: what the kernels compute,
    in `dtype`.  drop = (tap, first channel): that 64-channel K slice is left out; bad_tap: that tap reads one row too far."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    X = Halo(B, H, W, Cin, dtype, guard_after=W + 8, device="cpu").put(x)
    wt = w.to(dtype).reshape(Cout, Cin, ks * ks)
    acc = b.to(dtype)[None, :].repeat(X.P, 1)
    for t, off in enumerate(R.tap_offsets(ks, W)):
        a, wk = X.rows(off + (1 if t == bad_tap else 0)), wt[:, :, t]
        if drop is not None and drop[0] == t:
            keep = torch.ones(Cin, dtype=torch.bool)
            keep[drop[1]:drop[1] + 64] = False
            a, wk = a[:, keep], wk[:, keep]
        acc = acc + a @ wk.T
    return acc.view(B, H + 2, W + 2, Cout)[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous()


def rowshift_wgrad(dy, x, ks, ksplit, dtype, drop_slice=None):
    """dW[co][ci][t] = sum_s sum_{p in slice s} dY[p][co] X[p + off(t)][ci] with the rows rounded up as nppc_conv_wgrad rounds
    them (R = roundup(P, 64 ksplit); dY is zero behind P), slabs in `dtype`, added in fp64"""
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    P = B * (H + 2) * (W + 2)
    Rz = R.wgrad_rows_per_slab(P, ksplit, True)
    guard = Rz * ksplit - P + W + 8
    X = Halo(B, H, W, Cin, dtype, guard_after=guard, device="cpu").put(x)
    DY = Halo(B, H, W, Cout, dtype, guard_after=guard, device="cpu").put(dy)
    dW = torch.zeros(Cout, Cin, ks * ks, dtype=torch.float64)
    for t, off in enumerate(R.tap_offsets(ks, W)):
        for s in range(ksplit):
            if s != drop_slice:
                dW[:, :, t] += (DY.rows(s * Rz, Rz).T @ X.rows(s * Rz + off, Rz)).double()
    return dW.view(Cout, Cin, ks, ks)


def stored(y, dtype):
    return R.q(y.float(), dtype).double()


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", SHAPES[:3])
def test_row_shifted_products_over_the_haloed_matrix_are_the_convolution_and_its_weight_gradient(B, H, W, Cin, Cout, ks):
    x, w, b, dy, _, cr, _, (dw_ref, dw_mag) = operands(B, H, W, Cin, Cout, ks, torch.bfloat16)
    eps = 2.0 ** -52
    got = rowshift_conv(x.double(), w.double(), b.double(), ks, torch.float64)
    assert R.ratio(got - cr.ref, (ks * ks * Cin + 1) * eps * cr.mag) <= 1.0
    # autograd's weight gradient, the reference and the row-shifted slices agree
    wr = w.double().clone().requires_grad_(True)
    F.conv2d(x.double(), wr, None, padding=ks // 2).backward(dy.double())
    n = B * H * W
    assert R.ratio(wr.grad - dw_ref, n * eps * dw_mag) <= 1.0
    for ksplit in (1, 3):
        assert R.ratio(rowshift_wgrad(dy.double(), x.double(), ks, ksplit, torch.float64) - dw_ref, n * eps * dw_mag) <= 1.0
    # the input gradient reference is autograd's
    xr = x.double().clone().requires_grad_(True)
    F.conv2d(xr, w.double(), None, padding=ks // 2).backward(dy.double())
    dx = R.conv_dx_ref(dy, w, ks)
    assert R.ratio(xr.grad - dx.ref, (ks * ks * Cout + 1) * eps * dx.mag) <= 1.0
    assert R.tap_offsets(3, W)[0] == -(W + 2) - 1 and R.tap_offsets(3, W)[4] == 0 and R.tap_offsets(1, W) == [0]


def test_rows_per_slab_follow_the_entry_point():
    # bf16: R = roundup(P, 64 ksplit); P = 330: ksplit 3 -> R = 384; P = 1984: ksplit 32 -> 2048, 64 -> 4096
    assert R.wgrad_rows_per_slab(330, 3, True) == 128 and R.wgrad_rows_per_slab(330, 1, True) == 384
    assert R.wgrad_rows_per_slab(1984, 32, True) == 64 and R.wgrad_rows_per_slab(1984, 64, True) == 64
    # fp32: roundup(ceil(P / ksplit), 16)
    assert R.wgrad_rows_per_slab(330, 3, False) == 112 and R.wgrad_rows_per_slab(330, 24, False) == 16


# ------------------------------------------------------------------------------------------------ honest arithmetic
@pytest.mark.parametrize("dtype", STORAGE)
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", SHAPES)
def test_fp32_convolution_of_torch_stays_inside_the_bounds(B, H, W, Cin, Cout, ks, dtype):
    bf16 = dtype == torch.bfloat16
    x, w, b, dy, fold, cr, crf, _ = operands(B, H, W, Cin, Cout, ks, dtype)
    K = ks * ks * Cin
    y = F.conv2d(x, w, b, padding=ks // 2)
    r = R.ratio(stored(y, dtype) - cr.ref, R.conv_bound(cr, K, bf16))
    yf = F.leaky_relu(y * fold[0][None, :, None, None] + fold[1][None, :, None, None], 0.2)
    rf = R.ratio(stored(yf, dtype) - crf.ref, R.conv_bound(crf, K, bf16, fold))
    xr = x.clone().requires_grad_(True)
    F.conv2d(xr, w, None, padding=ks // 2).backward(dy)
    dx = R.conv_dx_ref(dy, w, ks)
    rd = R.ratio(stored(xr.grad, dtype) - dx.ref, R.conv_bound(dx, ks * ks * Cout, bf16))
    print(f"forward {r:.3f} folded {rf:.3f} input gradient {rd:.3f} of the bound")
    assert r < 1.0 and rf < 1.0 and rd < 1.0
    assert bool((fold[0] > 0).any()) and bool((fold[0] < 0).any())          # the leaky branch is taken on both sides of zero
    v = crf.raw * fold[0].double()[None, :, None, None] + fold[1].double()[None, :, None, None]
    assert bool((v > 0).any()) and bool((v < 0).any())


@pytest.mark.parametrize("dtype,ksplits", [pytest.param(torch.bfloat16, (1, 3, 32), id="bf16"),
                                           pytest.param(torch.float32, (3, 24), id="fp32")])
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", SHAPES)
def test_fp32_weight_gradient_of_autograd_stays_inside_the_bounds(B, H, W, Cin, Cout, ks, dtype, ksplits):
    bf16 = dtype == torch.bfloat16
    x, w, b, dy, _, _, _, (ref, mag) = operands(B, H, W, Cin, Cout, ks, dtype)
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, padding=ks // 2).backward(dy)
    P = B * (H + 2) * (W + 2)
    for ksplit in ksplits:
        r = R.ratio(wr.grad.double() - ref, R.conv_wgrad_bound(ref, mag, R.wgrad_rows_per_slab(P, ksplit, bf16), bf16))
        print(f"ksplit {ksplit}: {r:.3f} of the bound")
        assert r < 1.0
    # the slabs of the row-shifted formulation in fp32, added in fp64: what the kernels do
    got = rowshift_wgrad(dy, x, ks, 3, torch.float32)
    assert R.ratio(got - ref, R.conv_wgrad_bound(ref, mag, R.wgrad_rows_per_slab(P, 3, True), bf16)) < 1.0


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("dtype", STORAGE)
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", SHAPES)
def test_wrong_convolutions_fall_outside_the_bound(B, H, W, Cin, Cout, ks, dtype):
    bf16 = dtype == torch.bfloat16
    x, w, b, dy, fold, cr, _, _ = operands(B, H, W, Cin, Cout, ks, dtype)
    bound = R.conv_bound(cr, ks * ks * Cin, bf16)
    mid = ks * ks // 2                   # the centre tap: every pixel reads it
    assert R.ratio(stored(rowshift_conv(x, w, b, ks, torch.float32), dtype) - cr.ref, bound) < 1.0       # the honest one
    # one 64-channel K slice of one tap dropped
    err = (stored(rowshift_conv(x, w, b, ks, torch.float32, drop=(mid, Cin - 64)), dtype) - cr.ref).abs()
    assert R.ratio(err, bound) > 1.0 and float((err > bound).double().mean()) > 0.9
    # one tap's row offset off by one pixel
    assert R.ratio(stored(rowshift_conv(x, w, b, ks, torch.float32, bad_tap=mid), dtype) - cr.ref, bound) > 1.0
    # one small element off by eight times its bound: max |diff| / max |ref| < 3e-2 over the tensor lets it pass
    if bf16:
        y = stored(rowshift_conv(x, w, b, ks, torch.float32), dtype)
        i = int(cr.ref.abs().reshape(-1).argmin())
        y.view(-1)[i] += 8 * float(bound.reshape(-1)[i])
        assert R.ratio(y - cr.ref, bound) > 1.0 and R.rel(y, cr.ref) < 3e-2


@pytest.mark.parametrize("dtype", STORAGE)
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", SHAPES)
def test_wrong_weight_gradients_fall_outside_the_bound(B, H, W, Cin, Cout, ks, dtype):
    bf16 = dtype == torch.bfloat16
    x, w, b, dy, _, _, _, (ref, mag) = operands(B, H, W, Cin, Cout, ks, dtype)
    P = B * (H + 2) * (W + 2)
    # the loosest bound any case of the GPU test uses for this shape: one slab of all the rows
    bound = R.conv_wgrad_bound(ref, mag, R.wgrad_rows_per_slab(P, 1, bf16), bf16)
    assert R.ratio(rowshift_wgrad(dy, x, ks, 3, torch.float32) - ref, bound) < 1.0
    # one split-K slice dropped
    assert R.ratio(rowshift_wgrad(dy, x, ks, 3, torch.float32, drop_slice=1) - ref, bound) > 1.0
    # dW returned transposed in (co, ci): [ci][co] memory read as [co][ci]
    good = rowshift_wgrad(dy, x, ks, 3, torch.float32)
    assert R.ratio(good.permute(1, 0, 2, 3).contiguous().view_as(good) - ref, bound) > 1.0
    # the taps in the order of the backward pack (flipped)
    if ks == 3:
        assert R.ratio(good.flip(2, 3) - ref, bound) > 1.0
