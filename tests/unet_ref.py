"""fp64 references and derived error bounds for the kernels of csrc/unet.hip (BatchNorm, pooling, upsampling, the boundary
maps, the MFMA convolutions and their weight gradients) and the dropout bits of csrc/mc_pca.hip.  numpy / torch-CPU only:
imports without a GPU.

Every bound here is derived from the arithmetic the kernel is specified to do (how many fp32 roundings a value goes
through, how long a chain of fp32 additions is), never from what a kernel returned."""
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24           # unit roundoff of fp32
U8 = 2.0 ** -8             # unit roundoff of bf16 (round to nearest even)
M32 = 0xFFFFFFFF
SLOPE = 0.2
SLOPE_F32 = float(np.float32(SLOPE))      # the kernels take the slope as a float


def ratio(err, bound):
    """max err / bound over the elements; 0 where both are 0, inf where only the bound is: <= 1 iff err <= bound everywhere"""
    err = np.abs(np.asarray(err, np.float64)).reshape(-1)
    bound = np.asarray(bound, np.float64).reshape(-1)
    assert err.shape == bound.shape and np.all(bound >= 0) and np.all(np.isfinite(bound))
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def rel(a, b):
    """max |a - b| / max |b| (the project's existing measure)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def q(x, dtype):
    """round to the storage dtype: the kernels see these values exactly"""
    return x.to(dtype).float()


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_rows_per_block(P):
    """rows of the haloed matrix per workgroup of bn_stats_kernel / bn_bwd_reduce_kernel:
    max(1024, roundup256(ceil(P / 512)))"""
    r = (P + 511) // 512
    r = (r + 255) // 256 * 256
    return max(1024, r)


def bn_row_lanes(C):
    """row lanes of those kernels: 256 threads over C / 8 channel groups"""
    return 256 // (C // 8)


def bn_workgroups(P):
    return (P + bn_rows_per_block(P) - 1) // bn_rows_per_block(P)


def bn_chain(P, C):
    """m: the longest chain of fp32 additions of one thread of bn_bwd_reduce_kernel (rows it walks in its workgroup)"""
    rpb, rl = bn_rows_per_block(P), bn_row_lanes(C)
    return (rpb + rl - 1) // rl


def bn_stats_ref(x):
    """x [B,C,H,W] (exact storage values) -> (sum x, sum x^2, sum |x|) per channel, fp64"""
    x = x.double()
    return x.sum((0, 2, 3)).numpy(), (x * x).sum((0, 2, 3)).numpy(), x.abs().sum((0, 2, 3)).numpy()


def bn_finalize_ref(s1, s2, n, gamma, beta, rmean, rvar, eps=1e-5, momentum=0.1):
    """train-mode BatchNorm2d from the sums: (scale, shift, mean, rstd, running mean, running var), fp64.  eps and momentum
    reach the kernel as floats."""
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = g * rstd
    rm = (1.0 - momentum) * np.asarray(rmean, np.float64) + momentum * mean
    rv = (1.0 - momentum) * np.asarray(rvar, np.float64) + momentum * var * (n / max(n - 1.0, 1.0))
    return scale, b - mean * scale, mean, rstd, rm, rv


def _bc(v):
    return torch.as_tensor(np.asarray(v, np.float64))[None, :, None, None]


def bn_preact(x, scale, shift):
    """v = x * scale + shift in fp64 (scale, shift: the fp32 values of the device, or their fp64 references)"""
    return x.double() * _bc(scale) + _bc(shift)


def bn_act_ref(x, scale, shift, storage_bf16):
    """-> (y, bound): y = leaky(x sc + sh); the device rounds the product, the sum (or one fused rounding) and the slope
    product: 3 * 2^-24 * (|x sc| + |sh|), plus half an ulp of the storage in bf16"""
    xs = x.double() * _bc(scale)
    v = xs + _bc(shift)
    y = torch.where(v > 0, v, SLOPE_F32 * v)
    bound = 3 * U24 * (xs.abs() + _bc(shift).abs())
    if storage_bf16:
        bound = bound + U8 * y.abs()
    return y, bound


def bn_condition(x, gamma, beta, dtype, eps=1e-5, band=1e-3, step=1e-2, rounds=20):
    """Move every element whose pre-activation x*sc + sh lies within `band` of zero away from it (by `step`, or one storage ulp
    where that is larger), re-round to the storage dtype and repeat until none is left: the device recomputes the LeakyReLU
    mask from x*sc + sh > 0 in fp32, and a single sign flip of a value at rounding distance from zero would decide a tight
    bound.  -> the conditioned x (asserted clean)."""
    x = q(x, dtype)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    for _ in range(rounds):
        s1, s2, _ = bn_stats_ref(x)
        sc, sh, *_ = bn_finalize_ref(s1, s2, float(n), gamma, beta, np.zeros_like(s1), np.ones_like(s1), eps)
        v = bn_preact(x, sc, sh)
        bad = v.abs() < band
        if not bool(bad.any()):
            break
        sgn = torch.where(v >= 0, 1.0, -1.0) * torch.sign(_bc(sc))
        ulps = x.double().abs() * (2.0 ** -6 if dtype == torch.bfloat16 else 0.0)        # two bf16 ulps at least
        moved = x.double() + sgn * torch.clamp(ulps, min=step)
        x = q(torch.where(bad, moved, x.double()).float(), dtype)
    assert bn_near_zero(x, sc, sh, band) == 0
    return x


def bn_near_zero(x, scale, shift, band=1e-3):
    return int((bn_preact(x, scale, shift).abs() < band).sum())


def drop_scale_f32(p):
    """1 / (1 - p) as the host computes it, in fp32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def bn_bwd_sums_ref(x, ss, dya, dyb=None, keep=None, p=0.0):
    """The reduction of the BatchNorm + LeakyReLU (+ dropout) backward from the device's own fp32 ss = (scale, shift, mean,
    rstd): g = (dyA + dyB) * keep / (1 - p) * leaky'(x sc + sh), S1 = sum g, S2 = sum g * xhat, xhat = (x - mean) rstd.
    -> (S1, S2, sum |g|, sum |g xhat|) per channel and g, xhat, all fp64."""
    C = x.shape[1]
    ss = np.asarray(ss, np.float64)
    sc, sh, mean, rstd = ss[:C], ss[C:2 * C], ss[2 * C:3 * C], ss[3 * C:]
    g = dya.double() if dyb is None else dya.double() + dyb.double()
    if keep is not None:
        g = g * keep.double() * drop_scale_f32(p)
    v = bn_preact(x, sc, sh)
    g = torch.where(v > 0, g, SLOPE_F32 * g)
    xh = (x.double() - _bc(mean)) * _bc(rstd)
    gx = g * xh
    return (g.sum((0, 2, 3)).numpy(), gx.sum((0, 2, 3)).numpy(), g.abs().sum((0, 2, 3)).numpy(),
            gx.abs().sum((0, 2, 3)).numpy(), g, xh)


def bn_bwd_sum_bounds(P, C, abs_g, abs_gx):
    """A thread adds its m = bn_chain(P, C) rows in fp32 (<= m roundings of the running sum) after at most 4 roundings of the
    term itself (dyA + dyB, the dropout factor, the slope; one spare) -- 8 for g * xhat (x - mean, * rstd, the product; one
    spare) --, then everything is fp64: (m + 4) 2^-24 sum |g| and (m + 8) 2^-24 sum |g xhat| per channel."""
    m = bn_chain(P, C)
    return (m + 4) * U24 * abs_g, (m + 8) * U24 * abs_gx


def bn_dx_ref(ss, S1, S2, g, xh, n):
    C = g.shape[1]
    sc = np.asarray(ss, np.float64)[:C]
    return _bc(sc) * (g - _bc(S1 / n) - xh * _bc(S2 / n))


# ------------------------------------------------------------------------------------------------ pooling
def tie_alphabet(shape, gen):
    """values from {-1, -0.0, 0.0, 1}: 2x2 windows tie for their maximum most of the time"""
    a = torch.tensor([-1.0, -0.0, 0.0, 1.0])
    return a[torch.randint(0, 4, shape, generator=gen)]


def maxpool_first_max_ref(x):
    """MaxPool2d(2), floor mode: the first maximum in window scan order (y, then x) wins (strict >).
    -> (y [B,C,Ho,Wo], idx in 0..3)"""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    win = x[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)
    best, idx = win[..., 0].clone(), torch.zeros(B, C, Ho, Wo, dtype=torch.long)
    for t in range(1, 4):
        better = win[..., t] > best
        best = torch.where(better, win[..., t], best)
        idx = torch.where(better, torch.full_like(idx, t), idx)
    return best, idx


def maxpool_bwd_ref(dy, idx, H, W, fill=0.0):
    """dy routed to the recorded position, 0 at the other three; positions outside every window hold `fill`"""
    B, C, Ho, Wo = dy.shape
    win = torch.zeros(B, C, Ho, Wo, 4, dtype=dy.dtype)
    win.scatter_(4, idx[..., None], dy[..., None])
    dx = torch.full((B, C, H, W), fill, dtype=dy.dtype)
    dx[:, :, :2 * Ho, :2 * Wo] = win.reshape(B, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * Ho, 2 * Wo)
    return dx


def tie_fraction(x):
    """fraction of the 2x2 windows whose maximum is attained more than once"""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    win = x[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)
    return float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).float().mean())


# ------------------------------------------------------------------------------------------------ upsampling
def upsample_pad_ref(x, Ht, Wt):
    """nn.Upsample(scale_factor=2, bilinear, align_corners=True) + F.pad to (Ht, Wt), in the dtype of x (fp32 is the
    definition: the source index arithmetic is fp32).  -> (padded result, (py, px) of the window)"""
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = Ht - up.shape[2], Wt - up.shape[3]
    return F.pad(up, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2)), (dy // 2, dx // 2)


# ------------------------------------------------------------------------------------------------ boundary maps
EPS_LOG_F32 = float(np.float32(1e-6))


def logmag_ref(spec):
    """spec [B,2,F,T] fp32 -> log(|z| + 1e-6f) in fp64; bound 8 * 2^-24 * max(1, |ref|): squares, sum, square root, the
    added constant (<= 2.5 roundings of the logarithm's argument, each worth 2^-24 absolute in the logarithm) and a logf of
    one ulp of its result"""
    z = spec.double()
    ref = torch.log(torch.sqrt(z[:, 0] ** 2 + z[:, 1] ** 2) + EPS_LOG_F32)
    return ref, 8 * U24 * torch.clamp(ref.abs(), min=1.0)


def standardize_ref(a, s1, s2, n):
    """(a - mean) / std with the batch-global mean and unbiased std from (sum, sum of squares) -> (ref, bound, mean, std).
    The device rounds mean and std to fp32 (2^-24 |m| / s and 2^-24 |a - m| / s), the difference and the quotient:
    <= 2^-24 (|m| + 3 |a - m|) / s <= 4 * 2^-24 (|a| + |m|) / s"""
    mean = s1 / n
    std = float(np.sqrt(max((s2 - n * mean * mean) / (n - 1.0), 0.0)))
    a = a.double()
    return (a - mean) / std, 4 * U24 * (a.abs() + abs(mean)) / std, mean, std


def unet_out_ref(raw, mask, xin=None):
    """raw [B,K,H,W] (storage values), mask [B,W], xin [B,H,W] or None -> (out, bound): mode 0 raw (1 - m), mode 1
    x m + raw (1 - m).  Roundings: 1 - m, both products, the sum: 3 * 2^-24 (|x m| + |r (1 - m)|)"""
    m = mask.double()[:, None, None, :]
    t2 = raw.double() * (1.0 - m)
    t1 = torch.zeros_like(t2) if xin is None else xin.double()[:, None] * m
    return t1 + t2, 3 * U24 * (t1.abs() + t2.abs())


def unet_out_bwd_ref(dout, mask, storage_bf16):
    """dRaw = dOut (1 - m): two fp32 roundings (1 - m, the product), 3 * 2^-24 |ref| with the second-order terms, plus the
    storage rounding in bf16"""
    ref = dout.double() * (1.0 - mask.double()[:, None, None, :])
    return ref, (3 * U24 + (U8 if storage_bf16 else 0.0)) * ref.abs()


# ------------------------------------------------------------------------------------------------ dropout bits
def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """vectorised Philox4x32-10 (Salmon et al. 2011), the same rounds as vad_ref.philox4x32_10: uint64 arrays / scalars
    holding 32-bit words -> four uint64 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(M32) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def dropout_threshold(p):
    """floor(p * 2^32) with p as the fp32 the entry point receives, clamped to the u32 range"""
    return min(int(float(np.float32(p)) * 4294967296.0), M32)


def dropout_keep_ref(rows, C, p, seed, stream_id, philox=None):
    """keep[r][4 c4 + i] = word i of Philox(counter (r lo, r hi, c4, stream), key (seed lo, seed hi)) >= threshold(p)
    -> uint8 [rows][C].  philox: a scalar generator (counter, key) -> 4 words, e.g. vad_ref.philox4x32_10; default the
    vectorised one above."""
    th = dropout_threshold(p)
    key = (seed & M32, (seed >> 32) & M32)
    if philox is not None:
        out = np.empty((rows, C), np.uint8)
        for r in range(rows):
            for c4 in range(C // 4):
                w = philox((r & M32, r >> 32, c4, stream_id), key)
                out[r, 4 * c4:4 * c4 + 4] = [int(wi >= th) for wi in w]
        return out
    r = np.arange(rows, dtype=np.uint64)[:, None] + np.zeros((1, C // 4), np.uint64)
    c4 = np.arange(C // 4, dtype=np.uint64)[None, :] + np.zeros((rows, 1), np.uint64)
    w = philox4x32_10_np(r & np.uint64(M32), r >> np.uint64(32), c4, np.full_like(r, stream_id), *key)
    return (np.stack(w, -1) >= np.uint64(th)).astype(np.uint8).reshape(rows, C)


def keep_nchw(keep, B, H, W):
    """[rows][C] keep bits over the haloed rows -> [B,C,H,W] float64 (interior)"""
    C = keep.shape[1]
    return torch.from_numpy(keep.reshape(B, H + 2, W + 2, C)[:, 1:-1, 1:-1].astype(np.float64)).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ MFMA convolutions
class ConvRef(NamedTuple):
    ref: torch.Tensor        # [B,Cout,H,W] fp64: the convolution (+ bias), through the folded epilogue where one was given
    mag: torch.Tensor        # sum |x| |w| + |bias| of the convolution itself (before the fold)
    raw: torch.Tensor        # the convolution (+ bias) before the fold (== ref without one)


def conv_ref(x, w, bias, ks, fold=None, slope=SLOPE):
    """x [B,Cin,H,W], w [Cout,Cin,ks,ks]: the values the kernel reads (activations and packed weights already rounded to the
    storage dtype, see q), bias [Cout] fp32 or None, fold = (scale, shift) fp32 or None.  fp64 F.conv2d with zero padding
    ks // 2, then optionally leaky(v * scale + shift) with the slope as the fp32 the kernel is handed."""
    b64 = None if bias is None else bias.double()
    raw = F.conv2d(x.double(), w.double(), b64, padding=ks // 2)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None if b64 is None else b64.abs(), padding=ks // 2)
    if fold is None:
        return ConvRef(raw, mag, raw)
    v = raw * _bc(fold[0].double()) + _bc(fold[1].double())
    return ConvRef(torch.where(v > 0, v, float(np.float32(slope)) * v), mag, raw)


def conv_dx_ref(dy, w, ks):
    """input gradient of the same convolution: dy [B,Cout,H,W], w [Cout,Cin,ks,ks] (exact storage values) -> ConvRef of
    [B,Cin,H,W] (the transposed convolution the forward kernel computes on the backward pack)"""
    ref = F.conv_transpose2d(dy.double(), w.double(), padding=ks // 2)
    return ConvRef(ref, F.conv_transpose2d(dy.double().abs(), w.double().abs(), padding=ks // 2), ref)


def conv_bound(cr, K, storage_bf16, fold=None):
    """Element-wise bound on |kernel - cr.ref| of nppc_conv_fwd, K = ntap * Cin products per output.

    * The kernels add the K products (and the bias) in fp32.  bf16 x bf16 products are exact in fp32, so the error is that of
      the summation alone: its roundings are each at most 2^-24 of a partial sum <= mag and of either sign, and the project
      budgets such a chain at acc = 2 sqrt(K) 2^-24 mag (test_tcn_forward_gpu.py, test_wgrad_reduce_gpu.py) -- between the
      sqrt(K) of independent roundings and the K of the worst case.  fp32 operands: every product is rounded too, at most
      2^-24 |x w| each, together <= 2^-24 mag more.
    * Folded epilogue v = raw * scale + shift, leaky(v): the error of raw goes through |scale|; the product and the sum are
      rounded (one rounding where they fuse): <= 2^-24 (|raw scale| + |v|) <= 2 * 2^-24 (|raw scale| + |shift|) to first order.
      LeakyReLU is 1-Lipschitz, so a branch decided differently at a v within that error of zero costs no more than the
      error itself; on the negative side the slope (<= 1) shrinks both roundings to 0.4 and adds its own product rounding,
      0.2 * 2^-24 |v|: less than the 2 budgeted.
    * The store rounds once more: u_out (|ref| + e), u_out = 2^-8 (bf16, round to nearest even: exactly the worst case) or
      2^-24.
    bound = e + u_out (|ref| + e),   e = acc  or  |scale| acc + 2 * 2^-24 (|raw scale| + |shift|)."""
    acc = (2.0 * np.sqrt(K) + (0.0 if storage_bf16 else 1.0)) * U24 * cr.mag
    e = acc
    if fold is not None:
        sc, sh = _bc(fold[0].double()), _bc(fold[1].double())
        e = sc.abs() * acc + 2 * U24 * ((cr.raw * sc).abs() + sh.abs())
    return e + (U8 if storage_bf16 else U24) * (cr.ref.abs() + e)


def conv_wgrad_ref(dy, x, ks):
    """dW[co][ci][tap] = sum_p dY[p][co] X[p + off(tap)][ci] over the pixels, X zero outside the image: dy [B,Cout,H,W],
    x [B,Cin,H,W] (exact storage values) -> (dW [Cout,Cin,ks,ks] fp64, sum |dY| |X| of the same shape)"""
    r = ks // 2
    H, W = x.shape[2:]
    dy, xp = dy.double(), F.pad(x.double(), (r, r, r, r))
    ref = torch.empty(dy.shape[1], x.shape[1], ks, ks, dtype=torch.float64)
    mag = torch.empty_like(ref)
    for ty in range(ks):
        for tx in range(ks):
            win = xp[:, :, ty:ty + H, tx:tx + W]
            ref[:, :, ty, tx] = torch.einsum("bohw,bihw->oi", dy, win)
            mag[:, :, ty, tx] = torch.einsum("bohw,bihw->oi", dy.abs(), win.abs())
    return ref, mag


def wgrad_rows_per_slab(P, ksplit, storage_bf16):
    """rows of the haloed matrix that one split-K slab of nppc_conv_wgrad sums: bf16 rounds the row count up to
    R = roundup(P, 64 ksplit) and gives every slice R / ksplit; the fp32 kernel gives roundup(ceil(P / ksplit), 16)"""
    if storage_bf16:
        return (P + 64 * ksplit - 1) // (64 * ksplit) * 64
    return ((P + ksplit - 1) // ksplit + 15) // 16 * 16


def conv_wgrad_bound(ref, mag, Rz, storage_bf16):
    """Element-wise bound on dW after nppc_conv_wgrad_reduce.  A slab is an fp32 sum of Rz products (most of them the zeros
    of the halo): 2 sqrt(Rz) 2^-24 of its own magnitude sum, as for the convolution above, and one more 2^-24 of it for the
    slab as an fp32 number (the block sums a matrix instruction adds to its accumulator); over the slabs the magnitude sums
    add up to mag.  The reduction adds the slabs in fp64 and rounds once: 2^-24 |ref|.  fp32 operands: the products are
    rounded, 2^-24 mag more.
    bound = (2 sqrt(Rz) + 1 [+ 1]) 2^-24 mag + 2^-24 |ref|"""
    return (2.0 * np.sqrt(Rz) + 1.0 + (0.0 if storage_bf16 else 1.0)) * U24 * mag + U24 * ref.abs()


def tap_offsets(ks, W):
    """row offsets of the taps in the haloed matrix, in the kernels' tap order t = 3 ty + tx"""
    return [(t // 3 - 1) * (W + 2) + (t % 3 - 1) for t in range(9)] if ks == 3 else [0]
