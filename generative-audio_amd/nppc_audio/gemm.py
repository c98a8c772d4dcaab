"""Keyword front ends of the NT-GEMM and slab-reduction entry points (include/nppc_hip.h), and the choice among the LSTM
weight-gradient GEMM strategies.

The C entry points take up to 30 positional arguments, and ctypes checks only their number (`int` and `long` are
interchangeable to it), so two swapped leading dimensions load and run.  These functions name every operand, build the
positional list in the order of `_hip.SIGS` and hand it to `H.call`.  They pass what they are given through untouched: no
`.contiguous()`, no views, no derived leading dimensions.

An operand is a `(tensor, ld, batch_stride)` triple, a per-batch vector a `(tensor, batch_stride)` pair; an absent one is None.
"""
from . import _hip as H

_NO_VEC = (None, 0)
_NO_MAT = (None, 0, 0)


def lstm_wgrad_mode(prec, Hd, KX, Tv, S, have_guards):
    """(strategy, fold_bias) of the LSTM weight gradients (FSNEngine._lstm_wgrad) with S K-slices: "fused2" (two
    nppc_gemm_tn_splitk2 passes, one per layer), "tn" (one split-K TN product per gradient; fold_bias: the layer-2 bias
    gradient rides in the W_ih_l1 product) or "generic" (transposes + the NT split-K GEMM: fp32, small hidden sizes).
    have_guards: the forward kept the guard views of the h rows, which fused2 reads as h_{t-1}."""
    K4 = 4 * Hd
    if not (prec == H.PREC_BF16 and K4 % 128 == 0 and Hd % 64 == 0 and KX % 64 == 0):
        return "generic", False
    fold_bias = K4 % 256 == 0 and Hd % 128 == 0 and (K4 // 256) * (Hd // 128) * S >= 256
    if (have_guards and fold_bias and Hd % 192 == 0 and KX == 64 and Tv > 1
            and (K4 // 256) * (Hd // 192 + 1) * S >= 256):
        return "fused2", True
    return "tn", fold_bias


def gemm_nt(prec, epi, *, A, B, C, R, N, K, Tp, Tv, Nv, bias=None, res=None, slope=None, stats=None, relu_in=0, batch=1,
            ksplit=1, colpart=None, stream):
    """C[R][N] = A[R][K] * B[N][K]^T + epilogue `epi` (`nppc_gemm_nt`).  With `colpart` [batch][R/128][N] fp32 the launch also
    leaves the column sums of every 128-row output tile there (`nppc_gemm_nt_colsum`: no slope, stats, relu_in or ksplit)."""
    front = (prec, epi, *A, *B, *C, *(bias or _NO_VEC), *(res or _NO_MAT))
    if colpart is None:
        H.call("nppc_gemm_nt", *front, *(slope or _NO_VEC), *(stats or _NO_VEC), R, N, K, Tp, Tv, Nv, relu_in, batch, ksplit,
               stream)
        return
    if slope is not None or stats is not None or relu_in != 0 or ksplit != 1:
        raise ValueError("nppc_gemm_nt_colsum takes no slope, stats, relu_in or ksplit")
    H.call("nppc_gemm_nt_colsum", *front, R, N, K, Tp, Tv, Nv, batch, colpart, stream)


def gemm_nt_gn(prec, *, A, B, C, u, v, uv_stride, res, stats, count, eps, R, N, K, Tp, Tv, Nv, batch=1, stream):
    """the sconv product with the GroupNorm in front of it folded in (`nppc_gemm_nt_gn`): C = rstd_b * (A B^T) - mean_b *
    rstd_b * v + u + res; `stats` = the per-sample (sum, sumsq) of A, `count` = elements per sample"""
    H.call("nppc_gemm_nt_gn", prec, *A, *B, *C, u, v, uv_stride, *res, *stats, count, eps, R, N, K, Tp, Tv, Nv, batch, stream)


def reduce_slabs(slab, S, *, slab_stride, ld, dst, dst_ld, rows, col0=0, ncols, permH=0, accumulate=0, batch=1, s_slab=0,
                 s_dst=0, stream):
    """dst[r][c] (+)= sum of the S fp32 slabs at [r][col0 + c], c < ncols (`nppc_reduce_slabs`); permH = H: slab row unit * 4 + gate
    (i, g, f, o) goes to the LSTM's row gate (i, f, g, o) * H + unit"""
    H.call("nppc_reduce_slabs", slab, S, slab_stride, ld, dst, dst_ld, rows, col0, ncols, permH, accumulate, s_slab, s_dst,
           batch, stream)


def reduce_slabs_t(slab, S, *, slab_stride, ld, dst, dst_ld, rows, ncols, batch=1, s_slab=0, s_dst=0, stream):
    """dst[r][c] = sum of the S fp32 slabs at [c][r]: the transposed result (`nppc_reduce_slabs_t`)"""
    H.call("nppc_reduce_slabs_t", slab, S, slab_stride, ld, dst, dst_ld, rows, ncols, s_slab, s_dst, batch, stream)
