"""GPU: the weight-gradient path -- the batched split-K TN GEMM (csrc/tcn.hip launch_tn), the slab reductions into the
parameter gradients (csrc/train_ops.hip reduce_slabs_kernel / reduce_slabs_t_kernel, with the LSTM gate un-permutation) and
the tiled transpose -- against fp64 products and bit-exact fp32 host loops.

Every weight gradient of the direction net goes through these kernels (nppc_audio/engine.py _wgrad, _lstm_wgrad and the TCN
backward).  The reductions add the S slabs in index order in fp32 from 0, so a host loop `acc = acc + slab[k]` in fp32
reproduces them bit for bit: they are compared with torch.equal.  Every destination starts as a sentinel, and whatever lies
outside the written window must keep it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
NAN = float("nan")
U32 = 2.0 ** -24
SENT = -12345.0
EPI_PLAIN_F32 = 4


def bound_ratio(got, ref, bound):
    d = (got.double().cpu() - ref).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / bound).max())


# ---------------------------------------------------------------------------------------------------------------- TN GEMM
# launch_tn (default switches) for C_slab[b][s] = A[b][rows of slice s]^T B[b][rows of slice s], batch 3:
#   "dma192"  gemm_tn_dma_kernel<192, 32, 5>: M % 256 == 0, N % 192 == 0, (M/256)(N/192) ksplit batch >= 256
#             M = 512, N = 384, ksplit = 24: 2 * 2 * 24 * 3 = 288 workgroups (blockIdx.z = 72: the XCD remap is on)
#   "dma128"  gemm_tn_dma_kernel<128, 64, 3>: N % 128 == 0 (and N % 192 != 0), (M/256)(N/128) ksplit batch >= 256
#             M = 512, N = 256, ksplit = 22: 2 * 2 * 22 * 3 = 264 workgroups
#   "tiled128" gemm_tn_tiled_kernel<128>: N % 128 == 0 but M % 256 != 0 (no LDS-DMA, no 256-row tiles)
#             M = 384, N = 256, ksplit = 3
#   "tiled64" gemm_tn_tiled_kernel<64>: N % 128 != 0 -- N = 320, the C = 257 TCN weight gradient (M = 512 hidden channels)
#             M = 512, N = 320, ksplit = 8 (blockIdx.z = 24: XCD remap on)
TN_CASES = [pytest.param(512, 384, 128, 24, id="dma192-M512-N384"), pytest.param(512, 256, 128, 22, id="dma128-M512-N256"),
            pytest.param(384, 256, 128, 3, id="tiled128-M384-N256"), pytest.param(512, 320, 128, 8, id="tiled64-M512-N320"),
            pytest.param(128, 64, 64, 5, id="tiled64-M128-N64")]


@pytest.mark.parametrize("M,N,Rz,ksplit", TN_CASES)
def test_tn_splitk_batched_matches_fp64(M, N, Rz, ksplit, record_err):
    from nppc_audio import _hip as H
    nb = 3
    Rr = Rz * ksplit
    lda, ldb, ldc = M + 8, N + 24, N + 16
    sA, sB = Rr * lda + 64, Rr * ldb + 40                       # not the dense strides
    sC = ksplit * M * ldc + 136                                  # a sentinel gap after each batch entry's slabs
    g = torch.Generator().manual_seed(M + N + ksplit)
    a = torch.randn(nb, Rr, M, generator=g).bfloat16().double() * torch.tensor([1.0, 0.25, 4.0]).view(nb, 1, 1)
    b = torch.randn(nb, Rr, N, generator=g).bfloat16().double()
    A = torch.full((nb * sA,), NAN, dtype=torch.bfloat16)
    B = torch.full((nb * sB,), NAN, dtype=torch.bfloat16)
    for i in range(nb):
        A[i * sA: i * sA + Rr * lda].view(Rr, lda)[:, :M] = a[i].bfloat16()
        B[i * sB: i * sB + Rr * ldb].view(Rr, ldb)[:, :N] = b[i].bfloat16()
    C = torch.full((nb * sC,), SENT, device="cuda")
    H.call("nppc_gemm_tn_splitk_batched", A.cuda(), lda, sA, B.cuda(), ldb, sB, C, ldc, sC, M, N, Rr, ksplit, nb, H.stream())
    torch.cuda.synchronize()
    C = C.cpu()
    worst = 0.0
    for i in range(nb):
        blk = C[i * sC: (i + 1) * sC]
        assert bool((blk[ksplit * M * ldc:] == SENT).all())                 # the gap behind the slabs is untouched
        slabs = blk[:ksplit * M * ldc].view(ksplit, M, ldc)
        assert bool((slabs[:, :, N:] == SENT).all())                         # ld columns past N untouched
        ai, bi = a[i].view(ksplit, Rz, M), b[i].view(ksplit, Rz, N)
        ref = torch.bmm(ai.transpose(1, 2), bi)
        mag = torch.bmm(ai.abs().transpose(1, 2), bi.abs())
        # bf16 products are exact in fp32: the error is the fp32 accumulation of Rz terms and the fp32 result itself
        worst = max(worst, bound_ratio(slabs[:, :, :N], ref, 2 * math.sqrt(Rz) * U32 * mag + U32 * ref.abs()))
    record_err("slabs", worst, 1.0)


def test_tn_splitk_batched_rejects_an_empty_batch():
    from nppc_audio import _hip as H
    A = torch.zeros(128, 128, dtype=torch.bfloat16, device="cuda")
    C = torch.zeros(128, 128, device="cuda")
    for nb in (0, -1):
        with pytest.raises(RuntimeError, match="bad argument"):
            H.call("nppc_gemm_tn_splitk_batched", A, 128, 0, A, 128, 0, C, 128, 0, 128, 128, 128, 1, nb, H.stream())


# ---------------------------------------------------------------------------------------------------------------- reductions
def _slab_values(shape, g):
    """fp32 values over many binades, both signs: the order of the fp32 additions shows in the result"""
    return (torch.randn(*shape, generator=g) * torch.pow(10.0, torch.randint(-3, 4, shape, generator=g).float())).float()


def _host_sum(slabs):
    """fp32 sum in slab order starting from 0, like the kernels"""
    acc = torch.zeros_like(slabs[0])
    for k in range(slabs.shape[0]):
        acc = acc + slabs[k]
    return acc


def _lstm_pack(gt, Hd):
    """nn.LSTM weight layout [4 Hd][n] (gate blocks i, f, g, o) -> the packed layout the LSTM kernels produce: row u * 4 + g'
    with g' in the order i, g, f, o"""
    i, f, gg, o = gt[0:Hd], gt[Hd:2 * Hd], gt[2 * Hd:3 * Hd], gt[3 * Hd:4 * Hd]
    return torch.stack([i, gg, f, o], dim=1).reshape(4 * Hd, -1)


# (S, rows, ld, col0, ncols, permH, accumulate, batch)
RS_CASES = [(1, 37, 70, 0, 70, 0, 0, 1), (3, 50, 100, 13, 45, 0, 1, 3), (64, 33, 64, 7, 50, 0, 0, 2), (3, 4 * 29, 81, 5, 61, 29, 1, 3),
            (64, 4 * 40, 97, 0, 97, 40, 0, 1), (1, 4 * 7, 40, 33, 7, 7, 1, 2), (64, 4 * 13, 1, 0, 1, 13, 1, 3)]


@pytest.mark.parametrize("S,rows,ld,col0,ncols,permH,accumulate,nb", RS_CASES)
def test_reduce_slabs_bit_exact(S, rows, ld, col0, ncols, permH, accumulate, nb):
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(S + rows + ld + col0)
    slab_stride = rows * ld + 3
    sSlab = S * slab_stride + 11
    dst_ld = ncols + 5
    sDst = rows * dst_ld + 9
    slabs = torch.full((nb * sSlab,), NAN)
    want_rows = []                                    # per batch entry: [rows][ncols] in the destination's (torch) row order
    for i in range(nb):
        if permH:
            # gradients in nn.LSTM layout, packed the way the kernels leave them in the slabs
            gt = _slab_values((S, rows, ncols), g)
            for k in range(S):
                v = slabs[i * sSlab + k * slab_stride: i * sSlab + k * slab_stride + rows * ld].view(rows, ld)
                v[:, col0:col0 + ncols] = _lstm_pack(gt[k], permH)
            want_rows.append(_host_sum(gt))
        else:
            sv = _slab_values((S, rows, ncols), g)
            for k in range(S):
                v = slabs[i * sSlab + k * slab_stride: i * sSlab + k * slab_stride + rows * ld].view(rows, ld)
                v[:, col0:col0 + ncols] = sv[k]
            want_rows.append(_host_sum(sv))
    dst0 = torch.full((nb * sDst,), SENT)
    init = _slab_values((nb, rows, ncols), g)
    for i in range(nb):
        dst0[i * sDst: i * sDst + rows * dst_ld].view(rows, dst_ld)[:, :ncols] = init[i]
    dst = dst0.cuda()
    H.call("nppc_reduce_slabs", slabs.cuda(), S, slab_stride, ld, dst, dst_ld, rows, col0, ncols, permH, accumulate, sSlab, sDst, nb,
           H.stream())
    torch.cuda.synchronize()
    dst = dst.cpu()
    want = dst0.clone()
    for i in range(nb):
        w = want[i * sDst: i * sDst + rows * dst_ld].view(rows, dst_ld)
        w[:, :ncols] = (init[i] + want_rows[i]) if accumulate else want_rows[i]
    assert torch.equal(dst, want)                     # the window bit for bit, the sentinel everywhere else


# (S, rows, ncols, ld, batch): dst[b][r][c] = sum_s slab[b][s][c][r]
RST_CASES = [(1, 37, 45, 40, 1), (3, 100, 33, 128, 3), (64, 29, 70, 29, 2), (3, 257, 64, 320, 3)]


@pytest.mark.parametrize("S,rows,ncols,ld,nb", RST_CASES)
def test_reduce_slabs_t_bit_exact(S, rows, ncols, ld, nb):
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(S + rows + ncols)
    slab_stride = ncols * ld + 5
    sSlab = S * slab_stride + 13
    dst_ld = ncols + 3
    sDst = rows * dst_ld + 7
    slabs = torch.full((nb * sSlab,), NAN)
    sums = []
    for i in range(nb):
        sv = _slab_values((S, ncols, rows), g)
        for k in range(S):
            slabs[i * sSlab + k * slab_stride: i * sSlab + k * slab_stride + ncols * ld].view(ncols, ld)[:, :rows] = sv[k]
        sums.append(_host_sum(sv))
    dst = torch.full((nb * sDst,), SENT, device="cuda")
    H.call("nppc_reduce_slabs_t", slabs.cuda(), S, slab_stride, ld, dst, dst_ld, rows, ncols, sSlab, sDst, nb, H.stream())
    torch.cuda.synchronize()
    want = torch.full((nb * sDst,), SENT)
    for i in range(nb):
        want[i * sDst: i * sDst + rows * dst_ld].view(rows, dst_ld)[:, :ncols] = sums[i].T
    assert torch.equal(dst.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,cols,nb", [(37, 45, 3), (64, 33, 1), (130, 257, 3), (1, 70, 2)])
def test_transpose_bit_exact(prec, relu, rows, cols, nb):
    from nppc_audio import _hip as H
    dt = H.dtype_of(prec)
    g = torch.Generator().manual_seed(rows + cols + relu + prec)
    ld_in, ld_out = cols + 7, rows + 5
    sIn, sOut = rows * ld_in + 3, cols * ld_out + 6
    x = torch.randn(nb, rows, cols, generator=g).to(dt)
    inp = torch.full((nb * sIn,), NAN, dtype=dt)                 # NaN in the ld padding and the batch gaps: never read
    for i in range(nb):
        inp[i * sIn: i * sIn + rows * ld_in].view(rows, ld_in)[:, :cols] = x[i]
    out = torch.full((nb * sOut,), SENT, dtype=dt, device="cuda")
    H.call("nppc_transpose", prec, inp.cuda(), out, rows, cols, ld_in, ld_out, sIn, sOut, relu, nb, H.stream())
    torch.cuda.synchronize()
    want = torch.full((nb * sOut,), SENT, dtype=dt)
    for i in range(nb):
        want[i * sOut: i * sOut + cols * ld_out].view(cols, ld_out)[:, :rows] = x[i].T.clamp_min(0) if relu else x[i].T
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- _wgrad fallback
@pytest.mark.parametrize("prec,S", [(0, 4), (1, 2), (0, 1)])
def test_wgrad_fallback_split_k_then_reduce(prec, S, record_err):
    """engine.py _wgrad when nppc_gemm_nt_splitk does not apply (batch 3, ncolsN = 320 not a multiple of 128): nppc_gemm_nt
    epi 4 writes S fp32 slabs per branch, nppc_reduce_slabs adds them into dst[r][c] = sum_k AT[r][k] BT[c][k], c < ncols"""
    from nppc_audio import _hip as H
    nb, rows, ncolsN, ncols, K = 3, 256, 320, 257, 512
    dt = H.dtype_of(prec)
    g = torch.Generator().manual_seed(S + prec)
    lda, ldb = K + 8, K + 16
    sA, sB = rows * lda + 24, ncolsN * ldb + 8
    at = torch.randn(nb, rows, K, generator=g).to(dt).double()
    bt = torch.randn(nb, ncolsN, K, generator=g).to(dt).double()
    A = torch.full((nb * sA,), NAN, dtype=dt)
    B = torch.full((nb * sB,), NAN, dtype=dt)
    for i in range(nb):
        A[i * sA: i * sA + rows * lda].view(rows, lda)[:, :K] = at[i].to(dt)
        B[i * sB: i * sB + ncolsN * ldb].view(ncolsN, ldb)[:, :K] = bt[i].to(dt)
    slab = torch.full((nb * S * rows * ncolsN,), NAN, device="cuda")
    dst_ld, sDst = ncols + 11, rows * (ncols + 11) + 5
    dst = torch.full((nb * sDst,), SENT, device="cuda")
    s = H.stream()
    H.call("nppc_gemm_nt", prec, EPI_PLAIN_F32, A.cuda(), lda, sA, B.cuda(), ldb, sB, slab, ncolsN, rows * ncolsN, None, 0, None, 0,
           0, None, 0, None, 0, rows, ncolsN, K, rows, rows, ncolsN, 0, nb, S, s)
    H.call("nppc_reduce_slabs", slab, S, rows * ncolsN, ncolsN, dst, dst_ld, rows, 0, ncols, 0, 0, S * rows * ncolsN, sDst, nb, s)
    torch.cuda.synchronize()
    dst = dst.cpu()
    worst = 0.0
    for i in range(nb):
        d = dst[i * sDst: (i + 1) * sDst]
        assert bool((d[rows * dst_ld:] == SENT).all())
        d = d[:rows * dst_ld].view(rows, dst_ld)
        assert bool((d[:, ncols:] == SENT).all())
        ref = at[i] @ bt[i, :ncols].T
        mag = at[i].abs() @ bt[i, :ncols].abs().T
        # S slices of K/S terms accumulated in fp32, S rounded slab values added in fp32
        worst = max(worst, bound_ratio(d[:, :ncols], ref, 2 * math.sqrt(K / S) * U32 * mag + (S + 1) * U32 * mag))
    record_err("dst", worst, 1.0)

