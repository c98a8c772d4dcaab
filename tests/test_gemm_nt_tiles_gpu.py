"""GPU: the bf16 tiles of gemm_nt_lds_kernel (csrc/tcn.hip) -- 64 and 128 columns wide on the single-stage-image main loop
(nt_lds_mainloop_1buf, csrc/mfma_tile.h) with the multi-pass coalesced epilogue -- through nppc_gemm_nt, nppc_gemm_nt_gn and
nppc_gemm_nt_colsum, against fp64 evaluations of the same formulas: inputs rounded to bf16 first, the output compared as stored.

Shapes, the smallest at which this code can go wrong:
  R  128, 256 at Tp = 128, Tv = 125 (one / two row tiles; three padding rows per sample, which must come out zero);
  K  64, 128, 320: one stage (the image is never rewritten), two (rewritten once), five;
  N  64, 128 (one tile of each width), 192 and 576 with Nv = 514 (three / nine 64-wide tiles; the masked padding columns begin
     inside the last tile);
  batch 2 at batch strides that differ from the dense ones, leading dimensions with padding (multiples of 8: the coalesced
  epilogue), NaN wherever the kernel must not read or must mask by selection.

The limits are those of tests/test_tcn_forward_gpu.py (element-wise bound from the formats, statistics) and tests/test_tcn_gpu.py
(column sums, folded GroupNorm) for the same entry points."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
NAN = float("nan")
U32 = 2.0 ** -24
UBF = 2.0 ** -8
EPI_PLAIN, EPI_PRELU_STATS, EPI_RESIDUAL, EPI_RELU, EPI_PLAIN_F32, EPI_MASK_POS = 0, 1, 2, 3, 4, 5
Z, TP, TV = 2, 128, 125
DT = torch.bfloat16

N_CASES = ((64, 61), (128, 127), (192, 190), (576, 514))
SHAPES = [pytest.param(N, Nv, K, id=f"N{N}-K{K}") for N, Nv in N_CASES for K in (64, 128, 320)]
ROWS = (128, 256)


def bound_ratio(got, ref, bound):
    d = (got.double() - ref).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / bound).max())


def strided(rows, ld, stride, vals):
    """[Z][rows][ld] at batch stride `stride` in a NaN buffer, vals [Z][rows][cols] in the leading columns"""
    buf = torch.full((Z * stride,), NAN, dtype=vals.dtype)
    for z in range(Z):
        buf[z * stride: z * stride + rows * ld].view(rows, ld)[:, :vals.shape[2]] = vals[z]
    return buf.cuda()


def flat(vals, stride):
    buf = torch.full((Z * stride,), NAN, dtype=vals.dtype)
    for z in range(Z):
        buf[z * stride: z * stride + vals.shape[1]] = vals[z]
    return buf.cuda()


class Problem:
    """operands of one batched product (bf16 values held in fp64), built once per shape and left unchanged"""

    def __init__(self, N, Nv, K, R):
        g = torch.Generator().manual_seed(7 * N + 3 * K + R)
        self.N, self.Nv, self.K, self.R, self.B = N, Nv, K, R, R // TP
        self.lda, self.ldb, self.ldc, self.ldres = K + 8, K + 16, N + 8, N + 16
        self.sA, self.sB, self.sC, self.sRes = R * self.lda + 40, N * self.ldb + 24, R * self.ldc + 16, R * self.ldres + 32
        self.sBias, self.sSlope, self.sStats = N + 40, 5, 2 * self.B + 3
        self.valid_row = (torch.arange(R) % TP) < TV
        scale = torch.tensor([1.0, 3.0][:self.B]).repeat_interleave(TP)[:, None]     # a sample-index error shows in the statistics
        a = (torch.randn(Z, R, K, generator=g) * scale).to(DT)
        a[:, ~self.valid_row] = NAN
        w = (torch.randn(Z, N, K, generator=g) / math.sqrt(K)).to(DT)
        w[:, Nv:] = NAN
        self.a, self.w = a, w
        self.bias = torch.randn(Z, N, generator=g) * 0.3
        self.bias[:, Nv:] = NAN
        self.slope = torch.tensor([[0.25], [-0.3]])
        self.res = torch.randn(Z, R, N, generator=g).to(DT)
        pick = torch.rand(Z, R, N, generator=g)
        m = self.res.clone()                                  # mask operand: exact zeros, -0, NaN and negatives among the positives
        m[pick < 0.1] = 0.0
        m[(pick >= 0.1) & (pick < 0.15)] = NAN
        m[(pick >= 0.15) & (pick < 0.2)] = -0.0
        self.mask = m
        self.gn_v = torch.randn(Z, N, generator=g) * 0.5
        self.gn_stats = torch.tensor([[[40.0 + 9 * b + z, 900.0 + 50 * b] for b in range(self.B)] for z in range(Z)], dtype=torch.float64)
        self.gn_cnt = float(K * TV)
        self.A, self.W = strided(R, self.lda, self.sA, a), strided(N, self.ldb, self.sB, w)
        a0 = torch.nan_to_num(a.double(), nan=0.0)
        self.a0, self.w0 = a0, torch.nan_to_num(w.double(), nan=0.0)

    def product(self, relu_in=False, k0=0, k1=None):
        """(fp64 product, magnitude of its terms) over the K columns [k0, k1)"""
        a = self.a0[:, :, k0:k1]
        if relu_in:
            a = a.clamp_min(0.0)
        w = self.w0[:, :, k0:k1]
        return a @ w.transpose(1, 2), a.abs() @ w.abs().transpose(1, 2)

    def masked(self, v):
        v = v.clone()
        v[:, ~self.valid_row] = 0.0
        v[:, :, self.Nv:] = 0.0
        return v

    def out_buffer(self, dtype=DT, slabs=Z):
        return torch.full((slabs * self.sC,), NAN, dtype=dtype, device="cuda")

    def out(self, C, slabs=Z):
        return torch.stack([C[s * self.sC: s * self.sC + self.R * self.ldc].view(self.R, self.ldc) for s in range(slabs)]).cpu()

    def check_padding(self, o):
        """padding rows and columns exactly 0, nothing NaN inside [R][N], the ld columns past N untouched"""
        assert not bool(torch.isnan(o[:, :, :self.N].float()).any())
        assert not bool(o[:, ~self.valid_row, :self.N].float().any())
        assert not bool(o[:, :, self.Nv:self.N].float().any())
        assert bool(torch.isnan(o[:, :, self.N:].float()).all())

    def gemm_nt(self, epi, C, bias=None, res=None, slope=None, stats=None, relu_in=0, ksplit=1, colpart=None):
        from nppc_audio import _hip as H
        if colpart is not None:
            H.call("nppc_gemm_nt_colsum", 0, epi, self.A, self.lda, self.sA, self.W, self.ldb, self.sB, C, self.ldc, self.sC, bias,
                   self.sBias, res, self.ldres, self.sRes, self.R, self.N, self.K, TP, TV, self.Nv, Z, colpart, H.stream())
        else:
            H.call("nppc_gemm_nt", 0, epi, self.A, self.lda, self.sA, self.W, self.ldb, self.sB, C, self.ldc, self.sC, bias,
                   self.sBias, res, self.ldres, self.sRes, slope, self.sSlope, stats, self.sStats, self.R, self.N, self.K, TP, TV,
                   self.Nv, relu_in, Z, ksplit, H.stream())
        torch.cuda.synchronize()

    def elem_bound(self, ref, mag, uo=UBF):
        return uo * ref.abs() + 2 * math.sqrt(self.K) * U32 * mag + 4 * U32 * ref.abs()


@functools.lru_cache(maxsize=None)
def problem(N, Nv, K, R):
    return Problem(N, Nv, K, R)


def tile_width(N, K, ksplit=1, prec=0):
    from nppc_audio import _hip as H
    bn = ctypes.c_int(-1)
    H.call("nppc_gemm_nt_tile", prec, N, K, ksplit, ctypes.byref(bn))
    return bn.value


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_plain(N, Nv, K, R, record_err):
    p = problem(N, Nv, K, R)
    C = p.out_buffer()
    p.gemm_nt(EPI_PLAIN, C, bias=flat(p.bias, p.sBias))
    o = p.out(C)
    p.check_padding(o)
    v, mag = p.product()
    b = torch.nan_to_num(p.bias.double(), nan=0.0)[:, None, :]
    ref = p.masked(v + b)
    record_err("C", bound_ratio(o[:, :, :N], ref, p.elem_bound(ref, mag + b.abs())), 1.0)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_prelu_and_groupnorm_statistics(N, Nv, K, R, record_err):
    p = problem(N, Nv, K, R)
    C = p.out_buffer()
    prefill = torch.tensor([[[2.5 + b, 1.25 + 0.75 * b] for b in range(p.B)]] * Z, dtype=torch.float64)
    st = torch.full((Z * p.sStats,), NAN, dtype=torch.float64)
    for z in range(Z):
        st[z * p.sStats: z * p.sStats + 2 * p.B] = prefill[z].reshape(-1)
    st = st.cuda()
    p.gemm_nt(EPI_PRELU_STATS, C, bias=flat(p.bias, p.sBias), slope=flat(p.slope, p.sSlope), stats=st)
    o = p.out(C)
    p.check_padding(o)
    v, mag = p.product()
    b = torch.nan_to_num(p.bias.double(), nan=0.0)[:, None, :]
    s = p.slope.double()[:, :, None]
    v = v + b
    ref = p.masked(torch.where(v > 0, v, s * v))
    mag = (mag + b.abs()) * torch.maximum(s.abs(), torch.ones_like(s))
    record_err("C", bound_ratio(o[:, :, :N], ref, p.elem_bound(ref, mag)), 1.0)
    # (sum, sumsq) per sample against fp64 sums of the STORED values: a lane adds n_lane = 16 rows x BN / 32 columns of them in
    # fp32 (error <= (n_lane + 1) 2^-24 of the sum of magnitudes), the rest is fp64
    n_lane = 16 * tile_width(N, K) // 32
    vals = o[:, :, :N].double().view(Z, p.B, TP, N)[:, :, :TV].reshape(Z, p.B, -1)
    st = st.cpu()
    got = torch.stack([st[z * p.sStats: z * p.sStats + 2 * p.B].view(p.B, 2) for z in range(Z)])
    s1, s2, m1 = vals.sum(-1), (vals * vals).sum(-1), vals.abs().sum(-1)
    e1 = (got[..., 0] - prefill[..., 0] - s1).abs() / (m1 + 1e-300)
    e2 = (got[..., 1] - prefill[..., 1] - s2).abs() / (s2 + 1e-300)
    record_err("stats", float(torch.maximum(e1, e2).max()) / ((n_lane + 1) * U32), 1.0)
    for z in range(Z):                         # the gap past the samples of a batch entry is untouched
        assert bool(torch.isnan(st[z * p.sStats + 2 * p.B: (z + 1) * p.sStats]).all())


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_residual_with_tile_column_sums(N, Nv, K, R, record_err):
    p = problem(N, Nv, K, R)
    r = p.res.clone()
    r[:, ~p.valid_row] = NAN
    r[:, :, Nv:] = NAN
    res = strided(R, p.ldres, p.sRes, r)
    C, C1 = p.out_buffer(), p.out_buffer()
    cp = torch.full((Z, R // 128, N), NAN, device="cuda")
    p.gemm_nt(EPI_RESIDUAL, C, bias=flat(p.bias, p.sBias), res=res)
    p.gemm_nt(EPI_RESIDUAL, C1, bias=flat(p.bias, p.sBias), res=res, colpart=cp)
    o = p.out(C)
    p.check_padding(o)
    assert torch.equal(o[:, :, :N], p.out(C1)[:, :, :N])
    v, mag = p.product()
    b = torch.nan_to_num(p.bias.double(), nan=0.0)[:, None, :]
    r0 = torch.nan_to_num(r.double(), nan=0.0)
    ref = p.masked(v + b + r0)
    record_err("C", bound_ratio(o[:, :, :N], ref, p.elem_bound(ref, mag + b.abs() + r0.abs())), 1.0)
    want = o[:, :, :N].double().view(Z, R // 128, 128, N).sum(2)
    assert bool(torch.isfinite(cp).all())
    record_err("colsum", float((cp.double().cpu() - want).abs().max()), 1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_mask_pos_with_tile_column_sums(N, Nv, K, R, record_err):
    p = problem(N, Nv, K, R)
    res = strided(R, p.ldres, p.sRes, p.mask)
    C = p.out_buffer()
    cp = torch.full((Z, R // 128, N), NAN, device="cuda")
    p.gemm_nt(EPI_MASK_POS, C, res=res, colpart=cp)
    o = p.out(C)
    p.check_padding(o)
    v, mag = p.product()
    keep = p.mask.double() > 0                          # NaN > 0 is False: masked, like the kernel's !(res > 0)
    ref = p.masked(torch.where(keep, v, torch.zeros_like(v)))
    record_err("C", bound_ratio(o[:, :, :N], ref, p.elem_bound(ref, mag)), 1.0)
    assert float(o[:, :, :N][~keep].float().abs().max()) == 0.0       # masked by selection: exact zeros
    want = o[:, :, :N].double().view(Z, R // 128, 128, N).sum(2)      # each 128-row tile's column sums of the stored output
    assert bool(torch.isfinite(cp).all())
    record_err("colsum", float((cp.double().cpu() - want).abs().max()), 1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_relu_of_relu_input(N, Nv, K, R, record_err):
    p = problem(N, Nv, K, R)
    C = p.out_buffer()
    p.gemm_nt(EPI_RELU, C, bias=flat(p.bias, p.sBias), relu_in=1)
    o = p.out(C)
    p.check_padding(o)
    v, mag = p.product(relu_in=True)
    b = torch.nan_to_num(p.bias.double(), nan=0.0)[:, None, :]
    ref = p.masked((v + b).clamp_min(0.0))
    record_err("C", bound_ratio(o[:, :, :N], ref, p.elem_bound(ref, mag + b.abs())), 1.0)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_fp32_slabs_of_a_split_k(N, Nv, K, R, record_err):
    """ksplit = 2: K slices of 64 (one stage of the LDS kernels), 32 and 160 (no whole stage: the register-staged kernel); slab
    z * 2 + s holds the product over K columns [s K / 2, (s + 1) K / 2), masked like every epilogue"""
    p = problem(N, Nv, K, R)
    Ks = K // 2
    C = p.out_buffer(torch.float32, 2 * Z)
    p.gemm_nt(EPI_PLAIN_F32, C, ksplit=2)
    o = p.out(C, 2 * Z).view(Z, 2, R, p.ldc)
    worst = 0.0
    for s in range(2):
        p.check_padding(o[:, s])
        v, mag = p.product(k0=s * Ks, k1=(s + 1) * Ks)
        ref = p.masked(v)
        worst = max(worst, bound_ratio(o[:, s, :, :N], ref, U32 * ref.abs() + 2 * math.sqrt(Ks) * U32 * mag))
    record_err("slab", worst, 1.0)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("N,Nv,K", SHAPES)
def test_residual_with_folded_groupnorm(N, Nv, K, R, record_err):
    """nppc_gemm_nt_gn: C = rstd_b (A Wg^T) - mean_b rstd_b v + u + res, mean_b and rstd_b from the (sum, sumsq) of sample b"""
    from nppc_audio import _hip as H
    p = problem(N, Nv, K, R)
    eps = 1e-8
    r = p.res.clone()
    r[:, ~p.valid_row] = NAN
    r[:, :, Nv:] = NAN
    res = strided(R, p.ldres, p.sRes, r)
    u, gv = p.bias.clone(), p.gn_v.clone()
    gv[:, Nv:] = NAN
    st = torch.full((Z * p.sStats,), NAN, dtype=torch.float64)
    for z in range(Z):
        st[z * p.sStats: z * p.sStats + 2 * p.B] = p.gn_stats[z].reshape(-1)
    C = p.out_buffer()
    H.call("nppc_gemm_nt_gn", 0, p.A, p.lda, p.sA, p.W, p.ldb, p.sB, C, p.ldc, p.sC, flat(u, p.sBias), flat(gv, p.sBias), p.sBias,
           res, p.ldres, p.sRes, st.cuda(), p.sStats, p.gn_cnt, eps, R, N, K, TP, TV, Nv, Z, H.stream())
    torch.cuda.synchronize()
    o = p.out(C)
    p.check_padding(o)
    v, _ = p.product()
    mean = (p.gn_stats[..., 0] / p.gn_cnt)
    rstd = 1.0 / torch.sqrt(p.gn_stats[..., 1] / p.gn_cnt - mean * mean + eps)
    mean_r, rstd_r = (x.repeat_interleave(TP, dim=1)[:, :, None] for x in (mean, rstd))       # per row
    u0, v0 = (torch.nan_to_num(x.double(), nan=0.0)[:, None, :] for x in (u, gv))
    ref = p.masked(rstd_r * v - mean_r * rstd_r * v0 + u0 + torch.nan_to_num(r.double(), nan=0.0))
    record_err("C", float((o[:, :, :N].double() - ref).abs().max()), 3e-2 * float(ref.abs().max()))


def test_tile_width_per_shape():
    """the dispatch of nppc_gemm_nt / _colsum / _gn: 128 columns where they divide N (N = 512), 64 for the rest (the direction
    net's N = 576 -- a 192-wide tile measured slower -- and the restorer's N = 320); a K slice that is no whole stage goes to
    the register-staged kernel"""
    assert [tile_width(N, K) for N, K in ((512, 576), (512, 320), (576, 512), (576, 320), (320, 512), (320, 576))] == [128, 128, 64, 64, 64, 64]
    assert [tile_width(N, 64) for N in (64, 128, 192, 576)] == [64, 128, 64, 64]
    assert tile_width(576, 320, ksplit=2) == 0 and tile_width(576, 128, ksplit=2) == 64
    assert tile_width(576, 512, prec=1) == 64 and tile_width(512, 512, prec=1) == 128 and tile_width(512, 96) == 0
