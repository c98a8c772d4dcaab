"""GPU: the full-band TCN forward kernels, one by one, against fp64 references.

nppc_gemm_nt (csrc/tcn.hip launch_nt) with every epilogue -- 0 plain, 1 bias + PReLU + per-sample GroupNorm (sum, sumsq),
2 residual, 3 ReLU, 4 fp32 split-K slabs, 5 mask by (res > 0) -- on each kernel and epilogue layout it dispatches to;
nppc_tcn_dwconv (GroupNorm-1 apply + depthwise dilated k = 3 conv + PReLU-2 + GroupNorm-2 statistics); and one whole
TCNBlock plus the trailing ReLU -> Linear -> ReLU, chained the way nppc_audio/engine.py runs them, against oracle.nppc_ref.

Every reference is built in fp64 from the values the kernel reads (bf16-rounded where the kernel reads bf16).  The limits
are element-wise error bounds derived from the formats:
  u_out  = 2^-8 (bf16: 8-bit significand, round to nearest) or 2^-24 (fp32): rounding of the stored output, relative to it;
  accumulation of K products in fp32: 2 sqrt(K) 2^-24 times sum_k |a_k b_k| (the magnitude of the terms).
record_err gets max(|got - ref| / bound) with the limit 1.

Padding is NaN wherever the kernel must not read it or must mask it by selection: A rows with (row % Tp) >= Tv, weight rows
>= Nv, the ld columns past K / C, bias and slope entries between the branches' strides, frames >= Tv of the depthwise input."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import nppc_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
U32 = 2.0 ** -24
EPS = 1e-8
EPI_PLAIN, EPI_PRELU_STATS, EPI_RESIDUAL, EPI_RELU, EPI_PLAIN_F32, EPI_MASK_POS = 0, 1, 2, 3, 4, 5


def u_out(prec):
    return 2.0 ** -8 if prec == 0 else U32


def bound_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 where both are equal)"""
    d = (got.double().cpu() - ref).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / bound).max()) if d.numel() else 0.0


def stats_ratio(got, prefill, vals, n_lane):
    """the kernel's (sum, sumsq) per sample, added to `prefill`, against fp64 sums of the stored values `vals` [..., n]: each
    lane adds n_lane terms in fp32 (error <= (n_lane + 1) 2^-24 of the sum of magnitudes), the rest is fp64"""
    s1, s2 = vals.sum(-1), (vals * vals).sum(-1)
    m1, m2 = vals.abs().sum(-1), (vals * vals).sum(-1)
    e1 = (got[..., 0].double().cpu() - prefill[..., 0] - s1).abs() / (m1 + 1e-300)
    e2 = (got[..., 1].double().cpu() - prefill[..., 1] - s2).abs() / (m2 + 1e-300)
    return float(torch.maximum(e1, e2).max()) / ((n_lane + 1) * U32)


# ---------------------------------------------------------------------------------------------------------------- nppc_gemm_nt
# Kernel dispatch in launch_nt (bk = 64 bf16 / 32 fp32):
#   "reg"    gemm_nt_kernel, register-staged:        (K / ksplit) % bk != 0   -> bf16 with K % 64 == 32 (K = 96, 160)
#   "lds64"  gemm_nt_lds_kernel<.., 64>:             (K / ksplit) % bk == 0 and N % 128 != 0   (N = 320, the C = 257 ldC)
#   "lds128" gemm_nt_lds_kernel<.., 128>:            (K / ksplit) % bk == 0 and N % 128 == 0   (N = 256)
# Epilogue layout:
#   "staged" coalesced through LDS: LDS kernels only; epi 2 / 5 when ldc % 8 == 0 and ldres % 8 == 0 (both precisions);
#            epi 0 / 1 / 3 when ldc % 8 == 0, bf16, no split K (NPPC_NT_STAGED_PLAIN on, the default)
#   "acc"    accumulator layout: everything else -- here reached by ldc % 8 != 0 (and ldres % 8 != 0)
KERNEL_SHAPE = {"reg": (320, 160), "lds64": (320, 128), "lds128": (256, 192)}     # (N, K)
NV_SMALL = {320: 257, 256: 193}


def _nt_cases():
    cases = []
    for prec in (0, 1):
        for epi in (EPI_PLAIN, EPI_PRELU_STATS, EPI_RESIDUAL, EPI_RELU, EPI_PLAIN_F32, EPI_MASK_POS):
            for kern in ("reg", "lds64", "lds128"):
                if kern == "reg" and prec == 1:
                    continue                          # fp32 K % 32 == 0 is always a whole LDS stage
                for lay in ("staged", "acc"):
                    if lay == "staged" and (kern == "reg" or epi == EPI_PLAIN_F32 or
                                            (prec == 1 and epi in (EPI_PLAIN, EPI_PRELU_STATS, EPI_RELU))):
                        continue                      # no staged epilogue on these
                    cases.append(pytest.param(prec, epi, kern, lay, id=f"{'bf16' if prec == 0 else 'fp32'}-epi{epi}-{kern}-{lay}"))
    return cases


TV_CASES = [pytest.param(Tv, Tp, id=f"Tv{Tv}-Tp{Tp}") for Tv, Tp in ((1, 128), (37, 128), (127, 128), (128, 128), (129, 256),
                                                                     (200, 256))]


class _NT:
    """one batched nppc_gemm_nt problem with strided, NaN-padded operands (Z = 3 branches, B = 3 samples at Tp = 128, else 2)"""
    Z = 3

    def __init__(self, prec, epi, N, K, Nv, Tv, Tp, lay, relu_in, ksplit, seed):
        from nppc_audio import _hip as H
        Z = self.Z
        B = self.B = 3 if Tp == 128 else 2
        self.prec, self.epi, self.N, self.K, self.Nv, self.Tv, self.Tp = prec, epi, N, K, Nv, Tv, Tp
        self.relu_in, self.ksplit = relu_in, ksplit
        self.R = R_ = B * Tp
        dt = self.dt = H.dtype_of(prec)
        g = torch.Generator().manual_seed(seed)
        self.lda, self.ldb = K + 8, K + 16
        self.ldc = N + (8 if lay == "staged" else 3)
        self.ldres = N + (16 if lay == "staged" else 5)
        self.sA, self.sB = R_ * self.lda + 40, N * self.ldb + 24        # batch strides differ from the dense ones
        self.sC = R_ * self.ldc + (16 if lay == "staged" else 7)
        self.sRes = R_ * self.ldres + 32
        self.sBias, self.sSlope, self.sStats = N + 40, 5, 2 * B + 3
        valid_row = (torch.arange(R_) % Tp) < Tv
        self.valid_row = valid_row
        # A: per-sample scales that differ (a sample-index error in the statistics shows), NaN in the padding rows
        scale = torch.tensor([1.0, 3.0, 0.5][:B]).repeat_interleave(Tp)[:, None]
        a = (torch.randn(Z, R_, K, generator=g) * scale).to(dt).double()
        a[:, ~valid_row] = NAN
        self.a = a
        w = (torch.randn(Z, N, K, generator=g) / math.sqrt(K)).to(dt).double()
        w[:, Nv:] = NAN
        self.w = w
        self.A = self._strided((Z, R_, self.lda), self.sA, a, dt)
        self.W = self._strided((Z, N, self.ldb), self.sB, w, dt)
        self.bias = self.slope = self.res = self.stats = None
        self.bias_v = (torch.randn(Z, N, generator=g) * 0.3).double()    # fp32 parameters, exact in fp64
        self.bias_v[:, Nv:] = NAN                                       # read only for valid columns
        self.slope_v = torch.tensor([0.25, -0.3, 1.7]).double()            # a negative slope and one above 1
        if ksplit == 1:
            self.bias = self._flat(self.bias_v, self.sBias)
        if epi == EPI_PRELU_STATS:
            self.slope = self._flat(self.slope_v[:, None], self.sSlope)
            self.prefill = torch.tensor([[2.5 + b, 1.25 + 0.75 * b] for b in range(B)], dtype=torch.float64).repeat(Z, 1, 1)
            st = torch.full((Z * self.sStats,), NAN, dtype=torch.float64)
            for z in range(Z):
                st[z * self.sStats: z * self.sStats + 2 * B] = self.prefill[z].reshape(-1)
            self.stats = st.cuda()
        if epi in (EPI_RESIDUAL, EPI_MASK_POS):
            r = torch.randn(Z, R_, N, generator=g).to(dt).double()
            if epi == EPI_MASK_POS:                    # exact zeros, negatives (randn) and NaN inside the valid region
                pick = torch.rand(Z, R_, N, generator=g)
                r[pick < 0.1] = 0.0
                r[(pick >= 0.1) & (pick < 0.15)] = NAN
                r[(pick >= 0.15) & (pick < 0.2)] = -0.0
            else:
                r[:, ~valid_row] = NAN
                r[..., Nv:] = NAN
            self.r = r
            self.res = self._strided((Z, R_, self.ldres), self.sRes, r, dt)
        n_slab = Z * ksplit
        self.C = torch.full((n_slab * self.sC,), NAN, dtype=torch.float32 if epi == EPI_PLAIN_F32 else dt, device="cuda")

    @staticmethod
    def _strided(shape, stride, vals, dt):
        """[Z][rows][ld] at batch stride `stride` in a NaN buffer, vals [Z][rows][cols] in the leading columns"""
        Z, rows, ld = shape
        buf = torch.full((Z * stride,), NAN, dtype=dt)
        for z in range(Z):
            v = buf[z * stride: z * stride + rows * ld].view(rows, ld)
            v[:, :vals.shape[2]] = vals[z].to(dt)
        return buf.cuda()

    @staticmethod
    def _flat(vals, stride):
        buf = torch.full((vals.shape[0] * stride,), NAN)
        for z in range(vals.shape[0]):
            buf[z * stride: z * stride + vals.shape[1]] = vals[z].float()
        return buf.cuda()

    def run(self):
        from nppc_audio import _hip as H
        H.call("nppc_gemm_nt", self.prec, self.epi, self.A, self.lda, self.sA, self.W, self.ldb, self.sB, self.C, self.ldc, self.sC,
               self.bias, self.sBias, self.res, self.ldres, self.sRes, self.slope, self.sSlope, self.stats, self.sStats,
               self.R, self.N, self.K, self.Tp, self.Tv, self.Nv, self.relu_in, self.Z, self.ksplit, H.stream())
        torch.cuda.synchronize()

    def out(self, slab):
        """slab [R][ldc] of the output buffer (slab = z * ksplit + s)"""
        return self.C[slab * self.sC: slab * self.sC + self.R * self.ldc].view(self.R, self.ldc).cpu()

    def reference(self, z, k0, k1, with_epi):
        """(fp64 value, magnitude of its terms) of output z over the K columns [k0, k1)"""
        a = self.a[z, :, k0:k1].clone()
        a[~self.valid_row] = 0.0
        if self.relu_in:
            a = a.clamp_min(0.0)
        w = torch.nan_to_num(self.w[z, :, k0:k1], nan=0.0)
        v = a @ w.T
        mag = a.abs() @ w.abs().T
        if with_epi and self.bias is not None:
            b = torch.nan_to_num(self.bias_v[z], nan=0.0)
            v, mag = v + b, mag + b.abs()
        if with_epi and self.epi == EPI_PRELU_STATS:
            s = float(self.slope_v[z])
            v = torch.where(v > 0, v, s * v)
            mag = mag * max(1.0, abs(s))
        if with_epi and self.epi == EPI_RELU:
            v = v.clamp_min(0.0)
        if with_epi and self.epi == EPI_RESIDUAL:
            r = torch.nan_to_num(self.r[z], nan=0.0)
            v, mag = v + r, mag + r.abs()
        if with_epi and self.epi == EPI_MASK_POS:
            keep = self.r[z] > 0                   # NaN > 0 is False: masked, like the kernel's !(res > 0)
            v = torch.where(keep, v, torch.zeros_like(v))
        v[~self.valid_row] = 0.0
        v[:, self.Nv:] = 0.0
        return v, mag

    def check_padding(self, o):
        """padding region exactly 0, nothing NaN inside [R][N], the ld columns past N untouched"""
        assert not bool(torch.isnan(o[:, :self.N].float()).any())
        assert not bool(o[~self.valid_row, :self.N].float().any())
        assert not bool(o[:, self.Nv:self.N].float().any())
        assert bool(torch.isnan(o[:, self.N:].float()).all())


@pytest.mark.parametrize("Tv,Tp", TV_CASES)
@pytest.mark.parametrize("prec,epi,kern,lay", _nt_cases())
def test_gemm_nt_epilogues_match_fp64(prec, epi, kern, lay, Tv, Tp, record_err):
    N, K = KERNEL_SHAPE[kern]
    i = [1, 37, 127, 128, 129, 200].index(Tv)
    Nv = N - 1 if i % 2 == 0 else NV_SMALL[N]
    relu_in = i % 3 == 1 or (epi == EPI_RELU and i % 3 == 2)
    nt = _NT(prec, epi, N, K, Nv, Tv, Tp, lay, int(relu_in), 1, seed=1000 * epi + 10 * i + prec + 7 * len(kern) + len(lay))
    nt.run()
    worst = 0.0
    for z in range(nt.Z):
        o = nt.out(z)
        nt.check_padding(o)
        ref, mag = nt.reference(z, 0, K, True)
        uo = U32 if epi == EPI_PLAIN_F32 else u_out(prec)
        bound = uo * ref.abs() + 2 * math.sqrt(K) * U32 * mag + 4 * U32 * ref.abs()
        worst = max(worst, bound_ratio(o[:, :N], ref, bound))
        if epi == EPI_MASK_POS:
            off = ~(nt.r[z] > 0)
            assert float(o[:, :N][off].float().abs().max()) == 0.0         # masked by selection: exact zeros
    record_err("C", worst, 1.0)
    if epi == EPI_PRELU_STATS:
        vals = torch.stack([nt.out(z)[:, :N].double().view(nt.B, Tp, N)[:, :Tv].reshape(nt.B, -1) for z in range(nt.Z)])
        st = nt.stats.cpu()
        n_lane = {"reg": 32, "lds64": 32, "lds128": 64}[kern]       # fp32 terms per lane before the fp64 reduction
        got = torch.stack([st[z * nt.sStats: z * nt.sStats + 2 * nt.B].view(nt.B, 2) for z in range(nt.Z)])
        record_err("stats", stats_ratio(got, nt.prefill, vals, n_lane), 1.0)
        for z in range(nt.Z):                  # the gap past the B samples of a branch is untouched
            assert bool(torch.isnan(st[z * nt.sStats + 2 * nt.B: (z + 1) * nt.sStats]).all())


@pytest.mark.parametrize("prec,kern,ksplit", [(0, "reg", 2), (0, "reg", 4), (0, "lds64", 2), (0, "lds128", 4), (1, "lds64", 4),
                                              (1, "lds128", 2)])
def test_gemm_nt_split_k_slabs_sum_to_the_product(prec, kern, ksplit, record_err):
    """epi 4 with ksplit > 1: slab z * ksplit + s holds the product over K columns [s K/ks, (s+1) K/ks), masked like every
    epilogue; the slabs add up to the whole product.  Kernel per K slice: "reg" K/ks = 96 (bf16), "lds64" N = 320,
    "lds128" N = 256."""
    N = KERNEL_SHAPE[kern][0]
    K = {"reg": 96, "lds64": 64 if prec == 0 else 32, "lds128": 128 if prec == 0 else 32}[kern] * ksplit
    Tv, Tp = 100, 128
    nt = _NT(prec, EPI_PLAIN_F32, N, K, N - 63, Tv, Tp, "acc", int(ksplit == 4), ksplit, seed=11 * ksplit + len(kern) + prec)
    nt.run()
    Ks = K // ksplit
    w_slice, w_sum = 0.0, 0.0
    for z in range(nt.Z):
        total = torch.zeros(nt.R, N, dtype=torch.float64)
        for s in range(ksplit):
            o = nt.out(z * ksplit + s)
            nt.check_padding(o)
            ref, mag = nt.reference(z, s * Ks, (s + 1) * Ks, False)
            w_slice = max(w_slice, bound_ratio(o[:, :N], ref, U32 * ref.abs() + 2 * math.sqrt(Ks) * U32 * mag))
            total += o[:, :N].double()
        ref, mag = nt.reference(z, 0, K, False)
        w_sum = max(w_sum, bound_ratio(total, ref, 2 * math.sqrt(K) * U32 * mag + ksplit * U32 * mag))
    record_err("slab", w_slice, 1.0)
    record_err("sum", w_sum, 1.0)


def test_gemm_nt_argument_guards():
    from nppc_audio import _hip as H
    Z, Tp, Tv, N, K = 1, 128, 100, 128, 64
    R_ = Tp
    A = torch.zeros(R_ + 128, K + 32, dtype=torch.bfloat16, device="cuda")
    W = torch.zeros(N + 64, K + 32, dtype=torch.bfloat16, device="cuda")
    C = torch.zeros(R_ + 128, N + 64, dtype=torch.float32, device="cuda")
    res = torch.zeros_like(C).bfloat16()
    bias = torch.zeros(N, device="cuda")
    slope = torch.zeros(1, device="cuda")
    st = torch.zeros(2, dtype=torch.float64, device="cuda")

    def nt(epi=0, lda=K, ldb=K, R=R_, N_=N, K_=K, Tp_=Tp, bias_=None, res_=None, slope_=None, st_=None, ksplit=1):
        H.call("nppc_gemm_nt", 0, epi, A, lda, 0, W, ldb, 0, C, N + 64, 0, bias_, 0, res_, N + 64, 0, slope_, 0, st_, 2, R, N_, K_,
               Tp_, Tv, N_, 0, Z, ksplit, H.stream())

    nt(epi=EPI_PRELU_STATS, slope_=slope, st_=st)                          # the reference call itself is accepted
    nt(epi=EPI_PLAIN_F32, ksplit=2)
    for kw in (dict(R=R_ + 64), dict(N_=N + 32), dict(K_=K + 16), dict(Tp_=Tp + 64), dict(lda=K + 4), dict(ldb=K + 4),
               # split K: only the raw fp32 slabs, with no bias and no statistics (a K slice holds a partial sum)
               dict(epi=EPI_PLAIN, ksplit=2), dict(epi=EPI_RELU, ksplit=2, bias_=bias), dict(epi=EPI_PLAIN_F32, ksplit=2, bias_=bias),
               dict(epi=EPI_PLAIN_F32, ksplit=2, st_=st), dict(epi=EPI_RESIDUAL, ksplit=2, res_=res),
               dict(epi=EPI_MASK_POS, ksplit=4, res_=res), dict(epi=EPI_PRELU_STATS, ksplit=2, slope_=slope, st_=st)):
        with pytest.raises(RuntimeError, match="unsupported"):
            nt(**kw)
    for kw in (dict(epi=EPI_PRELU_STATS, st_=st), dict(epi=EPI_PRELU_STATS, slope_=slope), dict(epi=EPI_RESIDUAL),
               dict(epi=EPI_MASK_POS), dict(epi=6, res_=res, st_=st), dict(epi=7)):
        with pytest.raises(RuntimeError, match="bad argument"):
            nt(**kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- nppc_tcn_dwconv
def _dw_reference(y1, P, z, dil):
    """y1 [B,Cc,Tv] fp64 (stored values) -> (out, magnitude of the fp32 terms): group_norm -> depthwise conv -> PReLU"""
    B, Cc, Tv = y1.shape
    g, be, wd, bd, a2 = P["g"][z], P["b"][z], P["wd"][z], P["bd"][z], float(P["a2"][z])
    z1 = F.group_norm(y1, 1, g, be, EPS)
    u = F.conv1d(z1, wd.view(Cc, 1, 3), bd, padding=dil, dilation=dil, groups=Cc)
    out = torch.where(u > 0, u, a2 * u)
    # magnitude of what the kernel adds in fp32: z = y * (gamma rstd) + (beta - mean gamma rstd), o = bd + sum_k w_k z_k
    m = y1.mean(dim=(1, 2), keepdim=True)
    var = ((y1 - m) ** 2).mean(dim=(1, 2), keepdim=True)
    gr = g.abs().view(1, Cc, 1) / torch.sqrt(var + EPS)
    zmag = y1.abs() * gr + be.abs().view(1, Cc, 1) + m.abs() * gr
    mag = F.conv1d(zmag, wd.abs().view(Cc, 1, 3), bd.abs(), padding=dil, dilation=dil, groups=Cc) * max(1.0, abs(a2))
    return out, mag


# (Cc, Tv, dil, near_constant): Cc = 8 (one chunk), 192 (256 % 24 != 0: idle lanes), 2048 (Cc/8 = 256, the largest);
# dil >= Tv; Tv around the 32-frame workgroup edge
DW_CASES = [(8, 1, 1, 0), (8, 33, 64, 0), (64, 2, 1, 0), (64, 31, 2, 0), (64, 130, 9, 0), (192, 32, 5, 0), (192, 33, 1, 0),
            (192, 130, 64, 0), (512, 31, 9, 0), (512, 130, 2, 0), (2048, 33, 5, 0), (2048, 130, 1, 0), (2048, 2, 64, 0),
            (64, 70, 2, 1), (512, 33, 9, 1)]


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("Cc,Tv,dil,const", DW_CASES)
def test_dwconv_matches_groupnorm_depthwise_prelu(prec, Cc, Tv, dil, const, record_err):
    from nppc_audio import _hip as H
    Z, B = 3, 2
    Tp = 128 if Tv <= 128 else 256
    ld = Cc + 8
    dt = H.dtype_of(prec)
    g = torch.Generator().manual_seed(Cc + 10 * Tv + dil + 1000 * const + prec)
    if const:
        # near-constant: 0.5 everywhere but a few entries one bf16 step up -> variance ~ eps = 1e-8, the clamp and eps decide
        y1 = torch.full((Z, B, Cc, Tv), 0.5, dtype=torch.float64)
        y1[torch.rand(Z, B, Cc, Tv, generator=g) < 0.002] = 0.5 + 2.0 ** -8
        y1[0, 0] = 0.5                                 # exactly constant: variance 0 (or a rounding below it: the clamp)
    else:
        y1 = (torch.randn(Z, B, Cc, Tv, generator=g) * torch.tensor([1.0, 4.0]).view(1, B, 1, 1) + 0.3).to(dt).double()
    sP = 3 * Cc + 24
    P = {k: torch.randn(Z, Cc, generator=g).double() * s + o for k, s, o in (("g", 0.3, 1.0), ("b", 0.3, 0.0), ("bd", 0.2, 0.0))}
    P["wd"] = torch.randn(Z, Cc, 3, generator=g).double() * 0.6            # non-symmetric taps
    P["a2"] = torch.tensor([0.25, -0.4, 1.3], dtype=torch.float64)

    def par(v):
        buf = torch.full((Z * sP,), NAN)
        for z in range(Z):
            buf[z * sP: z * sP + v[z].numel()] = v[z].reshape(-1).float()
        return buf.cuda()

    P = {k: v.float().double() for k, v in P.items()}                      # what the kernel reads (fp32 parameters)
    sAct = B * Tp * ld + 16
    inp = torch.full((Z * sAct,), NAN, dtype=dt)
    for z in range(Z):
        inp[z * sAct: z * sAct + B * Tp * ld].view(B, Tp, ld)[:, :Tv, :Cc] = y1[z].permute(0, 2, 1).to(dt)
    inp = inp.cuda()
    out = torch.full((Z * sAct,), NAN, dtype=dt, device="cuda")
    sSt = 2 * B + 2
    st1 = torch.full((Z * sSt,), NAN, dtype=torch.float64)
    st2 = torch.full((Z * sSt,), NAN, dtype=torch.float64)
    prefill = torch.tensor([[1.5, 7.25], [-3.0, 0.5]], dtype=torch.float64)
    for z in range(Z):
        st1[z * sSt: z * sSt + 2 * B] = torch.stack([y1[z].sum(dim=(1, 2)), (y1[z] ** 2).sum(dim=(1, 2))], -1).reshape(-1)
        st2[z * sSt: z * sSt + 2 * B] = prefill.reshape(-1)
    st2 = st2.cuda()
    H.call("nppc_tcn_dwconv", prec, inp, out, st1.cuda(), st2, par(P["g"]), par(P["b"]), par(P["wd"]), par(P["bd"]),
           par(P["a2"][:, None]), B, Cc, ld, Tp, Tv, dil, EPS, sAct, sSt, sP, Z, H.stream())
    torch.cuda.synchronize()
    out, st2 = out.cpu(), st2.cpu()
    worst, vals, got_st = 0.0, [], []
    for z in range(Z):
        o = out[z * sAct: z * sAct + B * Tp * ld].view(B, Tp, ld)
        assert not bool(torch.isnan(o[:, :, :Cc].float()).any())
        assert not bool(o[:, Tv:, :Cc].float().any())                                    # padded frames written as 0
        assert bool(torch.isnan(o[:, :, Cc:].float()).all())                             # ld padding untouched
        ref, mag = _dw_reference(y1[z], P, z, dil)
        bound = u_out(prec) * ref.abs() + 8 * U32 * mag          # eight fp32 roundings along z -> w z -> sum -> PReLU
        worst = max(worst, bound_ratio(o[:, :Tv, :Cc].permute(0, 2, 1), ref, bound))
        vals.append(o[:, :Tv, :Cc].double().reshape(B, -1))
        got_st.append(st2[z * sSt: z * sSt + 2 * B].view(B, 2))
        assert bool(torch.isnan(st2[z * sSt + 2 * B: (z + 1) * sSt]).all())
    record_err("y2", worst, 1.0)
    rpi = 256 // (Cc // 8)                                    # frames per pass of a workgroup: 8 * ceil(32 / rpi) terms per lane
    record_err("stats", stats_ratio(torch.stack(got_st), prefill.expand(Z, B, 2), torch.stack(vals), 8 * -(-32 // rpi)), 1.0)


def test_dwconv_argument_guards():
    from nppc_audio import _hip as H
    x = torch.zeros(2 * 128 * 2056, device="cuda")
    st = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = torch.zeros(3 * 2056, device="cuda")
    for Cc in (12, 2056):                                     # Cc % 8, Cc / 8 > 256
        with pytest.raises(RuntimeError, match="bad argument"):
            H.call("nppc_tcn_dwconv", 1, x, x, st, st, p, p, p, p, p, 2, Cc, 2056, 128, 100, 1, EPS, 0, 0, 0, 1, H.stream())


# ---------------------------------------------------------------------------------------------------------------- TCN block + tail
def _block_params(C, Hd, Fo, g):
    P = {"conv1x1.weight": torch.randn(Hd, C, 1, generator=g) / math.sqrt(C), "conv1x1.bias": torch.randn(Hd, generator=g) * 0.1,
         "prelu1.weight": torch.rand(1, generator=g) * 0.5, "norm1.weight": torch.randn(Hd, generator=g) * 0.2 + 1.0,
         "norm1.bias": torch.randn(Hd, generator=g) * 0.2, "depthwise_conv.weight": torch.randn(Hd, 1, 3, generator=g) * 0.5,
         "depthwise_conv.bias": torch.randn(Hd, generator=g) * 0.1, "prelu2.weight": torch.rand(1, generator=g) * 0.5,
         "norm2.weight": torch.randn(Hd, generator=g) * 0.2 + 1.0, "norm2.bias": torch.randn(Hd, generator=g) * 0.2,
         "sconv.weight": torch.randn(C, Hd, 1, generator=g) / math.sqrt(Hd), "sconv.bias": torch.randn(C, generator=g) * 0.1,
         "fc.weight": torch.randn(Fo, C, generator=g) / math.sqrt(C), "fc.bias": torch.randn(Fo, generator=g) * 0.1}
    return {k: v.double() for k, v in P.items()}


def _gn_err(y, e, g, ds):
    """first-order bound of the error of group_norm(y) (per sample over [C, T]) from an element-wise error bound e of the stored
    y and a relative error bound ds of the kernel's (sum, sumsq) of it; the normalisation itself runs in fp64"""
    m = y.mean(dim=(1, 2), keepdim=True)
    var = ((y - m) ** 2).mean(dim=(1, 2), keepdim=True)
    r = 1.0 / torch.sqrt(var + EPS)
    ma, m2 = y.abs().mean(dim=(1, 2), keepdim=True), (y * y).mean(dim=(1, 2), keepdim=True)
    de = e.mean(dim=(1, 2), keepdim=True) + ds * ma
    dvar = 2 * ((y - m).abs() * e).mean(dim=(1, 2), keepdim=True) + ds * (m2 + 2 * m.abs() * ma)
    return g.abs().view(1, -1, 1) * r * (e + de + (y - m).abs() * dvar * r * r / 2)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("C,Tv,dil", [(257, 1, 1), (257, 70, 9), (257, 128, 1), (257, 130, 9), (64, 1, 9), (64, 70, 1),
                                      (64, 128, 9), (64, 130, 1)])
def test_tcn_block_and_tail_match_the_oracle(prec, C, Tv, dil, record_err):
    """conv1x1 + PReLU + statistics (nppc_gemm_nt epi 1) -> nppc_tcn_dwconv -> nppc_tcn_pack_sconv + nppc_gemm_nt_gn (sconv with
    GroupNorm-2 folded in, + skip) -> nppc_gemm_nt epi 3 with relu_in (ReLU, Linear(C -> F), ReLU), three branches with their
    own parameters at a constant stride, against R.tcn_block and relu -> linear -> relu in fp64.

    The bound propagates, to first order, the rounding of every stored intermediate (y1, y2, the folded sconv weights, the
    block output) and the fp32 accumulations through the reference's own arithmetic (absolute values of the linear maps)."""
    from nppc_audio import _hip as H
    Z, B = 3, 2
    Hd, Fo = (512, 257) if C == 257 else (192, 100)
    ldC, ldF = -(-C // 64) * 64, -(-Fo // 64) * 64
    Tp = 128 if Tv <= 128 else 256
    R_ = B * Tp
    dt = H.dtype_of(prec)
    uo = u_out(prec)
    g = torch.Generator().manual_seed(C + Tv + dil + prec)
    Ps = [_block_params(C, Hd, Fo, g) for _ in range(Z)]
    x = torch.randn(Z, B, C, Tv, generator=g).to(dt).double() * torch.tensor([1.0, 2.0]).view(1, B, 1, 1)
    # packed operands as engine.py builds them (weights rounded to the storage type)
    W1 = torch.zeros(Z, Hd, ldC, dtype=dt)
    Wfc = torch.zeros(Z, ldF, ldC, dtype=dt)
    for z in range(Z):
        W1[z, :, :C] = Ps[z]["conv1x1.weight"][:, :, 0].to(dt)
        Wfc[z, :Fo, :C] = Ps[z]["fc.weight"].to(dt)
        Ps[z]["conv1x1.weight"] = W1[z, :, :C].double()[:, :, None]
        Ps[z]["fc.weight"] = Wfc[z, :Fo, :C].double()
        for k in Ps[z]:
            if k not in ("conv1x1.weight", "fc.weight"):
                Ps[z][k] = Ps[z][k].float().double()                     # fp32 parameters
    sP = 4 * Hd + 64

    def par(name, n):
        buf = torch.full((Z * sP,), NAN)
        for z in range(Z):
            buf[z * sP: z * sP + n] = Ps[z][name].reshape(-1)[:n].float()
        return buf.cuda()

    # sconv weight as nppc_tcn_pack_sconv reads it: flat [Z][C][Hd] (fp32), gamma, beta [Hd], bias [C] at the branch stride
    lay_sc = C * Hd + 128
    Wsc = torch.zeros(Z * lay_sc)
    for z in range(Z):
        Wsc[z * lay_sc: z * lay_sc + C * Hd] = Ps[z]["sconv.weight"].reshape(-1).float()
    Wg = torch.full((Z, ldC, Hd), 3.0, dtype=dt, device="cuda")
    u = torch.full((Z, ldC), 3.0, device="cuda")
    v = torch.full((Z, ldC), 3.0, device="cuda")
    g2, b2, bsc = (torch.zeros(Z * lay_sc) for _ in range(3))
    for z in range(Z):
        g2[z * lay_sc: z * lay_sc + Hd] = Ps[z]["norm2.weight"].float()
        b2[z * lay_sc: z * lay_sc + Hd] = Ps[z]["norm2.bias"].float()
        bsc[z * lay_sc: z * lay_sc + C] = Ps[z]["sconv.bias"].float()
    H.call("nppc_tcn_pack_sconv", prec, Wsc.cuda(), g2.cuda(), b2.cuda(), bsc.cuda(), Wg, u, v, C, Hd, ldC, Hd, 1, Z, 0, lay_sc,
           0, ldC * Hd, H.stream())
    X = torch.zeros(Z, B, Tp, ldC, dtype=dt)
    X[:, :, :Tv, :C] = x.permute(0, 1, 3, 2).to(dt)
    X = X.cuda()
    sAct = R_ * Hd
    y1 = torch.full((Z, R_, Hd), NAN, dtype=dt, device="cuda")
    y2 = torch.full((Z, R_, Hd), NAN, dtype=dt, device="cuda")
    stats = torch.zeros(2, Z, B, 2, dtype=torch.float64, device="cuda")     # zeroed once, as the engine does per forward
    Xo = torch.full((Z, R_, ldC), NAN, dtype=dt, device="cuda")
    fb = torch.full((Z, R_, ldF), NAN, dtype=dt, device="cuda")
    s = H.stream()
    H.call("nppc_gemm_nt", prec, EPI_PRELU_STATS, X, ldC, R_ * ldC, W1.cuda(), ldC, Hd * ldC, y1, Hd, sAct, par("conv1x1.bias", Hd),
           sP, None, 0, 0, par("prelu1.weight", 1), sP, stats[0], B * 2, R_, Hd, ldC, Tp, Tv, Hd, 0, Z, 1, s)
    dwp = torch.full((Z * sP,), NAN)
    for z in range(Z):
        dwp[z * sP: z * sP + 3 * Hd] = Ps[z]["depthwise_conv.weight"].reshape(-1).float()
    H.call("nppc_tcn_dwconv", prec, y1, y2, stats[0], stats[1], par("norm1.weight", Hd), par("norm1.bias", Hd), dwp.cuda(),
           par("depthwise_conv.bias", Hd), par("prelu2.weight", 1), B, Hd, Hd, Tp, Tv, dil, EPS, sAct, B * 2, sP, Z, s)
    H.call("nppc_gemm_nt_gn", prec, y2, Hd, sAct, Wg, Hd, ldC * Hd, Xo, ldC, R_ * ldC, u, v, ldC, X, ldC, R_ * ldC, stats[1], B * 2,
           float(Hd * Tv), EPS, R_, ldC, Hd, Tp, Tv, C, Z, s)
    H.call("nppc_gemm_nt", prec, EPI_RELU, Xo, ldC, R_ * ldC, Wfc.cuda(), ldC, ldF * ldC, fb, ldF, R_ * ldF, par("fc.bias", Fo), sP,
           None, 0, 0, None, 0, None, 0, R_, ldF, ldC, Tp, Tv, Fo, 1, Z, 1, s)
    torch.cuda.synchronize()
    Xo, fb, Wg = Xo.cpu().view(Z, B, Tp, ldC), fb.cpu().view(Z, B, Tp, ldF), Wg.cpu()
    assert not bool(torch.isnan(Xo.float()).any()) and not bool(torch.isnan(fb.float()).any())
    assert not bool(Xo[:, :, Tv:].float().any()) and not bool(Xo[..., C:].float().any())        # padding written as exact 0
    assert not bool(fb[:, :, Tv:].float().any()) and not bool(fb[..., Fo:].float().any())
    wx, wf = 0.0, 0.0
    for z in range(Z):
        P = {f"b.{k}": val for k, val in Ps[z].items()}
        xz = x[z]
        ref_x = R.tcn_block(xz, P, "b", dil)
        ref_f = torch.relu(F.linear(torch.relu(ref_x).transpose(1, 2), P["b.fc.weight"], P["b.fc.bias"])).transpose(1, 2)
        # ---- first-order error bound, stage by stage
        p = Ps[z]
        pre1 = F.conv1d(xz, p["conv1x1.weight"], p["conv1x1.bias"])
        a1 = float(p["prelu1.weight"])
        m1 = (F.conv1d(xz.abs(), p["conv1x1.weight"].abs(), p["conv1x1.bias"].abs())) * max(1.0, abs(a1))
        y1r = torch.where(pre1 > 0, pre1, a1 * pre1)
        e_y1 = uo * y1r.abs() + 2 * math.sqrt(ldC) * U32 * m1
        z1 = F.group_norm(y1r, 1, p["norm1.weight"], p["norm1.bias"], EPS)
        _, mag_dw = _dw_reference(y1r, {"g": p["norm1.weight"][None], "b": p["norm1.bias"][None],
                                              "wd": p["depthwise_conv.weight"].view(1, Hd, 3), "bd": p["depthwise_conv.bias"][None],
                                              "a2": p["prelu2.weight"]}, 0, dil)
        ds = 65 * U32                          # (sum, sumsq): at most 64 fp32 terms per lane (epi 1, dwconv), then fp64
        e_z1 = _gn_err(y1r, e_y1, p["norm1.weight"], ds)
        u2 = F.conv1d(z1, p["depthwise_conv.weight"], p["depthwise_conv.bias"], padding=dil, dilation=dil, groups=Hd)
        a2 = float(p["prelu2.weight"])
        y2r = torch.where(u2 > 0, u2, a2 * u2)
        e_y2 = (F.conv1d(e_z1, p["depthwise_conv.weight"].abs(), None, padding=dil, dilation=dil, groups=Hd) * max(1.0, abs(a2)) +
                uo * y2r.abs() + 8 * U32 * mag_dw)
        e_z2 = _gn_err(y2r, e_y2, p["norm2.weight"], ds)
        W2 = p["sconv.weight"][:, :, 0]
        z2 = F.group_norm(y2r, 1, p["norm2.weight"], p["norm2.bias"], EPS)
        m2 = y2r.mean(dim=(1, 2), keepdim=True)
        r2 = 1.0 / torch.sqrt(((y2r - m2) ** 2).mean(dim=(1, 2), keepdim=True) + EPS)
        gW = (W2 * p["norm2.weight"][None, :]).abs()
        # folded sconv: Wg = gamma W rounded (relative uo), u = sum_k beta_k W_k + bias and v = sum_k Wg_k summed in fp32,
        # C = rstd y Wg^T - mean rstd v + u + x in fp32
        bW = W2.abs() @ p["norm2.bias"].abs()
        e_x = (W2.abs() @ e_z2 + uo * r2 * (gW @ (y2r - m2).abs()) +
               2 * math.sqrt(Hd) * U32 * (r2 * (gW @ y2r.abs() + m2.abs() * gW.sum(1)[None, :, None]) + bW.view(1, -1, 1)) +
               4 * U32 * ((W2.abs() @ z2.abs()) + xz.abs() + p["sconv.bias"].abs().view(1, -1, 1)) + uo * ref_x.abs())
        e_f = (p["fc.weight"].abs() @ e_x + 2 * math.sqrt(ldC) * U32 * (p["fc.weight"].abs() @ ref_x.clamp_min(0)) +
               4 * U32 * p["fc.bias"].abs().view(1, -1, 1) + uo * ref_f.abs())
        got_x = Xo[z, :, :Tv, :C].double().permute(0, 2, 1)
        got_f = fb[z, :, :Tv, :Fo].double().permute(0, 2, 1)
        wx = max(wx, bound_ratio(got_x, ref_x, e_x))
        wf = max(wf, bound_ratio(got_f, ref_f, e_f))
    record_err("block", wx, 1.0)
    record_err("tail", wf, 1.0)
