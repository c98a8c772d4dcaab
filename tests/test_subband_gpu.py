"""GPU: the sub-band stage and the LSTM output head, kernel by kernel, against fp64 references built from the oracle.

Sub-band stage (csrc/subband.hip, csrc/train_ops.hip): nppc_subband_mean + nppc_subband_stage compute
cat(unfold(src, nb), fb0, fb1, fb2) -> laplace_norm -> band_drop(G) (batch > 1 only) -> time-major [T'][B*F'][KX] with zero
padding and an optional ones column at 2nb+4; nppc_subband_stage_bwd is its gradient with respect to the pre-ReLU full-band
outputs (fullsubnet_plus.py:188-230, feature.py:254-285).  Output head: Linear(Hd -> O) on h2 [T][Nseq][Hd] with the
[t][n] -> [bo][o][fo][t - la] re-layout and look-ahead crop, forward, finalize of partial slabs, backward and the dY gather
(sequence_model.py:118-123).

Every buffer a kernel must not read or write outside the valid region is filled with NaN: padded frames (Tp > Tv), padded
columns (ld > F), the gap between the three full-band slabs, bins past F' * G, rows before the look-ahead."""
import pytest
import torch

from oracle import nppc_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


def amax(t):
    return float(t.float().abs().max()) if t.numel() else 0.0


def rel(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def _geom(B, F, G):
    """(effective drop-band groups, F', Nseq) as the reference computes them: drop_band only for a batch > 1"""
    Geff = G if B > 1 else 1
    Fo = F if Geff <= 1 else (F - F % Geff) // Geff
    return Geff, Fo, B * Fo


def _ref_subband(src, fb, nb, G):
    """src [B,F,Tv], fb [3,B,F,Tv] (fp64, post-ReLU) -> (normalised, drop-banded input [B',F',2nb+4,Tv], scale [B])"""
    unf = R.subband_unfold(src[:, None], nb)
    cat = torch.cat([unf, fb[0][:, :, None], fb[1][:, :, None], fb[2][:, :, None]], dim=2)
    sb = R.laplace_norm(cat)
    if src.shape[0] > 1:
        sb = R.band_drop(sb.permute(0, 2, 1, 3), G).permute(0, 2, 1, 3)
    return sb, 1.0 / (cat.mean(dim=(1, 2, 3)) + 1e-5)


def _time_major(sb, KX, ones_col):
    """[B',F',nfeat,Tv] -> [Tv][B'*F'][KX] zero padded, ones column at nfeat when ones_col"""
    Bo, Fo, nfeat, Tv = sb.shape
    x = torch.zeros(Tv, Bo * Fo, KX, dtype=torch.float64)
    x[:, :, :nfeat] = sb.reshape(Bo * Fo, nfeat, Tv).permute(2, 0, 1)
    if ones_col:
        x[:, :, nfeat] = 1.0
    return x


class _Stage:
    """device buffers of one staging problem: src [B][Tp][ldS], fb = three [B][Tp][ldF] slabs strideFb apart, all NaN
    outside the valid (t < Tv, f < F) region, and the fp64 values the kernels see (bf16-rounded in bf16)"""

    def __init__(self, prec, B, F, nb, Tv, seed):
        from nppc_audio import _hip as H
        self.dt = H.dtype_of(prec)
        self.B, self.F, self.nb, self.Tv = B, F, nb, Tv
        self.Tp, self.ldS, self.ldF = Tv + 3, F + 5, F + 9
        self.strideFb = B * self.Tp * self.ldF + 37                   # NaN gap between the slabs
        g = torch.Generator().manual_seed(seed)
        self.src = (torch.randn(B, F, Tv, generator=g).abs() + 0.05).to(self.dt).double()
        # pre-ReLU full-band outputs: a mix of positive and non-positive entries, the ReLU leaves exact zeros
        self.pre = (torch.randn(3, B, F, Tv, generator=g) * 0.8 + 0.1).to(self.dt).double()
        self.fb = torch.relu(self.pre)
        self.src_d = torch.full((B, self.Tp, self.ldS), NAN, dtype=self.dt, device="cuda")
        self.src_d[:, :Tv, :F] = self.src.permute(0, 2, 1).to(self.dt).cuda()
        self.fb_d = self.slabs()
        for m in range(3):
            self.slab(self.fb_d, m)[:, :Tv, :F] = self.fb[m].permute(0, 2, 1).to(self.dt).cuda()

    def slabs(self):
        return torch.full((3 * self.strideFb,), NAN, dtype=self.dt, device="cuda")

    def slab(self, buf, m):
        n = self.B * self.Tp * self.ldF
        return buf[m * self.strideFb: m * self.strideFb + n].view(self.B, self.Tp, self.ldF)

    def mean(self, prec, work):
        from nppc_audio import _hip as H
        from nppc_audio.engine import unfold_multiplicity
        mult = torch.from_numpy(unfold_multiplicity(self.F, self.nb)).cuda()
        scale = torch.full((self.B,), NAN, device="cuda")
        H.call("nppc_subband_mean", prec, self.src_d, self.ldS, self.fb_d, self.ldF, self.strideFb, mult, scale, work, self.B,
               self.F, self.Tp, self.Tv, 2 * self.nb + 4, H.stream())
        return scale

    def stage(self, prec, scale, G, KX, ones_col):
        from nppc_audio import _hip as H
        _, _, Nseq = _geom(self.B, self.F, G)
        x = torch.full((self.Tv + 1, Nseq, KX), NAN, dtype=self.dt, device="cuda")     # one spare frame: never written
        H.call("nppc_subband_stage", prec, self.src_d, self.ldS, self.fb_d, self.ldF, self.strideFb, scale, x[:self.Tv], self.B,
               self.F, self.Tp, self.Tv, self.nb, G, KX, ones_col, H.stream())
        return x


# (B, G, F, nb, Tv, KX, ones_col): B = 1 skips drop-band; G = 2, 3, 4 with every F % G; Tv below / at / above SM_CHUNKS (16);
# KX = 40 is the production narrow view at nb = 15
STAGE_CASES = [
    (1, 2, 257, 15, 17, 40, 1),
    (3, 2, 33, 3, 5, 16, 0),
    (4, 3, 257, 15, 70, 40, 0),
    (5, 3, 34, 1, 1, 8, 1),
    (7, 3, 33, 15, 17, 64, 1),
    (5, 4, 300, 3, 5, 16, 1),
    (5, 4, 257, 15, 16, 40, 1),
    (6, 4, 35, 1, 70, 8, 0),
    (5, 2, 300, 15, 17, 48, 0),
    (5, 4, 258, 3, 5, 16, 0),
]


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("B,G,F,nb,Tv,KX,ones_col", STAGE_CASES)
def test_subband_stage_forward_matches_reference(prec, B, G, F, nb, Tv, KX, ones_col, record_err):
    """scale and the whole staged buffer (zero padding, ones column and the untouched spare frame included)"""
    st = _Stage(prec, B, F, nb, Tv, seed=1000 * B + 10 * G + Tv)
    work = torch.zeros(2 * B, dtype=torch.float64, device="cuda")
    scale = st.mean(prec, work)
    x = st.stage(prec, scale, G, KX, ones_col)
    torch.cuda.synchronize()
    sb, want_scale = _ref_subband(st.src, st.fb, nb, G)
    want = _time_major(sb, KX, ones_col)
    record_err("scale", rel(scale, want_scale), 1e-6)
    assert bool(torch.isnan(x[Tv].float()).all())                     # nothing written past the Tv frames given
    got = x[:Tv].float()
    assert bool(torch.isfinite(got).all())
    nfeat = 2 * nb + 4
    assert amax(got[:, :, nfeat + ones_col:]) == 0.0
    if ones_col:
        assert bool((got[:, :, nfeat] == 1.0).all())
    record_err("x", rel(got, want), 1e-6 if prec == 1 else 1e-2)


def test_subband_stage_argument_guards():
    """the reference asserts batch > groups when batch > 1 (feature.py:263) and reflect-pads by nb < F bins; rows are staged 8
    elements at a time"""
    st = _Stage(1, 3, 33, 3, 5, seed=5)
    scale = torch.ones(3, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):
        st.stage(1, scale, 3, 16, 0)                                  # B == G
    with pytest.raises(RuntimeError, match="bad argument"):
        st.stage(1, scale, 4, 16, 0)                                  # B < G
    with pytest.raises(RuntimeError, match="bad argument"):
        st.stage(1, scale, 2, 12, 0)                                  # KX % 8 != 0
    with pytest.raises(RuntimeError, match="bad argument"):
        st.stage(1, scale, 2, 8, 0)                                   # 2nb+4 = 10 features do not fit in 8 columns
    narrow = _Stage(1, 3, 5, 5, 5, seed=7)
    with pytest.raises(RuntimeError, match="bad argument"):
        narrow.stage(1, scale, 2, 16, 0)                              # nb >= F: reflect padding needs nb < F
    one = _Stage(1, 1, 33, 3, 5, seed=6)
    one.stage(1, torch.ones(1, device="cuda"), 2, 16, 0)              # B = 1: drop-band is skipped, any G is accepted


@pytest.mark.parametrize("prec", [1, 0])
def test_subband_mean_rearms_its_workspace(prec, record_err):
    """the last workgroup of a sample turns the fp64 total into the scale and zeroes the sum and its arrival counter: a
    second launch on the same workspace (different data, a different number of chunks) starts from zero again"""
    work = torch.zeros(2 * 4, dtype=torch.float64, device="cuda")
    for i, (F, nb, Tv) in enumerate(((257, 15, 70), (33, 3, 5), (300, 1, 17))):
        st = _Stage(prec, 4, F, nb, Tv, seed=40 + i)
        scale = st.mean(prec, work)
        torch.cuda.synchronize()
        _, want = _ref_subband(st.src, st.fb, nb, 2)
        record_err(f"scale{i}", rel(scale, want), 1e-6)
        assert float(work.abs().max()) == 0.0, i                      # sums and counters re-armed


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("B,G,F,nb,Tv,KX,ones_col", STAGE_CASES)
def test_subband_stage_backward_matches_autograd(prec, B, G, F, nb, Tv, KX, ones_col, record_err):
    """dpre_fb against fp64 autograd of the staging composition with respect to the pre-ReLU full-band outputs (src is
    data: the kernel makes no gradient for it); bins a drop-band group leaves out receive only the gradient of the mean"""
    from nppc_audio import _hip as H
    st = _Stage(prec, B, F, nb, Tv, seed=2000 * B + 10 * G + Tv)
    dt = st.dt
    Geff, Fo, Nseq = _geom(B, F, G)
    nfeat = 2 * nb + 4
    work = torch.zeros(2 * B, dtype=torch.float64, device="cuda")
    scale = st.mean(prec, work)
    x = st.stage(prec, scale, G, KX, ones_col)
    torch.cuda.synchronize()
    # dx on the staged layout: correlated with x so the mean term sc * D / N is not lost next to sc * dx; the columns past
    # the features (ones column, padding) are NaN: the kernel must not read them
    g = torch.Generator().manual_seed(3000 + Tv)
    dx = torch.full((Tv, Nseq, KX), NAN, dtype=dt, device="cuda")
    dx[:, :, :nfeat] = (0.7 * x[:Tv, :, :nfeat].float().cpu() + 0.5 * torch.randn(Tv, Nseq, nfeat, generator=g)).to(dt).cuda()
    D = torch.full((B,), NAN, dtype=torch.float64, device="cuda")
    dpre = st.slabs()
    H.call("nppc_subband_stage_bwd", prec, dx, x[:Tv], st.fb_d, scale, D, dpre, B, F, st.Tp, Tv, st.ldF, st.strideFb, nb, G, KX,
           H.stream())
    torch.cuda.synchronize()
    pre = st.pre.clone().requires_grad_(True)
    sb, _ = _ref_subband(st.src, torch.relu(pre), nb, G)
    dxr = dx[:, :, :nfeat].double().cpu().permute(1, 2, 0).reshape(sb.shape)
    (sb * dxr).sum().backward()
    want = pre.grad                                                   # [3,B,F,Tv]
    got = torch.stack([st.slab(dpre, m)[:, :Tv, :F].double().cpu().permute(0, 2, 1) for m in range(3)])
    assert bool(torch.isfinite(got).all())
    tol = 2e-4 if prec == 1 else 4e-2
    record_err("dpre", rel(got, want), tol)
    # the dropped bins (other groups' bins and the bins past F' * G) on their own scale: only -sc * D / N reaches them
    if Geff > 1:
        f = torch.arange(F)
        grp = torch.arange(B) % Geff
        dropped = (f[None, :] % Geff != grp[:, None]) | (f[None, :] >= Fo * Geff)          # [B,F]
        mask = dropped[None, :, :, None].expand_as(want) & (st.pre > 0)
        assert bool(mask.any())
        record_err("dpre_dropped", rel(got[mask], want[mask]), tol)
    else:
        assert Fo == F
    # nothing outside the valid region written: padded frames, padded columns, the gaps between the slabs stay NaN
    valid = torch.zeros(st.B, st.Tp, st.ldF, dtype=torch.bool)
    valid[:, :Tv, :F] = True
    for m in range(3):
        assert bool(torch.isnan(st.slab(dpre, m).float().cpu()[~valid]).all()), m
    for m in range(3):
        gap = dpre[m * st.strideFb + B * st.Tp * st.ldF: (m + 1) * st.strideFb]
        assert bool(torch.isnan(gap.float()).all()), m


# ---------------------------------------------------------------- output head
def _head_ref(h2, wh, bias, la, Fo):
    """h2 [Tn][Nseq][Hd], wh [O][Hd], bias [O] (fp64) -> out [Bq][O][Fo][Tn - la]"""
    Tn, Nseq, _ = h2.shape
    y = h2[la:] @ wh.t() + bias                                       # [To, Nseq, O]
    return y.reshape(Tn - la, Nseq // Fo, Fo, -1).permute(1, 3, 2, 0)


def _head_inputs(prec, Hd, O, la, Bq, Fo, Tn, seed):
    from nppc_audio import _hip as H
    dt = H.dtype_of(prec)
    g = torch.Generator().manual_seed(seed)
    Nseq = Bq * Fo
    h2 = torch.randn(Tn, Nseq, Hd, generator=g).to(dt).double()
    wh = (torch.randn(O, Hd, generator=g) / Hd ** 0.5).to(dt).double()
    bias = torch.randn(O, generator=g).float().double()
    h2_d = h2.to(dt).cuda()
    h2_d[:la] = NAN                                                   # frames before the look-ahead are never read
    return dt, g, Nseq, h2, wh, bias, h2_d


# (prec, Hd, O, la, Bq, Fo, Tn): Hd % 32 != 0 takes the scalar kernel; O > 16 two output passes; Nseq % 16 != 0
HEAD_CASES = [
    (1, 16, 2, 2, 3, 7, 9),
    (0, 48, 20, 1, 2, 33, 6),
    (1, 48, 16, 0, 1, 257, 4),
    (1, 32, 10, 0, 1, 257, 5),
    (0, 32, 16, 2, 3, 7, 37),
    (1, 384, 20, 2, 2, 33, 6),
    (0, 384, 2, 1, 5, 13, 12),
    (1, 384, 10, 2, 1, 257, 3),
    (0, 384, 16, 0, 2, 11, 4),
    (0, 16, 10, 0, 2, 11, 4),
]


@pytest.mark.parametrize("prec,Hd,O,la,Bq,Fo,Tn", HEAD_CASES)
def test_sb_head_forward_matches_reference(prec, Hd, O, la, Bq, Fo, Tn, record_err):
    from nppc_audio import _hip as H
    dt, _, Nseq, h2, wh, bias, h2_d = _head_inputs(prec, Hd, O, la, Bq, Fo, Tn, seed=Hd + O + Tn)
    Opad = (O + 15) // 16 * 16
    whp = torch.zeros(Opad, Hd, dtype=dt, device="cuda")               # packed as the engine does: rows O..Opad-1 zero
    whp[:O] = wh.to(dt).cuda()
    n = Bq * O * Fo * (Tn - la)
    out = torch.full((n + 64,), NAN, device="cuda")
    bias_d = bias.float().cuda()
    H.call("nppc_sb_head", prec, h2_d, whp, bias_d, out, Nseq, Tn, la, Hd, O, Fo, H.stream())
    torch.cuda.synchronize()
    got = out[:n].view(Bq, O, Fo, Tn - la)
    assert bool(torch.isfinite(got).all())
    assert bool(torch.isnan(out[n:]).all())
    record_err("out", rel(got, _head_ref(h2, wh, bias, la, Fo)), 1e-5 if prec == 1 else 1e-4)


# (G, O, la, Bq, Fo, Tn): ns = 128 / O sequences per workgroup (O = 10: ns = 12, 128 % O != 0), Tn - la % 32 != 0
FINALIZE_CASES = [
    (1, 2, 2, 3, 7, 37),
    (2, 10, 1, 2, 33, 70),
    (4, 16, 0, 1, 257, 35),
    (2, 10, 2, 5, 13, 5),
    (4, 2, 2, 2, 11, 40),
    (1, 16, 1, 3, 9, 34),
]


@pytest.mark.parametrize("G,O,la,Bq,Fo,Tn", FINALIZE_CASES)
def test_sb_head_finalize_sums_slabs_in_order(G, O, la, Bq, Fo, Tn, record_err):
    """out = bias + sum_g hpart[g] (g in index order): bit-equal to the same fp32 sum on the host, and to fp64 within rounding"""
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(G * 100 + O + Tn)
    Nseq, To = Bq * Fo, Tn - la
    hpart = torch.randn(G, Tn, Nseq, O, generator=g)
    hpart[:, :la] = NAN                                               # partial sums of frames before the look-ahead: not read
    bias = torch.randn(O, generator=g)
    n = Bq * O * Fo * To
    out = torch.full((n + 64,), NAN, device="cuda")
    H.call("nppc_sb_head_finalize", hpart.cuda(), G, bias.cuda(), out, Nseq, Tn, la, O, Fo, H.stream())
    torch.cuda.synchronize()
    acc = torch.zeros(To, Nseq, O)
    for k in range(G):
        acc = acc + hpart[k, la:]
    want32 = (acc + bias).reshape(To, Bq, Fo, O).permute(1, 3, 2, 0)
    got = out[:n].view(Bq, O, Fo, To).cpu()
    assert torch.equal(got, want32)
    assert bool(torch.isnan(out[n:]).all())
    want = (hpart[:, la:].double().sum(0) + bias.double()).reshape(To, Bq, Fo, O).permute(1, 3, 2, 0)
    record_err("out", rel(got, want), 1e-6)
    with pytest.raises(RuntimeError, match="unsupported"):
        H.call("nppc_sb_head_finalize", hpart.cuda(), G, bias.cuda(), out, Nseq, Tn, la, 17, Fo, H.stream())


@pytest.mark.parametrize("prec,Hd,O,la,Bq,Fo,Tn", HEAD_CASES)
def test_sb_head_backward_matches_autograd(prec, Hd, O, la, Bq, Fo, Tn, record_err):
    """nppc_sb_head_bwd (dh2, and dWh / dbh ADDED to what the buffers hold) and nppc_sb_head_bwd_w against autograd"""
    from nppc_audio import _hip as H
    dt, g, Nseq, h2, wh, bias, h2_d = _head_inputs(prec, Hd, O, la, Bq, Fo, Tn, seed=7 * Hd + O + Tn)
    To = Tn - la
    dout = torch.randn(Bq, O, Fo, To, generator=g)
    h2r, whr, br = (t.clone().requires_grad_(True) for t in (h2, wh, bias))
    (_head_ref(h2r, whr, br, la, Fo) * dout.double()).sum().backward()
    whT = torch.zeros(Hd, 32, dtype=dt, device="cuda")                 # [u][o] = Wh[o][u], columns O..31 zero (as packed)
    whT[:, :O] = wh.t().to(dt).cuda()
    dh2 = torch.full((Tn, Nseq, Hd), NAN, dtype=dt, device="cuda")
    w0, b0 = torch.randn(O * Hd, generator=g), torch.randn(O, generator=g)
    dW = torch.full((O * Hd + 32,), NAN, device="cuda")
    db = torch.full((O + 32,), NAN, device="cuda")
    dW[:O * Hd], db[:O] = w0.cuda(), b0.cuda()
    dout_d = dout.cuda()
    H.call("nppc_sb_head_bwd", prec, dout_d, whT, h2_d, dh2, dW, db, Nseq, Tn, la, Hd, O, Fo, H.stream())
    dW2, db2 = torch.zeros(O, Hd, device="cuda"), torch.zeros(O, device="cuda")
    H.call("nppc_sb_head_bwd_w", prec, dout_d, h2_d, dW2, db2, Nseq, Tn, la, Hd, O, Fo, H.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dh2.float()).all())
    assert amax(dh2[:la]) == 0.0      # no gradient for frames before the look-ahead
    # bf16: the kernel's A fragment is dY in bf16 (2^-9 relative), dh2 is stored in bf16
    record_err("dh2", rel(dh2[la:], h2r.grad[la:]), 1e-5 if prec == 1 else 1e-2)
    tol = 2e-5 if prec == 1 else 1e-4
    assert bool(torch.isnan(dW[O * Hd:]).all()) and bool(torch.isnan(db[O:]).all())
    record_err("dWh", rel(dW[:O * Hd].view(O, Hd).double().cpu() - w0.view(O, Hd).double(), whr.grad), tol)
    record_err("dbh", rel(db[:O].double().cpu() - b0.double(), br.grad), tol)
    record_err("dWh_w", rel(dW2, whr.grad), tol)
    record_err("dbh_w", rel(db2, br.grad), tol)


@pytest.mark.parametrize("O,la,Bq,Fo,Tn", [(2, 2, 3, 7, 9), (10, 0, 2, 33, 6), (16, 1, 1, 257, 5), (13, 2, 5, 13, 40)])
def test_head_dy_gather_rows(O, la, Bq, Fo, Tn):
    """dyt [Tn][Nseq][16] bf16: dout re-laid out, zero past O and before the look-ahead; values already in bf16 pass bit
    for bit, any other fp32 value is rounded to the nearest bf16"""
    from nppc_audio import _hip as H
    g = torch.Generator().manual_seed(O + Tn)
    Nseq, To = Bq * Fo, Tn - la
    for exact in (True, False):
        dout = torch.randn(Bq, O, Fo, To, generator=g) * 3
        if exact:
            dout = dout.to(torch.bfloat16).float()
        dyt = torch.full((Tn + 1, Nseq, 16), NAN, dtype=torch.bfloat16, device="cuda")
        H.call("nppc_head_dy_gather", dout.cuda(), dyt[:Tn], Nseq, Tn, la, O, Fo, H.stream())
        torch.cuda.synchronize()
        want = torch.zeros(Tn, Nseq, 16)
        want[la:, :, :O] = dout.permute(3, 0, 2, 1).reshape(To, Nseq, O)
        got = dyt[:Tn].cpu()
        assert torch.equal(got, want.to(torch.bfloat16)), exact
        if exact:
            assert torch.equal(got.float(), want)
        assert bool(torch.isnan(dyt[Tn].float()).all())
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_head_dy_gather", dout.cuda(), dyt, Nseq, Tn, la, 17, Fo, H.stream())     # 16 columns per row
