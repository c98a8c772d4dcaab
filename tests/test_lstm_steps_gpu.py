"""Step-local fp64 checks of every launch plan of the fused 2-layer LSTM (nppc_audio/ops_lstm.py).

The whole-sequence comparisons of test_lstm_gpu.py let bf16 error build up over the steps, so their bounds are percent
level.  Here every time step is checked on its own ("teacher forcing"): the fp64 reference of step t starts from the
kernel's OWN saved state of step t - 1, so the element-wise bound does not grow with Tn and is derived term by term from
the number formats and the kernels' arithmetic:

forward (csrc/lstm.hip layer_step, lstm_coop.hip, lstm_ws.hip -- the same cell in all three):
  * operands: bf16 (or fp32) x_t, h_{t-1} and weights as the kernel consumed them; the recurrent h operand IS the stored
    copy (every plan rounds h to T once and both stores and re-reads that value: LDS tile, exchange slices, WS ring), so
    no carried-h term; products exact (bf16) or rounded (fp32), fp32 accumulation + the fp32 bias:
        ACC = gamma(K + 2) * (sum |w||v| + |b|),   K = I + H (layer 1), 2H (layer 2),  gamma(k) = k u / (1 - k u), u = 2^-24
  * fast activations: sigmoid = rcp(1 + __expf(-a)), tanh = 1 - 2 rcp(1 + __expf(2a)) (common.h): v_exp_f32 of a * log2e
    and v_rcp_f32, 1 ulp each, plus the rounding of a * log2e (relative |a| 2^-24 of the exponential):
        ACT(a) = 2^-22 (3 + |a|)   absolute
  * Lipschitz constants sigmoid' <= 1/4, tanh' <= 1 carry ACC into the gates
  * cell state: the kernel carries c in fp32 and STORES it rounded to T; the reference starts from the stored c_{t-1}:
        CARRY_C = u_T / (1 - u_T) |c_{t-1}|     (u_T = 2^-8 for bf16, 0 for fp32: the stored copy is the carried value)
  * fp32 rounding of the few cell operations: OPS = 4 u (|f c| + |i g|) for c, 2 u |h| for h
  * storage rounding of every compared output: STORE = u_T (|ref| + bound)        (round to nearest even, common.h f2bf)

backward (lstm2_bwd_kernel, lstm2_coop_bwd_kernel, lstm2_coop_bwd2_kernel, lstm2_coop_bwd4_kernel):
  * d h2_t = d h2ext_t + W_hh1^T dg2_{t+1},  d h1_t = W_ih1^T dg2_t + W_hh0^T dg1_{t+1},  dx_t = W_ih0^T dg1_t from the
    kernel's own bf16 gate gradients (the stored dg tile is the MFMA operand):  ACC = gamma(K + 2) sum |w||dg|, K = 4H per
    product (8H for d h1, two products summed in fp32)
  * K-split plans ship the partner's partial sums as bf16 (reduce-scatter): XCH = 2^-8 sum |w||dg| over the shipped slices,
    bounded by the whole sum
  * fused head: d h2ext = dY . Wh in fp32 from bf16 dY and Wh:  gamma(16 + 2) sum |dy||wh|
  * dc carried in fp32 by the kernel, in fp64 here from the end (it contracts: dc_t = dct_t f_t); its error bound B is
    carried beside it: B_{t-1} = B_t f_t + (local error of dct_t) f_t + 2 u |dct f|
  * fast tanh of the saved c: ACT(c); fp32 rounding of each product chain: 4 u |result|; storage rounding as above.
Every check reports max(|kernel - ref| / bound) through record_err(tag, fraction, 1.0).
"""
import math

import pytest
import torch

from oracle import nppc_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U_T = {0: 2.0 ** -8, 1: 0.0}        # storage rounding of the kernel's element type: bf16 (RNE), fp32 (stored = carried)
U_XCH = 2.0 ** -8                   # bf16 partial-sum shipments of the K-split backward plans
PRE = "sb_model.sequence_model."
FWD_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1",
             "bias_hh_l1")
BWD_NAMES = ("weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1")
GORD = [0, 2, 1, 3]                 # kernel gate order (i, g, f, o) -> torch gate block (i, f, g, o)


def gamma(k):
    return k * U32 / (1 - k * U32)


def act_err(a):
    return 2.0 ** -22 * (3 + a.abs())


def _weights(I, Hd, seed):
    spec = {k: v for k, v in W.fullsubnet_spec(num_freqs=9, sb_neighbors=(I - 4) // 2, sb_hidden=Hd).items()
            if k.startswith("sb_model.sequence_model")}
    assert spec[PRE + "weight_ih_l0"][1] == I
    return {k: torch.from_numpy(v) for k, v in W.make_weights(spec, seed).items()}


def _dt(prec):
    return torch.bfloat16 if prec == 0 else torch.float32


def _consumed(P, prec, dev):
    """fp64 copies of the weights as the kernels consume them (rounded to the element type) and of the fp32 bias sums"""
    q = {n: P[PRE + n].to(dev).to(_dt(prec)).double() for n in BWD_NAMES}
    for l in (0, 1):
        q[f"b{l}"] = (P[PRE + f"bias_ih_l{l}"].to(dev).float() + P[PRE + f"bias_hh_l{l}"].to(dev).float()).double()
    return q


def _plan_labels(monkeypatch):
    from nppc_audio import ops_lstm
    prof = []
    monkeypatch.setattr(ops_lstm, "PROFILE", prof)
    return prof


def _frac(diff, bound):
    """worst |kernel - ref| / bound; an element whose bound is 0 (an exact zero, e.g. df at t = 0) must match exactly"""
    f = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, math.inf, 0.0))
    return float(f.max())


# ------------------------------------------------------------------------------------------------------------- forward
def _poison_fwd(pk, train, N, Tn, dt, dev):
    """pre-create the saved-state workspaces lstm2_forward will use with NaN in every live row (zero guard / padding rows
    kept), so a row or column a kernel fails to store cannot pass on stale numbers"""
    from nppc_audio import ops_lstm
    tag = ("lstm", id(pk), train)
    Rp = ops_lstm.padded_rows(Tn * N, N)
    bufs = {}
    for k in ("h1", "h2"):
        b = ops_lstm.workspace(tag + (k, N, Tn), (N + Rp, pk.Hd), dt, dev, zero=True)
        b[N:N + Tn * N].fill_(float("nan"))
        bufs[k + "_guard"] = b
    for k, shp in (("c1", (Tn, N, pk.Hd)), ("c2", (Tn, N, pk.Hd)), ("g1", (Tn, N, pk.Hd, 4)), ("g2", (Tn, N, pk.Hd, 4))):
        bufs[k] = ops_lstm.workspace(tag + (k,), shp, dt, dev)
        bufs[k].fill_(float("nan"))
    return bufs


def _fwd_setup(I, Hd, N, Tn, prec, seed):
    from nppc_audio.ops_lstm import PackedLSTM
    dev = torch.device("cuda")
    P = _weights(I, Hd, seed)
    pk = PackedLSTM(I, Hd, prec, dev).pack(*[P[PRE + n].to(dev) for n in FWD_NAMES])
    g = torch.Generator().manual_seed(1000 * seed + N + Tn)
    x = torch.randn(Tn, N, I, generator=g)
    xt = torch.zeros(Tn, N, pk.kx, dtype=_dt(prec), device=dev)
    xt[:, :, :I] = x.to(dev)
    return P, pk, xt, g


def _run_train_fwd(pk, xt, mtile, head=None):
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import lstm2_forward
    Tn, N, _ = xt.shape
    bufs = _poison_fwd(pk, True, N, Tn, xt.dtype, xt.device)
    ops_lstm.clear_coop_timeouts()
    out = lstm2_forward(xt, pk, True, mtile, head=head)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert out[k].data_ptr() == b.data_ptr(), k          # the poisoned buffers are the ones the kernel wrote
    return out


def _cell_ref(a, c_prev, prec):
    """fp64 gates / cell / hidden of one layer for all steps at once from the pre-activations a [.., H, 4] (kernel order
    i, g, f, o) and their accumulation bound; returns (ref dict, bound dict) for the saved values"""
    A, dA = a
    i, g, f, o = torch.sigmoid(A[..., 0]), torch.tanh(A[..., 1]), torch.sigmoid(A[..., 2]), torch.sigmoid(A[..., 3])
    di = dA[..., 0] / 4 + act_err(A[..., 0])
    dg = dA[..., 1] + act_err(A[..., 1])
    df = dA[..., 2] / 4 + act_err(A[..., 2])
    do = dA[..., 3] / 4 + act_err(A[..., 3])
    carry = U_T[prec] / (1 - U_T[prec]) * c_prev.abs()
    c = f * c_prev + i * g
    dc = (f.abs() + df) * carry + df * c_prev.abs() + (i.abs() + di) * dg + di * g.abs() \
        + 4 * U32 * (f.abs() * (c_prev.abs() + carry) + (i.abs() + di) * (g.abs() + dg))
    tc = torch.tanh(c)
    h = o * tc
    dh = do * tc.abs() + (o.abs() + do) * (dc + act_err(c)) + 2 * U32 * (h.abs() + do + dc)
    gates = torch.stack([i, g, f, o], -1)
    dgates = torch.stack([di, dg, df, do], -1)
    return {"g": gates, "c": c, "h": h}, {"g": dgates, "c": dc, "h": dh}


def _gate_view(a, Tn, N, Hd):
    """[Tn*N, 4H] in torch gate blocks -> [Tn, N, H, 4] in kernel order (i, g, f, o)"""
    return a.view(Tn, N, 4, Hd)[:, :, GORD].permute(0, 1, 3, 2)


def check_forward_steps(tag, out, xt, P, prec, I, record_err):
    """teacher-forced fp64 replay of every step of both layers from the kernel's saved state"""
    Tn, N, _ = xt.shape
    Hd = out["h1"].shape[-1]
    dev = xt.device
    q = _consumed(P, prec, dev)
    u = U_T[prec]
    sv = {k: out[k].double() for k in ("h1", "h2", "c1", "c2", "g1", "g2")}
    for k, v in sv.items():
        assert bool(torch.isfinite(v).all()), (tag, k, "unwritten or non-finite saved state")
    x = xt[:, :, :I].double()
    zero = torch.zeros(1, N, Hd, dtype=torch.float64, device=dev)
    for layer in (1, 2):
        if layer == 1:
            v = torch.cat([x, torch.cat([zero, sv["h1"][:-1]])], -1)          # [x_t | h1_{t-1}], K = I + H
            Wt = torch.cat([q["weight_ih_l0"], q["weight_hh_l0"]], 1)
            b, K = q["b0"], I + Hd
        else:
            v = torch.cat([sv["h1"], torch.cat([zero, sv["h2"][:-1]])], -1)   # [h1_t | h2_{t-1}], K = 2H
            Wt = torch.cat([q["weight_ih_l1"], q["weight_hh_l1"]], 1)
            b, K = q["b1"], 2 * Hd
        v = v.reshape(Tn * N, -1)
        A = v @ Wt.t() + b
        S = v.abs() @ Wt.abs().t() + b.abs()
        A, dA = _gate_view(A, Tn, N, Hd), _gate_view(gamma(K + 2) * S, Tn, N, Hd)
        c_prev = torch.cat([zero, sv[f"c{layer}"][:-1]])
        ref, bnd = _cell_ref((A, dA), c_prev, prec)
        for k, got in (("g", sv[f"g{layer}"]), ("c", sv[f"c{layer}"]), ("h", sv[f"h{layer}"])):
            lim = bnd[k] + u * (ref[k].abs() + bnd[k])
            record_err(f"{tag}:L{layer}:{k}", _frac((got - ref[k]).abs(), lim), 1.0)
    # weight-gradient GEMM contract: N zero guard rows in front of step 0 and zero padding behind Tn * N
    for k in ("h1_guard", "h2_guard"):
        assert float(out[k][:N].abs().max()) == 0, (tag, k, "guard rows")
        assert float(out[k][N + Tn * N:].abs().max()) == 0, (tag, k, "padding rows")


FWD_CASES = [
    # (plan id, prec, Hd, I, N, Tn, mtile): N below / at / just past the row granularity 16 * mtile of each plan
    ("single_f32_h16", 1, 16, 10, 5, 1, 1), ("single_f32_h16", 1, 16, 10, 17, 9, 1),
    ("single_bf16_h16", 0, 16, 10, 33, 7, 2),
    ("single_f32", 1, 384, 34, 17, 5, 1),
    ("single_bf16_mt1", 0, 384, 34, 5, 2, 1), ("single_bf16_mt1", 0, 384, 34, 16, 1, 1), ("single_bf16_mt1", 0, 384, 34, 17, 6, 1),
    ("single_bf16_mt2", 0, 384, 34, 31, 2, 2), ("single_bf16_mt2", 0, 384, 34, 32, 5, 2), ("single_bf16_mt2", 0, 384, 34, 33, 3, 2),
    ("coop_g2_mt2", 0, 384, 34, 5, 1, (2, 2)), ("coop_g2_mt2", 0, 384, 34, 32, 2, (2, 2)), ("coop_g2_mt2", 0, 384, 34, 33, 7, (2, 2)),
    ("coop_g4_mt2", 0, 384, 34, 31, 2, (4, 2)), ("coop_g4_mt2", 0, 384, 34, 65, 5, (4, 2)),
    ("coop_g4_mt4", 0, 384, 34, 63, 3, (4, 4)), ("coop_g4_mt4", 0, 384, 34, 64, 2, (4, 4)), ("coop_g4_mt4", 0, 384, 34, 65, 4, (4, 4)),
    ("coop_g8_mt2", 0, 384, 34, 5, 2, (8, 2)), ("coop_g8_mt2", 0, 384, 34, 33, 5, (8, 2)),
    ("ws", 0, 384, 34, 129, 2, "ws"), ("ws", 0, 384, 34, 160, 1, "ws"), ("ws", 0, 384, 34, 161, 5, "ws"),
    ("ws", 0, 384, 34, 514, 3, "ws"),
    # long runs: the exchange / flag hand-offs repeat hundreds of times under the step-local bound
    ("coop_g2_mt2_long", 0, 384, 34, 100, 256, (2, 2)), ("ws_long", 0, 384, 34, 161, 256, "ws"),
]
FWD_LABEL = {"single": "lstm2_fwd", "coop_g2": "lstm2_fwd_coop_g2", "coop_g4": "lstm2_fwd_coop_g4",
             "coop_g8": "lstm2_fwd_coop_g8", "ws": "lstm2_fwd_ws"}


def _label_of(plan):
    return next(v for k, v in sorted(FWD_LABEL.items(), key=lambda kv: -len(kv[0])) if plan.startswith(k))


@pytest.mark.parametrize("plan,prec,Hd,I,N,Tn,mtile", FWD_CASES,
                         ids=[f"{c[0]}-N{c[4]}-T{c[5]}" for c in FWD_CASES])
def test_forward_steps_match_fp64(plan, prec, Hd, I, N, Tn, mtile, record_err, monkeypatch):
    from nppc_audio import ops_lstm
    P, pk, xt, _ = _fwd_setup(I, Hd, N, Tn, prec, 21)
    prof = _plan_labels(monkeypatch)
    out = _run_train_fwd(pk, xt, mtile)
    assert [p[0][0] for p in prof] == [_label_of(plan)], prof
    assert ops_lstm.coop_timeouts() == 0
    check_forward_steps(f"fwd:{plan}:{'bf16' if prec == 0 else 'f32'}", out, xt, P, prec, I, record_err)


# ------------------------------------------------------------------------------------------------------------ backward
def _gate_rows(Wt, Hd):
    """torch weight [4H (i,f,g,o blocks)][K] -> [4H (row unit*4 + gate, kernel order i,g,f,o)][K]"""
    K = Wt.shape[1]
    return Wt.view(4, Hd, K)[GORD].permute(1, 0, 2).reshape(4 * Hd, K)


def check_backward_steps(tag, saved, dg1_rows, dg2_rows, dx, P, prec, I, record_err, dh2=None, head=None, ksplit=False):
    """fp64 replay of the backward recurrence driven by the kernel's own gate gradients: predicts dg1, dg2 and dx of every
    step from the saved forward state and the kernel's dg of the neighbouring steps"""
    Tn, N, Hd = saved["h2"].shape
    dev = saved["h2"].device
    u = U_T[prec]
    R_ = Tn * N
    for name, rows in (("dg1", dg1_rows), ("dg2", dg2_rows)):
        assert bool(torch.isfinite(rows[:R_].float()).all()), (tag, name, "unwritten or non-finite rows")
        assert float(rows[R_:].float().abs().max()) == 0, (tag, name, "rows past Tn * N must stay zero")
    # dx: every one of its kx columns is written; the columns past I carry W_ih0 columns the packing zeroes -> exactly 0
    assert bool(torch.isfinite(dx.float()).all()), (tag, "dx unwritten or non-finite")
    assert float(dx[:, :, I:].float().abs().max()) == 0, (tag, "dx columns past I must be zero")
    q = _consumed(P, prec, dev)
    Wk = {n: _gate_rows(q[n], Hd) for n in BWD_NAMES}                     # [4H][K]
    dg1 = dg1_rows[:R_].double().view(Tn, N, 4 * Hd)
    dg2 = dg2_rows[:R_].double().view(Tn, N, 4 * Hd)
    zero = torch.zeros(1, N, 4 * Hd, dtype=torch.float64, device=dev)
    dg1n, dg2n = torch.cat([dg1[1:], zero]), torch.cat([dg2[1:], zero])   # dg of step t + 1 (0 past the end)

    def mm(a, n):
        return a @ Wk[n], a.abs() @ Wk[n].abs()

    # layer 2: d h2_t = d h2ext_t + W_hh1^T dg2_{t+1}
    rec2, s2 = mm(dg2n, "weight_hh_l1")
    dh_bnd2 = gamma(4 * Hd + 2) * s2 + (U_XCH * s2 if ksplit else 0)
    if head is not None:
        dyt, whT = head
        dy, wh = dyt.double(), whT.double()[:, :16]
        ext = dy @ wh.t()
        dh_bnd2 = dh_bnd2 + gamma(16 + 2) * (dy.abs() @ wh.abs().t())
    else:
        ext = dh2.double()
    dhs = {2: (ext + rec2, dh_bnd2)}
    # layer 1: d h1_t = W_ih1^T dg2_t + W_hh0^T dg1_{t+1}
    a1, s1a = mm(dg2, "weight_ih_l1")
    b1, s1b = mm(dg1n, "weight_hh_l0")
    dhs[1] = (a1 + b1, gamma(8 * Hd + 2) * (s1a + s1b) + (U_XCH * (s1a + s1b) if ksplit else 0))
    zc = torch.zeros(1, N, Hd, dtype=torch.float64, device=dev)
    for layer, got in ((2, dg2), (1, dg1)):
        gs = saved[f"g{layer}"].double()
        iv, gv, fv, ov = gs[..., 0], gs[..., 1], gs[..., 2], gs[..., 3]
        ct = saved[f"c{layer}"].double()
        cp = torch.cat([zc, ct[:-1]])
        dh, ddh = dhs[layer]
        dh_abs = dh.abs() + ddh
        tc = torch.tanh(ct)
        gtc = (1 - tc * tc)
        loc = dh * ov * gtc                               # dh o (1 - tanh^2 c)
        loc_b = ddh * ov.abs() * gtc + dh_abs * ov.abs() * 2 * tc.abs() * act_err(ct) + 4 * U32 * dh_abs * ov.abs()
        dct = torch.empty_like(loc)
        dct_b = torch.empty_like(loc)
        carry = torch.zeros(N, Hd, dtype=torch.float64, device=dev)         # dc_{t+1} f_{t+1}, fp64
        carry_b = torch.zeros_like(carry)
        for t in range(Tn - 1, -1, -1):
            dct[t] = loc[t] + carry
            dct_b[t] = loc_b[t] + carry_b + 2 * U32 * (loc[t].abs() + carry.abs() + loc_b[t] + carry_b)
            carry = dct[t] * fv[t]
            carry_b = dct_b[t] * fv[t].abs() + 2 * U32 * (carry.abs() + dct_b[t])
        dabs = dct.abs() + dct_b
        d_i = dct * gv * iv * (1 - iv)
        d_g = dct * iv * (1 - gv * gv)
        d_f = dct * cp * fv * (1 - fv)
        d_o = dh * tc * ov * (1 - ov)
        b_i = dct_b * (gv * iv * (1 - iv)).abs() + 4 * U32 * dabs * (gv * iv * (1 - iv)).abs()
        b_g = dct_b * (iv * (1 - gv * gv)).abs() + 4 * U32 * dabs * (iv * (1 - gv * gv)).abs()
        b_f = dct_b * (cp * fv * (1 - fv)).abs() + 4 * U32 * dabs * (cp * fv * (1 - fv)).abs()
        b_o = ddh * (tc * ov * (1 - ov)).abs() + dh_abs * (ov * (1 - ov)).abs() * act_err(ct) \
            + 4 * U32 * dh_abs * (tc * ov * (1 - ov)).abs()
        ref = torch.stack([d_i, d_g, d_f, d_o], -1).view(Tn, N, 4 * Hd)
        bnd = torch.stack([b_i, b_g, b_f, b_o], -1).view(Tn, N, 4 * Hd)
        lim = bnd + u * (ref.abs() + bnd)
        record_err(f"{tag}:dg{layer}", _frac((got - ref).abs(), lim), 1.0)
    # dx_t = W_ih0^T dg1_t
    xr, xs = mm(dg1, "weight_ih_l0")
    xb = gamma(4 * Hd + 2) * xs + (U_XCH * xs if ksplit else 0)
    lim = xb + u * (xr.abs() + xb)
    record_err(f"{tag}:dx", _frac((dx[:, :, :I].double() - xr).abs(), lim[..., :I]), 1.0)


def _poison_bwd(pb, N, Tn, kx, dt, dev):
    from nppc_audio import ops_lstm
    tag = ("lstm_bwd", id(pb))
    Rp = ops_lstm.padded_rows(Tn * N, N)
    bufs = {"dx": ops_lstm.workspace(tag + ("dx",), (Tn, N, kx), dt, dev)}
    bufs["dx"].fill_(float("nan"))
    for k in ("dg1", "dg2"):
        b = ops_lstm.workspace(tag + (k,), (Rp, 4 * pb.Hd), dt, dev, zero=True)
        b[:Tn * N].fill_(float("nan"))
        bufs[k] = b
    return bufs


def _bwd_run(plan, prec, Hd, I, N, Tn, monkeypatch, seed=31, fwd_mtile=1):
    """train forward (its saved state is the backward's input, not under test here) + the backward of `plan`"""
    from nppc_audio import _hip as H
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import PackedLSTMBwd, lstm2_backward
    monkeypatch.setattr(ops_lstm, "COOP_BWD_KSPLIT", not plan.startswith("coop_osplit"))
    monkeypatch.setattr(ops_lstm, "BWD_G4", "1" if plan.startswith("coop4") else "0")
    P, pk, xt, g = _fwd_setup(I, Hd, N, Tn, prec, seed)
    dev = xt.device
    pb = PackedLSTMBwd(I, Hd, prec, dev).pack(*[P[PRE + n].to(dev) for n in BWD_NAMES])   # packs after the flags flip
    saved = _run_train_fwd(pk, xt, fwd_mtile)
    head = dh2 = None
    if plan.endswith("head"):
        O = 10
        dyt = torch.zeros(Tn, N, 16, dtype=torch.bfloat16, device=dev)
        dyt[:, :, :O] = torch.randn(Tn, N, O, generator=g).to(dev)
        whT = torch.zeros(Hd, 32, dtype=torch.bfloat16, device=dev)
        whT[:, :O] = (torch.randn(Hd, O, generator=g) * 0.2).to(dev)
        head = (dyt, whT)
    else:
        dh2 = torch.randn(Tn, N, Hd, generator=g).to(dev).to(_dt(prec))
    bufs = _poison_bwd(pb, N, Tn, pk.kx, _dt(prec), dev)
    prof = _plan_labels(monkeypatch)
    ops_lstm.clear_coop_timeouts()
    dx, dg1, dg2 = lstm2_backward(saved, dh2, pb, pk.kx, coop=not plan.startswith("single"), head=head)
    torch.cuda.synchronize()
    assert dx.data_ptr() == bufs["dx"].data_ptr() and dg1.data_ptr() == bufs["dg1"].data_ptr()
    assert dg2.data_ptr() == bufs["dg2"].data_ptr()
    assert ops_lstm.coop_timeouts() == 0
    return P, saved, (dx, dg1, dg2), dh2, head, [p[0][0] for p in prof]


BWD_LABEL = {"single": "lstm2_bwd", "coop_osplit": "lstm2_bwd_coop_g2", "coop2": "lstm2_bwd_coop_ksplit",
             "coop4": "lstm2_bwd_coop_ksplit_g4"}
BWD_CASES = [
    # (plan id, prec, Hd, I, N, Tn): rows below / at / past the 16-row tile (single), 32-row CU pair, 64-row four-CU cluster
    ("single_f32_h16", 1, 16, 10, 5, 1), ("single_f32_h16", 1, 16, 10, 17, 9),
    ("single_bf16_h16", 0, 16, 10, 33, 6),
    ("single_f32", 1, 384, 34, 17, 4),
    ("single_bf16", 0, 384, 34, 5, 2), ("single_bf16", 0, 384, 34, 16, 1), ("single_bf16", 0, 384, 34, 17, 5),
    ("coop_osplit", 0, 384, 34, 5, 1), ("coop_osplit", 0, 384, 34, 32, 2), ("coop_osplit", 0, 384, 34, 33, 5),
    ("coop_osplit", 0, 384, 34, 65, 3),
    ("coop2", 0, 384, 34, 5, 2), ("coop2", 0, 384, 34, 31, 1), ("coop2", 0, 384, 34, 32, 3), ("coop2", 0, 384, 34, 33, 5),
    ("coop2", 0, 384, 34, 65, 2),
    ("coop2_head", 0, 384, 34, 5, 1), ("coop2_head", 0, 384, 34, 33, 4), ("coop2_head", 0, 384, 34, 77, 2),
    ("coop4", 0, 384, 34, 5, 2), ("coop4", 0, 384, 34, 63, 1), ("coop4", 0, 384, 34, 64, 3), ("coop4", 0, 384, 34, 65, 5),
    ("coop4", 0, 384, 34, 160, 2),
    ("coop4_head", 0, 384, 34, 5, 2), ("coop4_head", 0, 384, 34, 77, 3),
    ("coop2_long", 0, 384, 34, 100, 256), ("coop4_long", 0, 384, 34, 100, 256),
]


@pytest.mark.parametrize("plan,prec,Hd,I,N,Tn", BWD_CASES, ids=[f"{c[0]}-N{c[4]}-T{c[5]}" for c in BWD_CASES])
def test_backward_steps_match_fp64(plan, prec, Hd, I, N, Tn, record_err, monkeypatch):
    P, saved, (dx, dg1, dg2), dh2, head, labels = _bwd_run(plan, prec, Hd, I, N, Tn, monkeypatch)
    want = next(v for k, v in sorted(BWD_LABEL.items(), key=lambda kv: -len(kv[0])) if plan.startswith(k))
    assert labels == [want], labels
    check_backward_steps(f"bwd:{plan}:{'bf16' if prec == 0 else 'f32'}", saved, dg1, dg2, dx, P, prec, I, record_err,
                         dh2=dh2, head=head, ksplit=plan.startswith(("coop2", "coop4")))


@pytest.mark.parametrize("past", [False, True], ids=["at_limit", "past_limit"])
def test_cooperative_backward_size_limit(past, record_err, monkeypatch):
    """the largest N the CU-pair backward accepts is ceil(N / 32) * 2 == the device's CU count; one sequence more falls
    back to the single-workgroup kernel; both step-checked"""
    from nppc_audio import ops_lstm
    n_cu = ops_lstm._n_cu()
    N = (n_cu // 2) * 32 + (1 if past else 0)
    assert (((N + 31) // 32) * 2 <= n_cu) != past
    P, saved, (dx, dg1, dg2), dh2, head, labels = _bwd_run("coop2", 0, 384, 34, N, 2, monkeypatch)
    assert labels == (["lstm2_bwd"] if past else ["lstm2_bwd_coop_ksplit"]), labels
    check_backward_steps(f"bwd:limit:{'single' if past else 'coop2'}:bf16", saved, dg1, dg2, dx, P, 0, 34, record_err,
                         dh2=dh2, ksplit=not past)


# ------------------------------------------------------------------------------------------ fused head / inference
def _head_ref_check(tag, hpart, G, h2, wh, O, bias, record_err):
    """finalise the fused head's partial sums and compare with an fp64 head on the kernel's own saved h2:
    fp32 partial MFMA sums over H/G units each, G partials + bias summed in fp32 -> gamma(H + G + 2) (sum |w||h| + |b|)"""
    from nppc_audio import _hip as H
    Tn, N, Hd = h2.shape
    out = torch.full((1, O, N, Tn), float("nan"), device=h2.device)
    H.call("nppc_sb_head_finalize", hpart, G, bias, out, N, Tn, 0, O, N, H.stream())
    torch.cuda.synchronize()
    whd = wh[:O].double()
    ref = h2.double() @ whd.t() + bias.double()                               # [Tn][N][O]
    lim = gamma(Hd + G + 2) * (h2.double().abs() @ whd.abs().t() + bias.double().abs())
    got = out[0].permute(2, 1, 0).double()
    assert bool(torch.isfinite(got).all()), tag
    record_err(f"{tag}:head", _frac((got - ref).abs(), lim), 1.0)


@pytest.mark.parametrize("plan,N,Tn", [("coop_g2_head", 33, 6), ("coop_g2_head", 100, 64), ("ws_head", 161, 5)])
def test_training_forward_with_fused_head(plan, N, Tn, record_err, monkeypatch):
    """training launch with the head fused (CU-pair cmt == 2, weight-stationary): saved state step-checked and the finalised
    head against fp64 on the kernel's own h2"""
    from nppc_audio import ops_lstm
    I, Hd, O = 34, 384, 10
    P, pk, xt, g = _fwd_setup(I, Hd, N, Tn, 0, 41)
    wh = torch.zeros(16, Hd, dtype=torch.bfloat16, device=xt.device)
    wh[:O] = (torch.randn(O, Hd, generator=g) * 0.1).to(xt.device)
    bias = torch.randn(O, generator=g).to(xt.device)
    prof = _plan_labels(monkeypatch)
    out = _run_train_fwd(pk, xt, (2, 2) if plan.startswith("coop") else "ws", head=(wh, O))
    assert [p[0][0] for p in prof] == ["lstm2_fwd_coop_g2" if plan.startswith("coop") else "lstm2_fwd_ws"]
    assert "head_partial" in out and ops_lstm.coop_timeouts() == 0
    check_forward_steps(f"fwd:{plan}:bf16", out, xt, P, 0, I, record_err)
    _head_ref_check(f"fwd:{plan}:bf16", out["head_partial"], out["head_partial"].shape[0], out["h2"], wh, O, bias,
                    record_err)


INF_CASES = [
    # (plan id, inference mtile, training plan with the same per-row arithmetic, N, Tn)
    ("single_mt1", 1, 1, 17, 6), ("single_mt2", 2, 2, 33, 5), ("single_mt3", 3, 1, 49, 5),
    ("coop_g2_mt2", (2, 2), (2, 2), 33, 6), ("coop_g2_mt5", (2, 5), (2, 2), 81, 5),
    ("coop_g4_mt2", (4, 2), (4, 2), 33, 5), ("coop_g4_mt4", (4, 4), (4, 4), 65, 5),
    ("coop_g8_mt2", (8, 2), (8, 2), 33, 4), ("coop_g8_mt5", (8, 5), (8, 2), 81, 4),
]


@pytest.mark.parametrize("plan,mt_inf,mt_train,N,Tn", INF_CASES, ids=[f"{c[0]}-N{c[3]}-T{c[4]}" for c in INF_CASES])
def test_inference_forward_equals_training_launch(plan, mt_inf, mt_train, N, Tn, monkeypatch):
    """An inference launch saves no state.  Its h2 must be BIT-equal to the training launch's: both are the same template
    (lstm2_fwd_kernel / lstm2_coop_fwd_kernel with TRAIN off), and a row's arithmetic does not depend on the tile height
    mtile -- every output element is the same in-order MFMA chain over the same k-steps of the same bf16 operands, the same
    fp32 cell update, and the ring depth only moves loads.  Plus one short whole-sequence comparison with the fp64 oracle
    at the bf16 tolerance of test_lstm_gpu.py."""
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import lstm2_forward
    I, Hd = 34, 384
    P, pk, xt, _ = _fwd_setup(I, Hd, N, Tn, 0, 51)
    prof = _plan_labels(monkeypatch)
    train = _run_train_fwd(pk, xt, mt_train)["h2"].clone()
    ops_lstm.clear_coop_timeouts()
    inf = lstm2_forward(xt, pk, False, mt_inf)["h2"]
    torch.cuda.synchronize()
    want = "lstm2_fwd" if plan.startswith("single") else f"lstm2_fwd_coop_g{mt_inf[0]}"
    assert [p[0][0] for p in prof][-1] == want
    assert ops_lstm.coop_timeouts() == 0
    d = float((inf.float() - train.float()).abs().max())
    assert torch.equal(inf, train), (plan, d)
    ref = R.lstm2(xt[:, :, :I].float().cpu().permute(1, 0, 2).contiguous(), P, "sb_model.sequence_model").permute(1, 0, 2)
    assert float((inf.float().cpu() - ref).abs().max()) < 3e-2


@pytest.mark.parametrize("plan,N,Tn", [("coop_g2_head_mt2", 33, 6), ("coop_g2_head_mt5", 81, 5), ("ws_head", 161, 5)])
def test_inference_fused_head_equals_training_launch(plan, N, Tn, monkeypatch):
    """inference with the head fused keeps no h2 at all; its head partial sums must be bit-equal to those of the training
    launch of the same kernel (the head GEMM reads the same bf16 h2 tile from LDS: same operands, same order)"""
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import lstm2_forward
    I, Hd, O = 34, 384, 4
    P, pk, xt, g = _fwd_setup(I, Hd, N, Tn, 0, 61)
    wh = torch.zeros(16, Hd, dtype=torch.bfloat16, device=xt.device)
    wh[:O] = (torch.randn(O, Hd, generator=g) * 0.1).to(xt.device)
    mt_inf = {"coop_g2_head_mt2": (2, 2), "coop_g2_head_mt5": (2, 5), "ws_head": "ws"}[plan]
    tr = _run_train_fwd(pk, xt, "ws" if plan == "ws_head" else (2, 2), head=(wh, O))["head_partial"].clone()
    ops_lstm.clear_coop_timeouts()
    inf = lstm2_forward(xt, pk, False, mt_inf, head=(wh, O))
    torch.cuda.synchronize()
    assert "h2" not in inf and ops_lstm.coop_timeouts() == 0
    d = float((inf["head_partial"] - tr).abs().max())
    assert torch.equal(inf["head_partial"], tr), (plan, d)


# -------------------------------------------------------------------------------------------------------- production
def test_production_direction_net_plan_steps(record_err, monkeypatch):
    """BASELINE C2's direction-net plan at full width: N = 4096, the planned training forward (CU pairs, fused 10-output
    head) and the planned backward (K-split CU pairs, fused head backward), every step checked"""
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import PackedLSTMBwd, bwd_head_fusable, lstm2_backward
    monkeypatch.setattr(ops_lstm, "COOP_BWD_KSPLIT", True)
    monkeypatch.setattr(ops_lstm, "BWD_G4", "0")
    monkeypatch.setattr(ops_lstm, "WS_MODE", "auto")
    N, Tn, I, Hd, O = 4096, 3, 34, 384, 10
    P, pk, xt, g = _fwd_setup(I, Hd, N, Tn, 0, 71)
    dev = xt.device
    wh = torch.zeros(16, Hd, dtype=torch.bfloat16, device=dev)
    wh[:O] = (torch.randn(O, Hd, generator=g) * 0.2).to(dev)
    bias = torch.randn(O, generator=g).to(dev)
    prof = _plan_labels(monkeypatch)
    out = _run_train_fwd(pk, xt, None, head=(wh, O))
    assert [p[0][0] for p in prof] == ["lstm2_fwd_coop_g2"] and "head_partial" in out
    check_forward_steps("fwd:prod_c2:bf16", out, xt, P, 0, I, record_err)
    _head_ref_check("fwd:prod_c2:bf16", out["head_partial"], 2, out["h2"], wh, O, bias, record_err)
    pb = PackedLSTMBwd(I, Hd, 0, dev).pack(*[P[PRE + n].to(dev) for n in BWD_NAMES])
    assert bwd_head_fusable(N, pb)
    dyt = torch.zeros(Tn, N, 16, dtype=torch.bfloat16, device=dev)
    dyt[:, :, :O] = torch.randn(Tn, N, O, generator=g).to(dev)
    whT = torch.zeros(Hd, 32, dtype=torch.bfloat16, device=dev)
    whT[:, :16] = wh.t()
    bufs = _poison_bwd(pb, N, Tn, pk.kx, torch.bfloat16, dev)
    ops_lstm.clear_coop_timeouts()
    dx, dg1, dg2 = lstm2_backward(out, None, pb, pk.kx, head=(dyt, whT))
    torch.cuda.synchronize()
    assert prof[-1][0][0] == "lstm2_bwd_coop_ksplit" and dg1.data_ptr() == bufs["dg1"].data_ptr()
    assert ops_lstm.coop_timeouts() == 0
    check_backward_steps("bwd:prod_c2:bf16", out, dg1, dg2, dx, P, 0, I, record_err, head=(dyt, whT), ksplit=True)


def test_production_config5_weight_stationary_plan_steps(record_err, monkeypatch):
    """BASELINE config 5's weight-stationary plan at full width (N = 2056: ragged last chunk, several clusters): the
    training launch step-checked with the head fused and finalised, and the planned inference launch (WS_MODE auto picks
    the cluster kernel here) bit-equal to it on the head partial sums"""
    from nppc_audio import ops_lstm
    from nppc_audio.ops_lstm import lstm2_forward
    N, Tn, I, Hd, O = 2056, 3, 34, 384, 2
    P, pk, xt, g = _fwd_setup(I, Hd, N, Tn, 0, 81)
    dev = xt.device
    wh = torch.zeros(16, Hd, dtype=torch.bfloat16, device=dev)
    wh[:O] = (torch.randn(O, Hd, generator=g) * 0.1).to(dev)
    bias = torch.randn(O, generator=g).to(dev)
    prof = _plan_labels(monkeypatch)
    out = _run_train_fwd(pk, xt, "ws", head=(wh, O))
    check_forward_steps("fwd:prod_c5_ws:bf16", out, xt, P, 0, I, record_err)
    _head_ref_check("fwd:prod_c5_ws:bf16", out["head_partial"], 1, out["h2"], wh, O, bias, record_err)
    tr = out["head_partial"].clone()
    monkeypatch.setattr(ops_lstm, "WS_MODE", "auto")
    monkeypatch.setattr(ops_lstm, "WS", True)
    ops_lstm.clear_coop_timeouts()
    inf = lstm2_forward(xt, pk, False, None, head=(wh, O))
    torch.cuda.synchronize()
    assert [p[0][0] for p in prof] == ["lstm2_fwd_ws", "lstm2_fwd_ws"], prof
    assert ops_lstm.coop_timeouts() == 0
    assert torch.equal(inf["head_partial"], tr), float((inf["head_partial"] - tr).abs().max())
