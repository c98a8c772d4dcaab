"""Host side of the fused 2-layer LSTM kernels (csrc/lstm.hip, csrc/lstm_coop.hip, csrc/lstm_ws.hip).

Every launch is decided once: `plan_forward` / `plan_backward` turn the shape, the packed weights and the module switches
into a plan (which kernel, cluster geometry, staging width, workspace sizes, profile label), and `lstm2_forward` /
`lstm2_backward` only obtain the workspaces the plan names and make the one launch it names.  The rest of the
module is the packed weights and the registry of step-persistent workspaces with their sticky time-out counters."""
import ctypes
import os
from typing import NamedTuple

import torch

from . import _hip as H


# bench.py sets this to a list to collect (label, start_event, end_event) around every LSTM launch; the events
# are recorded on the current stream, i.e. the stream the kernels are enqueued on.
PROFILE = None


def _timed(label, fn):
    if PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    PROFILE.append((label, e0, e1))
    return r


class PackedLSTM:
    """Per-wave MFMA B-fragment packing of nn.LSTM(I,Hd,2) weights (+ summed biases)."""

    def __init__(self, I, Hd, prec, device):
        n1, n2, kx = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
        H.call("nppc_lstm2_packed_elems", I, Hd, ctypes.byref(n1), ctypes.byref(n2), ctypes.byref(kx))
        self.I, self.Hd, self.prec, self.kx = I, Hd, prec, kx.value
        dt = H.dtype_of(prec)
        self.wp1 = torch.empty(n1.value, dtype=dt, device=device)
        self.wp2 = torch.empty(n2.value, dtype=dt, device=device)
        self.bias1 = torch.empty(4 * Hd, dtype=torch.float32, device=device)
        self.bias2 = torch.empty(4 * Hd, dtype=torch.float32, device=device)
        # weight-stationary cluster kernel (csrc/lstm_ws.hip): its own A-fragment packing of the same weights
        self.ws = prec == H.PREC_BF16 and Hd == 384 and I <= 64
        if self.ws:
            m1, m2 = ctypes.c_long(), ctypes.c_long()
            H.call("nppc_lstm2_ws_packed_elems", ctypes.byref(m1), ctypes.byref(m2))
            self.wsp1 = torch.empty(m1.value, dtype=dt, device=device)
            self.wsp2 = torch.empty(m2.value, dtype=dt, device=device)
        own_workspaces(self)

    def pack(self, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1):
        ws = [t.detach().contiguous() for t in (w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1)]
        H.call("nppc_lstm2_pack_weights", self.prec, *ws, self.I, self.Hd, self.wp1, self.wp2, self.bias1,
               self.bias2, H.stream())
        if self.ws:
            H.call("nppc_lstm2_ws_pack", ws[0], ws[1], ws[4], ws[5], self.I, self.wsp1, self.wsp2, H.stream())
        return self


def pick_mtile(n_seq, prec, train, n_cu=256):
    """Rows per workgroup = 16*mtile: fill the CUs first, then grow the tile (weight reuse)."""
    if prec == H.PREC_F32:
        return 1
    for mt in ((2,) if train else (3, 2)):
        if (n_seq + 16 * mt - 1) // (16 * mt) >= n_cu * 2 // 3:
            return mt
    return 1


_WS = {}
COOP = True          # use the cooperative (weights split over CU pairs) kernels when the shape allows it
# weight-stationary 12-CU clusters (csrc/lstm_ws.hip) for the forward: "0" never, "1" inference launches, "2" also the training
# forward, "auto" (default) inference launches the streaming plan would give to clusters of four CUs or more
WS_MODE = os.environ.get("NPPC_LSTM_WS", "auto")
WS = WS_MODE != "0"
N_CU = None


def _n_cu():
    global N_CU
    if N_CU is None:
        N_CU = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return N_CU


def _flag_blocks():
    return [t for k, t in _WS.items() if k[0][-1] == "coop_flags"]


_RETIRED_TIMEOUTS = 0      # time-outs counted in flag blocks that have been released with their owner


def coop_timeouts():
    """Bounded hand-off spins that gave up since the counters were last cleared (0 on a healthy run).  The counter word
    of every flag block is STICKY: kernels only add to it and no launcher clears it (csrc/lstm_coop.hip), so a time-out
    in ANY earlier launch is still visible here.  Reads the device (one small copy per flag block: call it where the
    host synchronises anyway)."""
    return _RETIRED_TIMEOUTS + sum(int(t[-4].item()) for t in _flag_blocks())


_GUARDS = [None, ()]


def timeout_guards():
    """(device int64 tensor of the addresses of every live sticky time-out counter, count) for nppc_adam_step_guarded;
    rebuilt only when the set of flag blocks changes (a host -> device copy of a few words)"""
    blocks = _flag_blocks()
    key = tuple(t.data_ptr() for t in blocks)
    if _GUARDS[1] != key or _GUARDS[0] is None:
        ptrs = [t[-4:].data_ptr() for t in blocks]
        _GUARDS[0] = torch.tensor(ptrs or [0], dtype=torch.int64, device=blocks[0].device if blocks else "cuda")
        _GUARDS[1] = key
    return _GUARDS[0], len(blocks)


def clear_coop_timeouts():
    global _RETIRED_TIMEOUTS
    _RETIRED_TIMEOUTS = 0
    for t in _flag_blocks():
        t[-4:].zero_()


def release_workspaces(owner_id):
    """drop every step-persistent workspace of one owner (a packed-weight object or an engine; key[1] of its workspace
    keys is id(owner)).  Registered as a weakref finalizer by the owners, so the tens of GB of saved LSTM state of a
    deleted model return to the allocator instead of living as long as the process."""
    global _RETIRED_TIMEOUTS
    for k in [k for k in _WS if len(k[0]) > 1 and k[0][1] == owner_id]:
        t = _WS.pop(k)
        if k[0][-1] == "coop_flags":
            try:
                _RETIRED_TIMEOUTS += int(t[-4].item())
            except Exception:          # interpreter / device shutting down
                pass


def own_workspaces(owner):
    import weakref
    weakref.finalize(owner, release_workspaces, id(owner))


def check_coop_timeouts(where):
    """raise if any cooperative LSTM hand-off timed out: the kernels carry on with wrong numbers after a time-out, so
    everything computed since (gradients, Adam state) is suspect"""
    n = coop_timeouts()
    if n:
        clear_coop_timeouts()
        raise RuntimeError(f"{n} cooperative LSTM hand-off time-out(s) detected at {where}: a partner workgroup was not "
                           "co-resident or stalled; results since the last check are invalid")


def workspace(key, shape, dtype, device, zero=False):
    """Step-persistent device workspace (allocated, and if asked zeroed, ONCE: kernels never touch the padding)."""
    k = (key, tuple(shape), dtype, str(device))
    t = _WS.get(k)
    if t is None:
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=device)
        _WS[k] = t
    return t


COOP_BWD_KSPLIT = True    # cooperative backward variant: True = K-split (bf16 partial-sum exchange), False = output-split
# K-split backward on four-CU clusters of 64 sequences instead of CU pairs of 32 (half the weight-fragment bytes per CU and step):
# "1" whenever ceil(N / 64) * 4 CUs are free, "0" never
BWD_G4 = os.environ.get("NPPC_LSTM_BWD_G4", "0")
WGRAD_SPLITS = 64             # K-slices of the weight-gradient GEMMs (engine._lstm_wgrad)
ROW_PAD = 64 * WGRAD_SPLITS   # row granularity of their operands: 64-row stages x K-slices; buffers carry this much slack


def padded_rows(R, shift=0):
    """rows to allocate for a [R][cols] GEMM operand: whole ROW_PAD blocks, plus slack for the one-step shift"""
    return (R + ROW_PAD - 1) // ROW_PAD * ROW_PAD + ROW_PAD + shift


def rows_view(flat, Tn, N):
    """[Rpad][cols] zero-padded operand buffer -> its live [Tn][N][cols] prefix"""
    return flat[:Tn * N].view(Tn, N, flat.shape[1])


FUSED_HEAD_MAX_O = 16    # one MFMA column tile


def _coop_plan(N, packed, train):
    """(G, mtile, clusters) of the streaming cooperative forward for N sequences; clusters == 0: no cooperative plan"""
    G, cmt, ncl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    H.call("nppc_lstm2_coop_plan", packed.prec, int(train), N, packed.Hd, _n_cu(), ctypes.byref(G), ctypes.byref(cmt),
           ctypes.byref(ncl))
    return G.value, cmt.value, ncl.value


def ws_plan(N, packed):
    """(clusters, nch_max) of the weight-stationary forward for N sequences, or None"""
    if not getattr(packed, "ws", False):
        return None
    cl, nch = ctypes.c_int(), ctypes.c_int()
    H.call("nppc_lstm2_ws_plan", packed.prec, N, packed.Hd, packed.I, _n_cu(), ctypes.byref(cl), ctypes.byref(nch))
    return (cl.value, nch.value) if cl.value > 0 else None


class ForwardPlan(NamedTuple):
    """the one launch of lstm2_forward for (N, packed, train, mtile, head): decided by plan_forward, read by the launcher"""
    kernel: str        # "single" (nppc_lstm2_fwd), "coop" (nppc_lstm2_fwd_coop), "coop_head" (nppc_lstm2_fwd_coop_head), "ws" (nppc_lstm2_fwd_ws)
    G: int             # CUs per cluster: 1, streaming clusters of 2 / 4 / 8, weight-stationary clusters of 12
    mtile: int         # 16-row tiles per workgroup ("single") or per cluster ("coop*"); 0 for "ws"
    clusters: int      # cooperative clusters (0 for "single")
    nch: int           # "ws": chunks of sequences per cluster (nch_max of nppc_lstm2_ws_plan); else 0
    fused_head: bool   # the kernel takes the output head and leaves head_partial
    x_ld: int          # row width (elements) of x_tm: packed.kx, or 40 for the fused-head CU-pair inference launch
    label: str         # name of the launch in ops_lstm.PROFILE


# packed input rows for the frozen restorer's inference launch (CU-pair kernel with the fused head, which fetches rows of any
# 16-byte multiple width): 40 columns instead of 64 (34 features + the spare column + pad to 16 bytes), -37 % of the staged
# bytes and of the kernel's x reads
X_LD_PACKED = 40


def plan_forward(N, packed, train, mtile=None, head_O=None):
    """mtile: None = the default plan, under the switches COOP / WS / WS_MODE; an int = the single-workgroup kernel with that
    tile; (G, mtile) = that streaming cooperative plan; "ws" = the weight-stationary kernel.  The last three are forced by tests
    and benchmarks and refuse (AssertionError) what they cannot run.  head_O: outputs of the head the caller offers to fuse."""
    default, kx = mtile is None, packed.kx
    fusable = head_O is not None and head_O <= FUSED_HEAD_MAX_O         # one MFMA column tile
    coop = _coop_plan(N, packed, train) if (COOP and default) else (0, 0, 0)
    # "1" | "2": the weight-stationary kernel whenever its plan applies; "auto": only where the streaming plan would not be CU pairs
    if mtile == "ws" or (default and COOP and WS and (not train or WS_MODE == "2")
                         and (WS_MODE != "auto" or (coop[2] > 0 and coop[0] >= 4))):
        ws = ws_plan(N, packed)
        # inference needs the fused head: h2 only lives in a two-slot exchange ring
        if ws is not None and (train or head_O is not None) and (head_O is None or fusable):
            return ForwardPlan("ws", 12, 0, ws[0], ws[1], head_O is not None, kx, "lstm2_fwd_ws")
        assert mtile != "ws", "the weight-stationary plan does not apply to this shape"
    if isinstance(mtile, tuple):
        coop = (*mtile, (N + 16 * mtile[1] - 1) // (16 * mtile[1]))
        assert coop[2] * coop[0] <= _n_cu(), "cooperative launch needs one CU per workgroup"
    G, cmt, ncl = coop
    if ncl > 0 and fusable and G == 2 and (not train or cmt == 2):
        x_ld = X_LD_PACKED if (default and not train and packed.I + 1 <= X_LD_PACKED) else kx
        return ForwardPlan("coop_head", G, cmt, ncl, 0, True, x_ld, f"lstm2_fwd_coop_g{G}")
    if ncl > 0:
        return ForwardPlan("coop", G, cmt, ncl, 0, False, kx, f"lstm2_fwd_coop_g{G}")
    return ForwardPlan("single", 1, pick_mtile(N, packed.prec, train) if default else mtile, 0, 0, False, kx, "lstm2_fwd")


def lstm2_forward(x_tm, packed, train, mtile=None, head=None, plan=None):
    """x_tm [Tn][N][plan.x_ld] (time-major, zero padded) -> dict(h2[, h1, g1, g2, c1, c2]) time-major.
    In train mode h1/h2 are prefixes of zero-padded row buffers (`h1_rows`, `h2_rows`: [Rpad][H]) that the
    weight-gradient GEMMs read directly.
    head = (whp [16][H] packed head weights, O): when the plan fuses the output head (CU-pair and weight-stationary kernels),
    the result carries head_partial [2 or 1][Tn][N][O] fp32 (the caller finishes with nppc_sb_head_finalize) -- in
    inference INSTEAD of h2, in training beside the saved state; any other plan ignores `head`.
    plan: plan_forward(N, packed, train, mtile, O) when the caller has made it already (it staged x_tm at plan.x_ld)."""
    Tn, N, kx = x_tm.shape
    p = plan or plan_forward(N, packed, train, mtile, None if head is None else head[1])
    # rows at the plan's width; full-width rows suit every kernel (the one that takes packed rows is told the pitch)
    assert kx in (p.x_ld, packed.kx) and x_tm.dtype == H.dtype_of(packed.prec)
    Hd, dt, dev = packed.Hd, x_tm.dtype, x_tm.device
    tag, out = ("lstm", id(packed), train), {}
    if train:
        # N zero guard rows in front (h_{-1} = 0): `h1_guard` row r is h1 row r - N, the B operand of the weight-gradient
        # product that pairs the gate gradients of step t with h_{t-1} without shifting the gate gradients
        Rp = padded_rows(Tn * N, N)
        # (N, Tn) in the key: the guard rows in front and the padding rows behind Tn * N must be zero and are zeroed once per
        # buffer; two (N, Tn) pairs with equal N + Rp must not share one (the larger N's guard rows would hold stale h)
        for k in ("h1", "h2"):
            out[k + "_guard"] = workspace(tag + (k, N, Tn), (N + Rp, Hd), dt, dev, zero=True)
            out[k + "_rows"] = out[k + "_guard"][N:]
            out[k] = rows_view(out[k + "_rows"], Tn, N)
        for k, gates in (("c1", ()), ("c2", ()), ("g1", (4,)), ("g2", (4,))):
            out[k] = workspace(tag + (k,), (Tn, N, Hd) + gates, dt, dev)
    whp, O = head if p.fused_head else (None, 0)
    ncl, G, cmt, nch = p.clusters, p.G, p.mtile, p.nch
    saved = [out.get(k) for k in ("g1", "g2", "c1", "c2")]
    if p.kernel == "ws":
        # weight-stationary cluster forward (csrc/lstm_ws.hip).  Inference: h1 / h2 only live in two-slot exchange rings;
        # training keeps the whole saved state and takes the head along when asked
        cst = workspace(tag + ("ws_cst",), (ncl * G * nch * 2048,), torch.float32, dev)
        flags = workspace(tag + ("ws", "coop_flags"), (ncl * nch * 16 + 4,), torch.int32, dev, zero=True)
        h1, h2 = (out["h1"], out["h2"]) if train else [workspace(tag + (k,), (2, N, Hd), dt, dev) for k in ("ws_h1ring", "ws_h2ring")]
        if p.fused_head:
            out["head_partial"] = workspace(tag + ("ws_hpart", O), (1, Tn, N, O), torch.float32, dev)
        launch = ("nppc_lstm2_fwd_ws", int(train), x_tm, packed.wsp1, packed.wsp2, packed.bias1, packed.bias2, h1, h2, *saved, cst,
                  flags, whp, out.get("head_partial"), O, N, Tn, ncl, nch)
    else:
        if p.kernel != "single":
            xch = workspace(tag + ("coop_xch",), (ncl * 2 * 2 * 16 * cmt * Hd,), dt, dev)
            flags = workspace(tag + ("coop_flags",), (ncl * 2 * G + 4,), torch.int32, dev, zero=True)
            xch_args = (xch, xch.numel() * xch.element_size(), flags, N, Tn, packed.I, Hd)
        if p.kernel == "coop_head":
            out["head_partial"] = workspace(tag + ("hpart", O), (2, Tn, N, O), torch.float32, dev)
        elif not train:
            out["h2"] = workspace(tag + ("h2",), (Tn, N, Hd), dt, dev)
        state = (x_tm, packed.wp1, packed.wp2, packed.bias1, packed.bias2, out.get("h2"), out.get("h1"), *saved)
        if p.kernel == "coop_head":
            launch = ("nppc_lstm2_fwd_coop_head", packed.prec, int(train), cmt, *state, *xch_args, whp, out["head_partial"], O, kx)
        elif p.kernel == "coop":
            launch = ("nppc_lstm2_fwd_coop", packed.prec, int(train), G, cmt, *state, *xch_args)
        else:
            launch = ("nppc_lstm2_fwd", packed.prec, int(train), cmt, *state, N, Tn, packed.I, Hd)
    _timed((p.label, int(train), N, Tn, nch or cmt), lambda: H.call(*launch, H.stream()))
    return out


class PackedLSTMBwd:
    """Backward (transposed) packing: B fragment column = input feature, k = unit*4 + gate(i,g,f,o)."""

    def __init__(self, I, Hd, prec, device):
        n1, n2 = ctypes.c_long(), ctypes.c_long()
        H.call("nppc_lstm2_bwd_packed_elems", I, Hd, ctypes.byref(n1), ctypes.byref(n2))
        self.I, self.Hd, self.prec = I, Hd, prec
        dt = H.dtype_of(prec)
        self.wb1 = torch.empty(n1.value, dtype=dt, device=device)
        self.wb2 = torch.empty(n2.value, dtype=dt, device=device)
        own_workspaces(self)
        self.coop = prec == H.PREC_BF16 and Hd == 384 and I <= 64
        if self.coop:
            nc = ctypes.c_long()
            H.call("nppc_lstm2_coop_bwd_packed_elems", ctypes.byref(nc))
            self.cwb1 = torch.empty(nc.value, dtype=dt, device=device)
            self.cwb2 = torch.empty(nc.value, dtype=dt, device=device)
            H.call("nppc_lstm2_coop_bwd2_packed_elems", ctypes.byref(nc))
            self.kwb1 = torch.empty(nc.value, dtype=dt, device=device)     # K-split variant
            self.kwb2 = torch.empty(nc.value, dtype=dt, device=device)
            n4, nx, nf = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
            H.call("nppc_lstm2_coop_bwd4_sizes", 64, ctypes.byref(n4), ctypes.byref(nx), ctypes.byref(nf))
            self.k4wb1 = torch.empty(n4.value, dtype=dt, device=device)    # K-split on four-CU clusters
            self.k4wb2 = torch.empty(n4.value, dtype=dt, device=device)

    def pack(self, w_ih0, w_hh0, w_ih1, w_hh1):
        ws = [t.detach().contiguous() for t in (w_ih0, w_hh0, w_ih1, w_hh1)]
        H.call("nppc_lstm2_pack_weights_bwd", self.prec, *ws, self.I, self.Hd, self.wb1, self.wb2, H.stream())
        if self.coop:
            if COOP_BWD_KSPLIT:
                H.call("nppc_lstm2_coop_bwd2_pack", *ws, self.I, self.kwb1, self.kwb2, H.stream())
                if BWD_G4 != "0":
                    H.call("nppc_lstm2_coop_bwd4_pack", *ws, self.I, self.k4wb1, self.k4wb2, H.stream())
            else:
                H.call("nppc_lstm2_coop_bwd_pack", *ws, self.I, self.cwb1, self.cwb2, H.stream())
        return self


class BackwardPlan(NamedTuple):
    """one launch shape of lstm2_backward: a row of BWD_PLANS, with the sizes for N sequences filled in by plan_backward"""
    entry: str               # entry point for dh2 given
    head_entry: str          # entry point for the fused head backward (dyt, whT instead of dh2); None: this kernel has none
    label: str               # name of the launch in ops_lstm.PROFILE
    G: int                   # CUs per cluster (1: the single-workgroup kernel, no exchange and no flags)
    weights: tuple           # attributes of PackedLSTMBwd: the packing this kernel reads
    xch_key: tuple           # workspace key of the exchange buffer ...
    xch_elems: int           # ... its elements: per cluster in the table, in all in a plan
    xch_dtype: torch.dtype   # ... None: the dtype of the saved state
    flag_key: tuple          # workspace key of the flag block (allocated ZEROED: a stale epoch word is a hand-off that spins) ...
    flag_words: int          # ... its words: per cluster in the table; in all, with the 4 sticky time-out words behind them, in a plan


BWD_PLANS = {
    # K-split on four-CU clusters of 64 sequences; one entry point for both gradient forms; sizes from nppc_lstm2_coop_bwd4_sizes
    "ksplit_g4": BackwardPlan("nppc_lstm2_bwd_coop4", "nppc_lstm2_bwd_coop4", "lstm2_bwd_coop_ksplit_g4", 4, ("k4wb1", "k4wb2"),
                              ("coop_xch4",), None, torch.uint8, ("g4", "coop_flags"), None),
    # K-split on CU pairs of 32 sequences.  C2_XCH bytes of bf16 partial sums [layer][parity][cu][32][384]; C2_FPC = 48: epochs
    # [layer][cu][wave]
    "ksplit": BackwardPlan("nppc_lstm2_bwd_coop2", "nppc_lstm2_bwd_coop2_head", "lstm2_bwd_coop_ksplit", 2, ("kwb1", "kwb2"),
                           ("coop_xch",), 2 * 2 * 2 * 32 * 384, None, ("coop_flags",), 48),
    # output-split on CU pairs of 32 sequences.  Gate gradients [layer][parity][cu] x CB_MC * CB_KC = [32][768]; epochs [layer][cu]
    "osplit": BackwardPlan("nppc_lstm2_bwd_coop", None, "lstm2_bwd_coop_g2", 2, ("cwb1", "cwb2"),
                           ("coop_xch",), 2 * 2 * 2 * 32 * 768, None, ("coop_flags",), 4),
    "single": BackwardPlan("nppc_lstm2_bwd", None, "lstm2_bwd", 1, ("wb1", "wb2"), None, 0, None, None, 0),
}


def plan_backward(N, packed_bwd, coop=None):
    """the BackwardPlan of lstm2_backward(saved of N sequences, ..., packed_bwd, coop=coop) under COOP / COOP_BWD_KSPLIT / BWD_G4"""
    if not ((COOP if coop is None else coop) and packed_bwd.coop and ((N + 31) // 32) * 2 <= _n_cu()):
        return BWD_PLANS["single"]
    if COOP_BWD_KSPLIT and BWD_G4 != "0" and ((N + 63) // 64) * 4 <= _n_cu():
        npk, nx, nf = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        H.call("nppc_lstm2_coop_bwd4_sizes", N, ctypes.byref(npk), ctypes.byref(nx), ctypes.byref(nf))
        return BWD_PLANS["ksplit_g4"]._replace(xch_elems=nx.value, flag_words=nf.value)
    p, ncl = BWD_PLANS["ksplit" if COOP_BWD_KSPLIT else "osplit"], (N + 31) // 32
    return p._replace(xch_elems=ncl * p.xch_elems, flag_words=ncl * p.flag_words + 4)


def bwd_head_fusable(N, packed_bwd, coop=None):
    """True when lstm2_backward will run a K-split cooperative kernel, which can take the head backward (dyt, whT)"""
    return plan_backward(N, packed_bwd, coop).head_entry is not None


def lstm2_backward(saved, dh2, packed_bwd, kx, coop=None, head=None):
    """saved = lstm2_forward(train=True) dict; dh2 [Tn][N][H] -> (dx [Tn][N][kx], dg1_rows, dg2_rows): the gate gradients
    as zero-padded row buffers [Rpad][4H] (row t*N + n, column unit*4 + gate in (i,g,f,o) order).
    head = (dyt [Tn][N][16] bf16, whT [H][32] bf16) with dh2 None: the K-split cooperative kernel forms
    d h2 = dY . Wh itself (only valid when bwd_head_fusable(N, packed_bwd))."""
    Tn, N, Hd = saved["h2"].shape
    dt, dev = saved["h2"].dtype, saved["h2"].device
    tag = ("lstm_bwd", id(packed_bwd))
    dx = workspace(tag + ("dx",), (Tn, N, kx), dt, dev)
    Rp = padded_rows(Tn * N, N)
    dg1 = workspace(tag + ("dg1",), (Rp, 4 * Hd), dt, dev, zero=True)
    dg2 = workspace(tag + ("dg2",), (Rp, 4 * Hd), dt, dev, zero=True)
    p = plan_backward(N, packed_bwd, coop)
    assert head is None or p.head_entry is not None, "the fused head backward needs the K-split cooperative kernel"
    st, wb = [saved[k] for k in ("g1", "g2", "c1", "c2")], [getattr(packed_bwd, w) for w in p.weights]
    if p.G == 1:
        _timed((p.label, 1, N, Tn, 1), lambda: H.call(
            p.entry, packed_bwd.prec, *st, dh2, *wb, dx, dg1, dg2, N, Tn, packed_bwd.I, Hd, H.stream()))
        return dx, dg1, dg2
    fn, grads = (p.entry, (dh2,)) if head is None else (p.head_entry, tuple(head))
    if p.entry == p.head_entry:           # one entry point takes (dh2, dyt, whT), the form not given as null pointers
        grads = (dh2, None, None) if head is None else (None, *head)
    xch = workspace(tag + p.xch_key, (p.xch_elems,), p.xch_dtype or dt, dev)
    flags = workspace(tag + p.flag_key, (p.flag_words,), torch.int32, dev, zero=True)
    _timed((p.label, 1, N, Tn, p.G), lambda: H.call(fn, *st, *grads, *wb, dx, dg1, dg2, xch, xch.numel() * xch.element_size(),
                                                   flags, N, Tn, _n_cu(), H.stream()))
    return dx, dg1, dg2
