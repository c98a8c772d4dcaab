"""Launch sequences of the FullSubNet+-shaped nets on the HIP kernels (no torch compute ops).

`FSNEngine` owns the packed weights, the time-major activation buffers and the launch order for
one net (the frozen restorer: 3 input maps; the direction net: 6 maps, 2K outputs).  It mirrors
FullSubNet_Plus.forward (FullSubNet_plus/.../fullsubnet_plus.py:143-230) and
MultiDirectionFullSubNet_Plus.forward (nppc_audio/networks.py:63-163) stage by stage.
"""
import ctypes
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import _hip as H
from .gemm import gemm_nt, gemm_nt_gn, lstm_wgrad_mode, reduce_slabs, reduce_slabs_t
from .ops_lstm import (PackedLSTM, PackedLSTMBwd, ROW_PAD, WGRAD_SPLITS, lstm2_backward, lstm2_forward, own_workspaces, padded_rows,
                       plan_backward, plan_forward, rows_view, workspace)

TCN_HIDDEN = 512
TCN_DILATIONS = (1, 2, 5, 9, 1, 2, 5, 9)
BRANCHES = ("", "_real", "_imag")   # channel_attention{,_real,_imag} / fb_model{,_real,_imag}
EPI_PLAIN, EPI_PRELU_STATS, EPI_RESIDUAL, EPI_RELU, EPI_PLAIN_F32, EPI_MASK_POS = 0, 1, 2, 3, 4, 5
LSTM_PARAMS = "sb_model.sequence_model."
TSSE_PARAMS = tuple(f"channel_attention.{m}.{leaf}" for m in ("smallConv1d.0", "middleConv1d.0", "largeConv1d.0",
                                                              "feature_concate_fc", "fc1", "fc2") for leaf in ("weight", "bias"))
TCN_MID_GRADS = ("norm2.weight", "norm2.bias", "norm1.weight", "norm1.bias", "depthwise_conv.weight", "depthwise_conv.bias",
                 "prelu1.weight", "prelu2.weight", "conv1x1.bias")       # gradients of the fused middle backward, in argument order
TCN_WGRAD_SPLITS = 8         # K-slices of the split-K weight-gradient GEMMs of the full-band model (fc_output_layer; fp32: all)


def rup(a, b):
    return (a + b - 1) // b * b


class BackwardPlan(NamedTuple):
    """what one FSNEngine.backward does where: decided once per buffer set (FSNEngine._backward_plan), read by its stages"""
    fused_head: bool  # the K-split cooperative LSTM kernel forms d h2 = dY . Wh itself from the gathered dY rows: no dh2 tensor
    head_wgrad: bool  # the head's weight gradient h2^T . dY runs with the LSTM weight gradients on the side stream, not in front
    S2: int           # K-slices of the split-K weight-gradient GEMMs of the full-band model: as many as divide the B * Tp rows
    Fr: int           # F rounded up to the 128-row tiles of those GEMMs (rows of the fc_output_layer product)
    Cr: int           # ldC likewise (rows of the sconv.weight product)
    tn_ok: bool       # bf16: the 1x1-conv weight gradients run on the TN GEMM straight from the row-major activations (no transposes)
    cs_ok: bool       # the GEMM that PRODUCES a block's upstream gradient also leaves its column sums: no pass over dXo for sconv.bias
    early: bool       # grad_range_hook gets ranges of the flat gradient as they become final: the sub-band tail, TCN blocks 7..4


class FlatParams:
    """All parameters of a module re-homed into ONE fp32 device buffer (named_parameters order).

    The three full-band branches are identical sub-trees laid out back to back, so any parameter of
    branch z sits at a constant element stride from branch 0: kernels batch the branches over
    blockIdx.z with that single stride.  Parameters stay individual nn.Parameters (views), so
    state_dict()/optimizers see the reference names and shapes.
    """

    def __init__(self, module, device):
        named = list(module.named_parameters())
        total = sum(p.numel() for _, p in named)
        self.flat = torch.empty(total, dtype=torch.float32, device=device)
        self.grad = None
        self.off = {}
        o = 0
        for n, p in named:
            k = p.numel()
            self.flat[o:o + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[o:o + k].view(p.shape)
            self.off[n] = (o, tuple(p.shape))
            o += k
        self.named = named

    def view(self, name):
        o, shp = self.off[name]
        return self.flat[o:o + int(np.prod(shp))].view(shp)

    def gview(self, name):
        o, shp = self.off[name]
        return self.grad[o:o + int(np.prod(shp))].view(shp)

    def version(self):
        """changes whenever any parameter was written: in-place torch ops (load_state_dict, torch optimizers) bump the
        parameter's own counter, the HIP optimizers bump the flat buffer's (trainer.HipAdam / FlatAdamStepper)"""
        return (self.flat._version, sum(p._version for _, p in self.named))

    def ensure_grad(self):
        if self.grad is None:
            self.grad = torch.zeros_like(self.flat)
        return self.grad

    def attention_stride(self):
        """element stride between the three (equally shaped) attention layers channel_attention{,_real,_imag}"""
        names = [n for n, _ in self.named if n.startswith("channel_attention.")]
        a = self.off["channel_attention." + names[0].split(".", 1)[1]][0]
        strides = set()
        for n in names:
            leaf = n.split(".", 1)[1]
            o0, o1, o2 = (self.off[f"channel_attention{br}.{leaf}"][0] for br in BRANCHES)
            strides.add(o1 - o0)
            strides.add(o2 - o1)
        assert len(strides) == 1 and a >= 0
        return strides.pop()

    def branch_stride(self):
        a = self.off["fb_model.fc_output_layer.weight"][0]
        b = self.off["fb_model_real.fc_output_layer.weight"][0]
        c = self.off["fb_model_imag.fc_output_layer.weight"][0]
        assert b - a == c - b > 0
        a2 = self.off["fb_model.sequence_model.0.conv1x1.weight"][0]
        b2 = self.off["fb_model_real.sequence_model.0.conv1x1.weight"][0]
        assert b2 - a2 == b - a
        return b - a


def unfold_multiplicity(F, nb):
    """mult[f] = number of (bin, tap) pairs whose reflected source bin is f (sum of the unfolded block)."""
    m = np.zeros(F, np.float32)
    for f in range(F):
        for j in range(-nb, nb + 1):
            i = f + j
            if i < 0:
                i = -i
            if i >= F:
                i = 2 * (F - 1) - i
            m[i] += 1
    return m


class FSNEngine:
    # engines with side-stream work (weight gradients of a backward in defer_join mode, the re-pack of the updated weights)
    # that the main stream has not been made to wait for yet.  A cooperative LSTM kernel needs every CU for its own
    # workgroups, so NOTHING of ours may be in flight on another stream when one is launched: every engine joins ALL of them
    # right before its LSTM launches (the trainer's pre_lstm_hook normally has done so already), and its OWN pending work
    # at the top of forward / backward, before any kernel reads the packed weights the side stream may still be rewriting.
    import weakref as _weakref
    _unjoined = _weakref.WeakValueDictionary()

    def __init__(self, flat, *, num_freqs, n_maps, out_size, sb_neighbors, look_ahead, sb_hidden, groups, kersize,
                 prec, trainable):
        self.fp = flat
        self.F, self.nm, self.O = num_freqs, n_maps, out_size
        self.nb, self.la, self.Hd, self.G = sb_neighbors, look_ahead, sb_hidden, groups
        self.ks = tuple(kersize)
        self.prec = prec
        self.dt = H.dtype_of(prec)
        self.trainable = trainable
        self.C = n_maps * num_freqs
        self.ldC = rup(self.C, 64)
        self.ldF = rup(num_freqs, 64)
        self.KC = self.ldC                     # K of the input GEMMs: the zero-padded row width (multiple of 64: LDS-staged GEMM path)
        self.dev = flat.flat.device
        self.I = 2 * sb_neighbors + 1 + 3
        self.sP = flat.branch_stride()
        self.sAtt = flat.attention_stride()
        self.packed_version = None
        self._tn_tables = {}                  # problem tables of the grouped TCN weight-gradient launches (_tcn_wgrad_grouped)
        self._side = None                     # side stream for the LSTM weight-gradient GEMMs (backward)
        self._gen = 0                         # train-forward generation: backward must consume the LATEST train forward
        self.last_train = None
        self.grad_range_hook = None           # fn(flat_grad, lo, hi): range final for this step (dp.FlatGradientReducer)
        self.early_buckets_ok = self._check_bucket_layout() if trainable else False
        self.pre_lstm_hook = None             # one-shot callback run right before this engine's next LSTM launch (trainer)
        self.defer_join = False               # backward leaves the side-stream join to the caller (join_side)
        self.join_pending = False
        self.bufs = {}
        own_workspaces(self)                  # step-persistent workspaces keyed by id(self) die with the engine
        self.lstm = PackedLSTM(self.I, self.Hd, prec, self.dev)
        self.KX = self.lstm.kx
        self.mult = torch.from_numpy(unfold_multiplicity(self.F, self.nb)).to(self.dev)
        C, ldC, ldF = self.C, self.ldC, self.ldF
        self.W1p = torch.zeros(8, 3, TCN_HIDDEN, ldC, dtype=self.dt, device=self.dev)
        self.W2p = torch.zeros(8, 3, ldC, TCN_HIDDEN, dtype=self.dt, device=self.dev)      # sconv weights x norm2.weight
        self.u2 = torch.zeros(8, 3, ldC, dtype=torch.float32, device=self.dev)            # norm2.bias through sconv + sconv.bias
        self.v2 = torch.zeros(8, 3, ldC, dtype=torch.float32, device=self.dev)            # row sums of W2p
        self.Wfcp = torch.zeros(3, ldF, ldC, dtype=self.dt, device=self.dev)
        self.Opad = rup(self.O, 16)
        self.Whp = torch.zeros(self.Opad, self.Hd, dtype=self.dt, device=self.dev)
        if trainable:
            if self.O > 32:
                raise NotImplementedError("n_directions <= 16 is what the head-backward kernel is built for")
            self.lstm_bwd = PackedLSTMBwd(self.I, self.Hd, prec, self.dev)
            self.W1T = torch.zeros(8, 3, ldC, TCN_HIDDEN, dtype=self.dt, device=self.dev)   # [c][k] = W1[k][c]
            self.W2T = torch.zeros(8, 3, TCN_HIDDEN, ldC, dtype=self.dt, device=self.dev)   # [k][c] = W2[c][k]
            self.WfcT = torch.zeros(3, ldC, ldF, dtype=self.dt, device=self.dev)            # [c][f] = Wfc[f][c]
            self.WhT = torch.zeros(self.Hd, 32, dtype=self.dt, device=self.dev)             # [u][o] = Wh[o][u]
            self.gbuf = [None, None]

    def _check_bucket_layout(self):
        """the early gradient buckets (backward: the sub-band tail of the flat buffer; TCN blocks 4..7 of a branch) are
        handed to the exchange as RANGES: true only when the flat buffer really has that layout -- everything from
        sb_model.sequence_model.weight_ih_l0 to the end belongs to sb_model, and the range conv1x1.weight of block 4 ..
        sconv.bias of block 7 of a branch holds nothing but that branch's blocks 4..7.  A subclass that registers parameters
        elsewhere falls back to the single exchange in `finish` (no early bucket is announced)."""
        off = self.fp.off
        try:
            t0 = off["sb_model.sequence_model.weight_ih_l0"][0]
            if any(o >= t0 and not n.startswith("sb_model.") for n, (o, _) in off.items()):
                return False
            for br in BRANCHES:
                a = off[f"fb_model{br}.sequence_model.4.conv1x1.weight"][0]
                b, shp = off[f"fb_model{br}.sequence_model.7.sconv.bias"]
                b += int(np.prod(shp))
                pre = tuple(f"fb_model{br}.sequence_model.{i}." for i in (4, 5, 6, 7))
                if any(a <= o < b and not n.startswith(pre) for n, (o, _) in off.items()):
                    return False
        except KeyError:
            return False
        return True

    # ------------------------------------------------------------------ weights
    def p(self, name):
        return self.fp.view(name)

    def pack_weights(self, force=False):
        ver = self.fp.version()
        if not force and self.packed_version == ver:
            return
        s = H.stream()
        C, ldC, ldF = self.C, self.ldC, self.ldF
        # the 8 TCN blocks x 3 branches are equally shaped and sit at constant strides in the flat buffer: one launch each
        lay = self.fp.off["fb_model.sequence_model.1.conv1x1.weight"][0] - self.fp.off["fb_model.sequence_model.0.conv1x1.weight"][0]
        brs = self.fp.branch_stride()
        if self.packed_version is None:            # first pack: check the constant-stride assumption once
            for i in range(8):
                for z, br in enumerate(BRANCHES):
                    for leaf in ("conv1x1.weight", "sconv.weight", "conv1x1.bias", "sconv.bias", "norm1.weight", "norm1.bias",
                                 "norm2.weight", "norm2.bias", "depthwise_conv.weight", "depthwise_conv.bias", "prelu1.weight",
                                 "prelu2.weight"):
                        assert (self.fp.off[f"fb_model{br}.sequence_model.{i}.{leaf}"][0]
                                == self.fp.off[f"fb_model.sequence_model.0.{leaf}"][0] + i * lay + z * brs)
        w1, w2 = self.p("fb_model.sequence_model.0.conv1x1.weight"), self.p("fb_model.sequence_model.0.sconv.weight")

        def packed(src, dst, N, K, Npad, ldd, tr):
            H.call("nppc_pack_matrix_batched", self.prec, src, dst, N, K, Npad, ldd, tr, 8, 3, lay, brs, dst.stride(0),
                   dst.stride(1), s)

        packed(w1, self.W1p, TCN_HIDDEN, C, TCN_HIDDEN, ldC, 0)
        # sconv with norm2 folded in (csrc/tcn.hip: EPI_RESIDUAL_GN): the normalised activation is never materialised
        H.call("nppc_tcn_pack_sconv", self.prec, w2, self.p("fb_model.sequence_model.0.norm2.weight"),
               self.p("fb_model.sequence_model.0.norm2.bias"), self.p("fb_model.sequence_model.0.sconv.bias"), self.W2p, self.u2,
               self.v2, C, TCN_HIDDEN, ldC, TCN_HIDDEN, 8, 3, lay, brs, self.W2p.stride(0), self.W2p.stride(1), s)
        for z, br in enumerate(BRANCHES):
            H.call("nppc_pack_matrix", self.prec, self.p(f"fb_model{br}.fc_output_layer.weight"), self.Wfcp[z], self.F, C,
                   ldF, ldC, 0, s)
        H.call("nppc_pack_matrix", self.prec, self.p("sb_model.fc_output_layer.weight"), self.Whp, self.O, self.Hd,
               self.Opad, self.Hd, 0, s)
        if self.trainable:
            packed(w1, self.W1T, C, TCN_HIDDEN, ldC, TCN_HIDDEN, 1)
            packed(w2, self.W2T, TCN_HIDDEN, C, TCN_HIDDEN, ldC, 1)
            for z, br in enumerate(BRANCHES):
                H.call("nppc_pack_matrix", self.prec, self.p(f"fb_model{br}.fc_output_layer.weight"), self.WfcT[z], C,
                       self.F, ldC, ldF, 1, s)
            H.call("nppc_pack_matrix", self.prec, self.p("sb_model.fc_output_layer.weight"), self.WhT, self.Hd, self.O,
                   self.Hd, 32, 1, s)
            self.lstm_bwd.pack(*[self.p(LSTM_PARAMS + n) for n in ("weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1")])
        self.lstm.pack(*[self.p(LSTM_PARAMS + n) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
                                                            "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")])
        self.packed_version = ver

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B, T, train, ragged=False):
        key = (B, T, train, ragged)
        if key in self.bufs:
            return self.bufs[key]
        dev, dt = self.dev, self.dt
        Tv = T + self.la
        Tp = rup(Tv, 128)
        nblk = 8 if train else 1
        d = dict(B=B, T=T, Tv=Tv, Tp=Tp)
        d["rs"] = torch.empty(3 * self.nm, B, self.F, dtype=torch.float64, device=dev)
        d["scale"] = torch.empty(3, self.nm, B, self.F, dtype=torch.float32, device=dev)
        d["X"] = torch.zeros(9 if train else 3, 3, B, Tp, self.ldC, dtype=dt, device=dev)   # X[0] = TCN input (kept)
        d["y1"] = torch.zeros(nblk, 3, B, Tp, TCN_HIDDEN, dtype=dt, device=dev)
        d["y2"] = torch.zeros(nblk, 3, B, Tp, TCN_HIDDEN, dtype=dt, device=dev)
        d["a2"] = torch.zeros(3, B, Tp, TCN_HIDDEN, dtype=dt, device=dev)
        d["stats"] = torch.zeros(8, 2, 3, B, 2, dtype=torch.float64, device=dev)
        d["fb"] = torch.zeros(3, B, Tp, self.ldF, dtype=dt, device=dev)
        if self.nm == 2:
            d["rawmag"] = torch.zeros(B, Tp, self.ldF, dtype=dt, device=dev)
        d["sbscale"] = torch.empty(B, dtype=torch.float32, device=dev)
        d["sbwork"] = torch.zeros(2 * B, dtype=torch.float64, device=dev)     # nppc_subband_mean: sums + arrival counters
        G = self.G if (B > 1 and not ragged) else 1       # a ragged batch is B clips run alone: no drop-band
        Fo = self.F if G <= 1 else (self.F - self.F % G) // G
        d["G"], d["Fo"], d["Nseq"] = G, Fo, B * Fo
        d["x_rows"] = torch.zeros(padded_rows(Tv * B * Fo, B * Fo), self.KX, dtype=dt, device=dev)   # GEMM operand
        d["x_tm"] = rows_view(d["x_rows"], Tv, B * Fo)
        if train:
            d["tsse_saved"] = {k: torch.empty(3, self.nm, B, *shp, dtype=torch.float32, device=dev)
                               for k, shp in (("ns", ()), ("pre", (self.F, 3)), ("sq", (self.F,)),
                                              ("h1", (self.F // 2,)), ("sg", (self.F,)))}
        self.bufs[key] = d
        return d

    # ------------------------------------------------------------------ forward
    def forward(self, maps, train=False, mtile=None, frames=None):
        """maps: 3*n_maps tensors [B,1,F,T] fp32 ordered (mag, real, imag)[, (enh mag, real, imag)].
        Returns the net output [B', O, F', T] fp32 (B' in drop-band order) and keeps what backward needs.

        frames: None, or a device int32 [B] of per-item frame counts T_b <= T (ragged inference, either net): item b's
        output is the output of its first T_b frames run alone (no drop-band), frames t >= T_b of it are 0.  T comes from
        the padded input's shape: nothing is read back from the device."""
        H.require_gpu()
        assert len(maps) == 3 * self.nm
        for m in maps:
            assert m.dim() == 4, "inputs are [B, 1, F, T]"      # fullsubnet_plus.py:157
            assert m.shape[1] == 1 and m.shape[2] == self.F
        B, _, F, T = maps[0].shape
        ragged = frames is not None
        if ragged:
            if train:
                raise RuntimeError("ragged batches (frames=) are inference only: no train-mode forward")
            if not (frames.is_cuda and frames.dtype == torch.int32 and frames.shape == (B,)):
                raise ValueError(f"frames must be a device int32 tensor of shape ({B},)")
            frames = frames.contiguous()
        elif B > 1:
            assert B > self.G, f"Batch size = {B}, num_groups = {self.G}."   # feature.py:263
        self.join_side()                      # own side-stream work (re-pack of the updated weights) before anything reads it
        self.pack_weights()
        d = self._buffers(B, T, train, ragged)
        s = H.stream()
        Tp, prec, ldC, ldF = d["Tp"], self.prec, self.ldC, self.ldF
        R = B * Tp
        maps = [m.contiguous().float() for m in maps]
        d["maps"] = maps if train else None
        sv = d.get("tsse_saved")
        # 1-3: laplace norm + TSSE attention scale, transposed into the TCN input: all 3 * n_maps maps in three launches
        sv_ = [sv[k] if sv else None for k in ("ns", "pre", "sq", "h1", "sg")]
        tw = [self.p(n) for n in TSSE_PARAMS]
        tsse_w = (*tw[:6], self.ks[0], self.ks[1], self.ks[2], *tw[6:], self.sAtt)       # three convs, kernel sizes, three Linears
        if ragged:
            H.call("nppc_tsse_fwd_maps_ragged", prec, H.ptr_array(maps), 3 * self.nm, d["rs"], *tsse_w, d["scale"], d["X"][0],
                   R * ldC, frames, B, F, T, self.la, Tp, ldC, s)
        else:
            H.call("nppc_tsse_fwd_maps", prec, H.ptr_array(maps), 3 * self.nm, d["rs"], *tsse_w, d["scale"], *sv_, d["X"][0],
                   R * ldC, B, F, T, self.la, Tp, ldC, s)
        if self.nm == 2 and ragged:
            # every row of the (reused) buffer: the item's own frames, zeros from T_b on
            H.call("nppc_rawmag_stage_ragged", prec, maps[0], d["rawmag"], frames, B, F, T, Tp, ldF, s)
        elif self.nm == 2:
            H.call("nppc_scale_transpose", prec, maps[0], None, d["rawmag"], B, F, T, Tp, ldF, 0, s)
        self._fwd_fullband(d, train, frames)
        out = self._fwd_subband(d, T, train, mtile, frames)
        self.last = d
        if train:
            self._gen += 1
            d["gen"] = self._gen
            d["consumed"] = False            # the buffer dict is reused by every step of this shape
            self.last_train = d
        return out

    def _fwd_fullband(self, d, train, frames):
        """4: eight TCN blocks, the three branches batched over blockIdx.z; 5: trailing ReLU + Linear(C -> F) + ReLU"""
        s, ragged = H.stream(), frames is not None
        B, Tv, Tp, prec = d["B"], d["Tv"], d["Tp"], self.prec
        F, C, ldC, ldF, sP, R, sAct = self.F, self.C, self.ldC, self.ldF, self.sP, B * Tp, B * Tp * TCN_HIDDEN
        d["stats"].zero_()
        for i, dil in enumerate(TCN_DILATIONS):
            pre = f"fb_model.sequence_model.{i}."
            xi, xo = (i, i + 1) if train else ((0 if i == 0 else 1 + (i - 1) % 2), 1 + i % 2)
            bi = i if train else 0
            Xin, Xout = d["X"][xi], d["X"][xo]
            y1, y2 = d["y1"][bi], d["y2"][bi]
            st1, st2 = d["stats"][i, 0], d["stats"][i, 1]
            gemm_nt(prec, EPI_PRELU_STATS, A=(Xin, ldC, R * ldC), B=(self.W1p[i], ldC, TCN_HIDDEN * ldC), C=(y1, TCN_HIDDEN, sAct),
                    bias=(self.p(pre + "conv1x1.bias"), sP), slope=(self.p(pre + "prelu1.weight"), sP), stats=(st1, B * 2),
                    R=R, N=TCN_HIDDEN, K=self.KC, Tp=Tp, Tv=Tv, Nv=TCN_HIDDEN, batch=3, stream=s)
            dw = (self.p(pre + "norm1.weight"), self.p(pre + "norm1.bias"), self.p(pre + "depthwise_conv.weight"),
                  self.p(pre + "depthwise_conv.bias"), self.p(pre + "prelu2.weight"))
            if ragged:
                # GroupNorm sums of each item's own rows (replacing the uniform launch's), and the centred depthwise conv
                # stopped at each item's end: the only two places where frames past an item could reach into it
                H.call("nppc_tcn_gn_stats_ragged", prec, y1, st1, frames, self.la, B, TCN_HIDDEN, TCN_HIDDEN, Tp, Tv, sAct,
                       B * 2, 3, s)
                H.call("nppc_tcn_dwconv_ragged", prec, y1, y2, st1, *dw, frames, self.la, B, TCN_HIDDEN, TCN_HIDDEN, Tp, Tv,
                       dil, 1e-8, sAct, B * 2, sP, 3, s)
                H.call("nppc_tcn_gn_stats_ragged", prec, y2, st2, frames, self.la, B, TCN_HIDDEN, TCN_HIDDEN, Tp, Tv, sAct,
                       B * 2, 3, s)
            else:
                H.call("nppc_tcn_dwconv", prec, y1, y2, st1, st2, *dw, B, TCN_HIDDEN, TCN_HIDDEN, Tp, Tv, dil, 1e-8, sAct,
                       B * 2, sP, 3, s)
            gemm_nt_gn(prec, A=(y2, TCN_HIDDEN, sAct), B=(self.W2p[i], TCN_HIDDEN, ldC * TCN_HIDDEN), C=(Xout, ldC, R * ldC),
                       u=self.u2[i], v=self.v2[i], uv_stride=ldC, res=(Xin, ldC, R * ldC), stats=(st2, B * 2),
                       count=float(TCN_HIDDEN * Tv), eps=1e-8, R=R, N=ldC, K=TCN_HIDDEN, Tp=Tp, Tv=Tv, Nv=C, batch=3, stream=s)
        Xlast = d["X"][8 if train else 2]
        gemm_nt(prec, EPI_RELU, A=(Xlast, ldC, R * ldC), B=(self.Wfcp, ldC, ldF * ldC), C=(d["fb"], ldF, R * ldF),
                bias=(self.p("fb_model.fc_output_layer.bias"), sP), R=R, N=ldF, K=self.KC, Tp=Tp, Tv=Tv, Nv=F, relu_in=1, batch=3,
                stream=s)

    def _fwd_subband(self, d, T, train, mtile, frames):
        """6: sub-band unfold + concat + norm + drop-band, staged time-major; 7: the LSTM; 8: the output head -> the net output"""
        s, ragged = H.stream(), frames is not None
        B, Tv, Tp, prec, F, ldC, ldF, R = d["B"], d["Tv"], d["Tp"], self.prec, self.F, self.ldC, self.ldF, d["B"] * d["Tp"]
        if self.nm == 1:
            src, ldS = d["X"][0, 0], ldC          # attention-scaled, normalised magnitude (fullsubnet_plus.py:203)
        else:
            src, ldS = d["rawmag"], ldF           # RAW padded magnitude (networks.py:133)
        if ragged:
            H.call("nppc_subband_mean_ragged", prec, src, ldS, d["fb"], ldF, R * ldF, self.mult, d["sbscale"], frames, self.la,
                   B, F, Tp, Tv, self.I, s)
        else:
            H.call("nppc_subband_mean", prec, src, ldS, d["fb"], ldF, R * ldF, self.mult, d["sbscale"], d["sbwork"], B, F, Tp,
                   Tv, self.I, s)
        # mtile None: cooperative kernel when the shape allows; it also takes the output head to fuse (bf16 pair kernel)
        head = (self.Whp, self.O) if (prec == H.PREC_BF16 and self.Opad == 16) else None
        # the frozen net's fused-head inference launch reads rows of 40 columns (the same buffer, viewed narrower): the
        # staging kernel writes 37 % less, the recurrent kernel fetches 80 instead of 128 bytes per sequence and step
        plan = plan_forward(d["Nseq"], self.lstm, train, mtile, head and head[1])
        x_tm, xld = d["x_tm"], plan.x_ld
        if xld != self.KX:
            x_tm = d["x_rows"].view(-1)[:Tv * d["Nseq"] * xld].view(Tv, d["Nseq"], xld)
        H.call("nppc_subband_stage", prec, src, ldS, d["fb"], ldF, R * ldF, d["sbscale"], x_tm, B, F, Tp, Tv,
               self.nb, d["G"] if ragged else self.G, xld, int(train), s)
        # 7: two-layer LSTM over T' steps for the B*F' sequences
        if self.pre_lstm_hook is not None:
            # everything another stream still has in flight must be joined BEFORE a cooperative (CU-pair) kernel goes out:
            # its workgroups need the whole chip to themselves.  The trainer parks the previous step's deferred tail
            # (side-stream weight gradients, gradient exchange, Adam) here: it overlaps this net's small front kernels.
            hook, self.pre_lstm_hook = self.pre_lstm_hook, None
            hook()
        FSNEngine.join_all()                  # (a no-op after the trainer's hook; any other caller gets the join for free)
        lo = lstm2_forward(x_tm, self.lstm, train, head=head, plan=plan)
        d["lstm"] = lo
        # 8: Linear(H -> O) + re-layout + look-ahead crop
        out = torch.empty(B, self.O, d["Fo"], T, dtype=torch.float32, device=self.dev)
        if "head_partial" in lo:
            H.call("nppc_sb_head_finalize", lo["head_partial"], lo["head_partial"].shape[0], self.p("sb_model.fc_output_layer.bias"), out, d["Nseq"], Tv,
                   self.la, self.O, d["Fo"], s)
        else:
            H.call("nppc_sb_head", prec, lo["h2"], self.Whp, self.p("sb_model.fc_output_layer.bias"), out, d["Nseq"], Tv,
                   self.la, self.Hd, self.O, d["Fo"], s)
        if ragged:                            # the output crop: frames t >= T_b of item b are 0
            H.call("nppc_crop_frames_ragged", out, self.O * d["Fo"], T, frames, B, s)
        return out

    # ------------------------------------------------------------------ backward (direction net, trainable restorer)
    def _grad_buffer(self):
        """Flat gradient buffer that does NOT alias the parameters' current .grad (so autograd's accumulate
        semantics stay right whether or not the caller cleared the grads)."""
        first = self.fp.named[0][1]
        for k in (0, 1):
            if self.gbuf[k] is None:
                self.gbuf[k] = torch.empty_like(self.fp.flat)
            if first.grad is None or first.grad.data_ptr() != self.gbuf[k].data_ptr():
                self.fp.grad = self.gbuf[k]
                return self.gbuf[k]
        raise RuntimeError("unreachable")

    def g(self, name):
        return self.fp.gview(name)

    def _tcn_wgrad_grouped(self, d, w, G, blocks):
        """both weight gradients of TCN blocks `blocks` x the three branches, one grouped launch per kind (sconv.weight,
        conv1x1.weight): row-major operands as they are, written finished into the flat gradient (no split-K slabs, no reductions).
        The problem tables of nppc_gemm_tn_grouped are built once per set of buffers (workspaces, saved activations and both flat
        gradient buffers keep their addresses)"""
        C, ldC, R, dXL, a2L, h2L = self.C, self.ldC, d["B"] * d["Tp"], w.dXL, w.a2L, w.h2L
        key = (G.data_ptr(), d["X"].data_ptr(), a2L[0].data_ptr(), R, blocks)
        tabs = self._tn_tables.get(key)
        if tabs is None:
            sc, c1 = [], []
            for i in blocks:
                for z, br in enumerate(BRANCHES):
                    pre = f"fb_model{br}.sequence_model.{i}."
                    # dW2^T[k][c] = sum_r a2[r][k] * dXo[r][c], stored transposed: sconv.weight is [C][512]
                    sc.append((a2L[i][z], TCN_HIDDEN, dXL[i + 1][z], ldC, self.g(pre + "sconv.weight"), TCN_HIDDEN, C,
                               H.TN_STORE_TRANSPOSED))
                    # dW1[k][c] = sum_r dpre1[r][k] * Xin[r][c]: conv1x1.weight is [512][C]
                    c1.append((h2L[i][z], TCN_HIDDEN, d["X"][i][z], ldC, self.g(pre + "conv1x1.weight"), C, C, H.TN_STORE_ASIS))
            tabs = (H.tn_problem_table(sc, TCN_HIDDEN, ldC, R), H.tn_problem_table(c1, TCN_HIDDEN, ldC, R))
            self._tn_tables[key] = tabs
        for tab in tabs:
            H.call("nppc_gemm_tn_grouped", tab, tab.shape[0], TCN_HIDDEN, ldC, R, H.stream())

    def _ws(self, name, shape, dtype=None, zero=False):
        return workspace(("eng", id(self), name), shape, dtype or self.dt, self.dev, zero)

    def _wgrad(self, d, p, w, dst_name, *, A, rows, B, ncols, slab, relu_b=0):
        """full-band weight gradient where the TN GEMM does not apply: dst[z][r][c] = sum_k A[z][k][r] * B[z][k][c] for the three
        branches z, r < rows = (padded to the 128-row tile, valid), c < ncols.  A = (tensor [3][R][lda], columns, lda), B = (tensor
        [3][R][ldb], ldb): two transposes into tA / tB, the NT product into split-K fp32 slabs, their reduction"""
        s, prec, R, S = H.stream(), self.prec, d["B"] * d["Tp"], p.S2
        (a, cols_a, lda), (b, ldb), (rows, out_rows) = A, B, rows
        H.call("nppc_transpose", prec, a, w.tA, R, cols_a, lda, R, R * lda, w.sTA, 0, 3, s)
        H.call("nppc_transpose", prec, b, w.tB, R, ldb, ldb, R, R * ldb, w.sTB, relu_b, 3, s)
        gemm_nt(prec, EPI_PLAIN_F32, A=(w.tA, R, w.sTA), B=(w.tB, R, w.sTB), C=(slab, ldb, rows * ldb), R=rows, N=ldb, K=R,
                Tp=rows, Tv=rows, Nv=ldb, batch=3, ksplit=S, stream=s)
        reduce_slabs(slab, S, slab_stride=rows * ldb, ld=ldb, dst=self.g(dst_name), dst_ld=ncols, rows=out_rows, ncols=ncols,
                     batch=3, s_slab=S * rows * ldb, s_dst=self.sP, stream=s)

    def _scatter_slabs(self, slab, S, slab_stride, ld, dests, s):
        """columns [col0, col0 + ncols) of the sum of the S slabs [4H][ld] -> the LSTM parameter gradient `name`, for every
        (name, dst_ld, col0, ncols) of dests; a bias_ih_* gradient is also that of its bias_hh_* twin"""
        for name, dst_ld, col0, ncols in dests:
            reduce_slabs(slab, S, slab_stride=slab_stride, ld=ld, dst=self.g(name), dst_ld=dst_ld, rows=4 * self.Hd, col0=col0,
                         ncols=ncols, permH=self.Hd, stream=s)
            if ".bias_ih_" in name:
                self.g(name.replace(".bias_ih_", ".bias_hh_")).copy_(self.g(name))

    def _lstm_wgrad(self, dg1, dg2, x_rows, h1_rows, h2_rows, Tv, Nseq, head=None, guards=None):
        """LSTM weight / bias gradients from the row-major gate gradients (runs on the side stream).
        head = (dyt_rows [Rpad][16] bf16, O): also the output head's weight / bias gradients, as one more TN product
        h2^T . dY (the 16-column dY rows are read as a 64-column operand: the extra columns are ignored)."""
        s = H.stream()
        Hd, I, KX, Rr, q = self.Hd, self.I, self.KX, Tv * Nseq, LSTM_PARAMS
        jobs = [   # (dgates, row offset of dgates, input rows, input width, destinations (_scatter_slabs))
            (dg1, 0, x_rows, KX, [(q + "weight_ih_l0", I, 0, I), (q + "bias_ih_l0", 1, I, 1)]),
            (dg2, 0, x_rows, KX, [(q + "bias_ih_l1", 1, I, 1)]),
            (dg2, 0, h1_rows, Hd, [(q + "weight_ih_l1", Hd, 0, Hd)])]
        if Tv > 1:
            jobs += [(dg1, Nseq, h1_rows, Hd, [(q + "weight_hh_l0", Hd, 0, Hd)]),
                     (dg2, Nseq, h2_rows, Hd, [(q + "weight_hh_l1", Hd, 0, Hd)])]
        mode, fold_bias = lstm_wgrad_mode(self.prec, Hd, KX, Tv, WGRAD_SPLITS, guards is not None)
        if mode == "generic":
            return self._lstm_wgrad_generic(jobs, dg1, dg2, Rr, s)
        # 64 K-slices: (4H/128) * (H/128) * 64 = 2304 workgroups for 512 slots (16 slices = 576 left the second
        # round of workgroups 1/8 full: 481 -> 674 TFLOP/s on the H x 4H products, tools/bench_tn.py)
        S = WGRAD_SPLITS
        assert 64 * S <= ROW_PAD                 # operand buffers are padded by ROW_PAD rows (ops_lstm.padded_rows)
        slab = self._ws("slab", (S * 4 * Hd * max(Hd, KX),), torch.float32)
        if mode == "fused2":
            slab = self._lstm_wgrad_fused2(dg1, dg2, x_rows, h1_rows, guards, Rr, S, s)
        else:
            self._lstm_wgrad_tn(jobs, slab, fold_bias, Rr, S, s)
        if head is not None:
            dyt_rows, O = head
            rows = (Rr + 64 * S - 1) // (64 * S) * (64 * S)
            H.call("nppc_gemm_tn_splitk", h2_rows, Hd, dyt_rows, 16, slab, 64, Hd, 64, rows, S, s)
            reduce_slabs_t(slab, S, slab_stride=Hd * 64, ld=64, dst=self.g("sb_model.fc_output_layer.weight"), dst_ld=Hd, rows=O,
                           ncols=Hd, stream=s)
            H.colsum(self.prec, dyt_rows, self.g("sb_model.fc_output_layer.bias"), Rr, O, 16, 0, 0, 1,
                     lambda n: self._ws("cs_head", (n,), torch.float32), s)

    def _lstm_wgrad_fused2(self, dg1, dg2, x_rows, h1_rows, guards, Rr, S, s):
        """ONE pass over each layer's gate gradients for both of its weight gradients (`nppc_gemm_tn_splitk2`):
          layer 1: dg1^T . [h1_{t-1} | x_t]   (x's spare column carries the bias gradient)
          layer 2: dg2^T . [h1_t | h2_{t-1}]  (+ row sums of dg2 = the bias gradient)
        h_{t-1} is the guard view of the h rows (N zero rows in front), so the gate gradients are not shifted.  Returns its slab."""
        Hd, I, KX, K4, q = self.Hd, self.I, self.KX, 4 * self.Hd, LSTM_PARAMS
        (h1_guard, h2_guard), rows = guards, (Rr + 64 * S - 1) // (64 * S) * (64 * S)
        slab = self._ws("slab2", (S * K4 * 2 * Hd,), torch.float32)
        rsum = self._ws("rowsum", (S, K4), torch.float32)
        H.call("nppc_gemm_tn_splitk2", dg1, K4, h1_guard, Hd, Hd, x_rows, KX, KX, slab, Hd + KX, K4, rows, S, None, s)
        self._scatter_slabs(slab, S, K4 * (Hd + KX), Hd + KX, [(q + "weight_hh_l0", Hd, 0, Hd), (q + "weight_ih_l0", I, Hd, I),
                                                              (q + "bias_ih_l0", 1, Hd + I, 1)], s)
        H.call("nppc_gemm_tn_splitk2", dg2, K4, h1_rows, Hd, Hd, h2_guard, Hd, Hd, slab, 2 * Hd, K4, rows, S, rsum, s)
        self._scatter_slabs(slab, S, K4 * 2 * Hd, 2 * Hd, [(q + "weight_ih_l1", Hd, 0, Hd), (q + "weight_hh_l1", Hd, Hd, Hd)], s)
        self._scatter_slabs(rsum, S, K4, 1, [(q + "bias_ih_l1", 1, 0, 1)], s)
        return slab

    def _lstm_wgrad_tn(self, jobs, slab, fold_bias, Rr, S, s):
        """one split-K TN product per job, straight from the row-major operands.  fold_bias: the layer-2 bias gradient
        (column sums of dg2) comes out of the W_ih_l1 product as row sums of its A operand (LDS-DMA kernel, csrc/tcn.hip)
        instead of out of a 64-column product of its own that re-read all of dg2"""
        K4, q = 4 * self.Hd, LSTM_PARAMS
        for dg, off, inp, width, dests in jobs:
            rows = (Rr - off + 64 * S - 1) // (64 * S) * (64 * S)
            if fold_bias and dests[0][0] == q + "bias_ih_l1":
                continue
            if fold_bias and dests[0][0] == q + "weight_ih_l1":
                rsum = self._ws("rowsum", (S, K4), torch.float32)
                H.call("nppc_gemm_tn_splitk_rowsum", dg.view(-1)[off * K4:], K4, inp, width, slab, width, K4, width, rows, S,
                       rsum, s)
                self._scatter_slabs(rsum, S, K4, 1, [(q + "bias_ih_l1", 1, 0, 1)], s)
            else:
                H.call("nppc_gemm_tn_splitk", dg.view(-1)[off * K4:], K4, inp, width, slab, width, K4, width, rows, S, s)
            self._scatter_slabs(slab, S, K4 * width, width, dests, s)

    def _lstm_wgrad_generic(self, jobs, dg1, dg2, Rr, s):
        """fp32 parity mode, small hidden sizes: transposed copies + the NT split-K GEMM"""
        K4, KX = 4 * self.Hd, self.KX
        bk = 64 if self.prec == H.PREC_BF16 else 32
        # split-K: the products are (4H x H) outputs over T'*N rows -- 72 workgroups at C2 without it, each walking a million
        # rows (the fp32 step spent 372 of its 556 ms in these five launches, profiles/r03_bench_c2_fp32_kernel_stats.csv)
        Sg = max(1, min(64, Rr // (16 * bk)))
        Rp = rup(Rr, bk * Sg)
        K4p, Hp, KXp = rup(K4, 128), rup(self.Hd, 128), rup(KX, 128)
        dgT = [self._ws("dg1T", (K4p, Rp), zero=True), self._ws("dg2T", (K4p, Rp), zero=True)]
        for src, dst in ((dg1, dgT[0]), (dg2, dgT[1])):
            H.call("nppc_transpose", self.prec, src, dst, Rr, K4, K4, Rp, 0, 0, 0, 1, s)
        slab = self._ws("slab", (Sg * K4p * max(Hp, KXp),), torch.float32)
        for dg, off, inp, width, dests in jobs:
            wp = rup(width, 128)
            inT = self._ws(f"inT_{id(inp)}_{off}", (wp, Rp), zero=True)
            # shifted product: input row r pairs with dgates row r + off -> place it at column r + off (scalar stores)
            H.call("nppc_transpose", self.prec, inp, inT.view(-1)[off:], Rr - off, width, width, Rp, 0, 0, 0, 1, s)
            H.call("nppc_gemm_nt_splitk", self.prec, dgT[0] if dg is dg1 else dgT[1], Rp, inT, Rp, slab, wp, K4p, wp, Rp, Sg, s)
            self._scatter_slabs(slab, Sg, K4p * wp, wp, dests, s)

    def _backward_plan(self, d):
        """the BackwardPlan of buffer set d, cached with it: shapes and precision decide, and `key` (the hook; ops_lstm's backward plan takes the head)"""
        key = (self.grad_range_hook is not None and self.early_buckets_ok, plan_backward(d["Nseq"], self.lstm_bwd).head_entry is not None)
        if d.get("bwd_plan", (None,))[0] != key:
            prec, ldC, R = self.prec, self.ldC, d["B"] * d["Tp"]
            bk = 64 if prec == H.PREC_BF16 else 32
            fused = prec == H.PREC_BF16 and self.O <= 16 and key[1]
            S2 = TCN_WGRAD_SPLITS if R % (64 * TCN_WGRAD_SPLITS) == 0 else (8 if R % (32 * 8) == 0 else 1)
            tn_ok = prec == H.PREC_BF16 and TCN_HIDDEN % 128 == 0 and ldC % 64 == 0 and R % (64 * S2) == 0
            d["bwd_plan"] = (key, BackwardPlan(
                fused_head=fused, head_wgrad=fused and self.Hd % 128 == 0 and self.KX % 64 == 0, S2=S2, Fr=rup(self.F, 128),
                Cr=rup(ldC, 128), tn_ok=tn_ok, cs_ok=tn_ok and self.ldF % bk == 0 and TCN_HIDDEN % bk == 0, early=key[0]))
        return d["bwd_plan"][1]

    def backward(self, dout, gen=None):
        """dout [B', O, F', T] fp32 -> flat parameter gradient (same layout as the flat parameter buffer).

        Contract: ONE backward per train-mode forward, and it must be the latest one -- the saved activations live in
        step-persistent workspaces that the next train-mode forward of this engine overwrites.  `gen` (the generation
        number the forward returned in `last_train["gen"]`) makes a violation an error instead of a wrong gradient."""
        d = self.last_train
        if d is None or "lstm" not in d or "g1" not in d["lstm"]:
            raise RuntimeError("backward needs a forward(train=True) first")
        FSNEngine.join_all()                  # the cooperative LSTM backward wants the chip to itself
        if gen is not None and gen != d["gen"]:
            raise RuntimeError(
                f"direction-net backward for forward #{gen}, but forward #{d['gen']} has since overwritten the saved "
                "activations: this engine keeps ONE set of saved state (one backward per train-mode forward, no "
                "gradient accumulation over micro-batches); run backward before the next forward")
        if d.get("consumed"):
            raise RuntimeError("direction-net backward called twice for one forward (retain_graph / double backward are "
                               "not supported: the flat gradient buffer is overwritten, not accumulated)")
        d["consumed"] = True
        p = self._backward_plan(d)
        G = self._grad_buffer()
        G.zero_()
        dx, dg1, dg2, head = self._bwd_head_lstm(d, p, dout)
        self._bwd_lstm_wgrad(d, p, G, dg1, dg2, head)
        dpre_fb, Dsb = self._bwd_staging(d, dx)
        w = self._bwd_workspaces(d, p)
        self._bwd_fc(d, p, w, dpre_fb)
        dX0 = self._bwd_tcn(d, p, w, G)
        self._bwd_tsse(d, dX0, dx, Dsb)
        self._bwd_fc_wgrad_join(d, p, w, dpre_fb)
        return G

    def _on_side(self, fn):
        """run fn (which launches on the current stream) on the side stream once the current stream got here"""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            fn()

    def _bwd_head_lstm(self, d, p, dout):
        """1. head: dh2 = dY Wh, dWh, dbh; LSTM recurrence backward.  Returns dx, the gate gradients of both layers and the
        `head` operand of _lstm_wgrad (None: the head's parameter gradients are done here)"""
        s = H.stream()
        lo, Nseq, Fo, Tv, Hd, O = d["lstm"], d["Nseq"], d["Fo"], d["Tv"], self.Hd, self.O
        gW, gb = self.g("sb_model.fc_output_layer.weight"), self.g("sb_model.fc_output_layer.bias")
        if not p.fused_head:
            dh2 = self._ws("dh2", (Tv, Nseq, Hd))
            H.call("nppc_sb_head_bwd", self.prec, dout, self.WhT, lo["h2"], dh2, gW, gb, Nseq, Tv, self.la, Hd, O, Fo, s)
            return (*lstm2_backward(lo, dh2, self.lstm_bwd, self.KX), None)
        dyt_rows = self._ws("dyt_rows", (padded_rows(Tv * Nseq) + 8, 16), zero=True)   # dY rows, zero padded like the GEMM operands
        dyt = rows_view(dyt_rows, Tv, Nseq)
        H.call("nppc_head_dy_gather", dout, dyt, Nseq, Tv, self.la, O, Fo, s)
        if not p.head_wgrad:
            H.call("nppc_sb_head_bwd_w", self.prec, dout, lo["h2"], gW, gb, Nseq, Tv, self.la, Hd, O, Fo, s)
        return (*lstm2_backward(lo, None, self.lstm_bwd, self.KX, head=(dyt, self.WhT)), (dyt_rows, O) if p.head_wgrad else None)

    def _bwd_lstm_wgrad(self, d, p, G, dg1, dg2, head):
        """2. LSTM weight gradients: dW[k][c] = sum_rows dgates[row][k] * input[row][c], rows = (t, sequence).  Row-major operands
        straight from the recurrent kernels; h_{t-1} is the same buffer one time block (Nseq rows) earlier; the staged input carries
        a ones column (index I), so its product column is the bias gradient.  They only feed the flat gradient, so they run on a side
        stream beside the full-band backward chain (dozens of small kernels that leave most CUs idle); joined at the end of backward."""
        lo = d["lstm"]
        if self._side is None:
            # lowest priority: the dependent chain on the main stream is what the step waits for; the weight-gradient
            # GEMMs are throughput work
            prio = max(torch.cuda.Stream.priority_range()) if hasattr(torch.cuda.Stream, "priority_range") else 0
            self._side = torch.cuda.Stream(device=self.dev, priority=prio)
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            self._lstm_wgrad(dg1, dg2, d["x_rows"], lo["h1_rows"], lo["h2_rows"], d["Tv"], d["Nseq"], head=head,
                             guards=(lo["h1_guard"], lo["h2_guard"]) if "h1_guard" in lo else None)
            if p.early:
                # the sub-band segment (LSTM + head: the tail of the flat buffer) is final once these GEMMs are done
                self.grad_range_hook(G, self.fp.off[LSTM_PARAMS + "weight_ih_l0"][0], G.numel())

    def _bwd_staging(self, d, dx):
        """3. sub-band staging backward -> gradient of the pre-ReLU full-band outputs (and the per-item sums Dsb)"""
        B, Tp, ldF = d["B"], d["Tp"], self.ldF
        dpre_fb = self._ws("dpre_fb", (3, B, Tp, ldF), zero=True)
        Dsb = self._ws("Dsb", (B,), torch.float64)
        H.call("nppc_subband_stage_bwd", self.prec, dx, d["x_tm"], d["fb"], d["sbscale"], Dsb, dpre_fb, B, self.F, Tp, d["Tv"], ldF,
               B * Tp * ldF, self.nb, self.G, self.KX, H.stream())
        return dpre_fb, Dsb

    def _bwd_workspaces(self, d, p):
        """the buffers that more than one stage of the full-band backward (4, 5, 7) touches, as the plan asks for them"""
        B, Tp, ldC, R, ws = d["B"], d["Tp"], self.ldC, d["B"] * d["Tp"], self._ws
        w = SimpleNamespace(slab2=None)
        w.tA = ws("tA", (3, max(p.Cr, TCN_HIDDEN, p.Fr), R), zero=True)       # transposed dY operand
        w.tB = ws("tB", (3, max(ldC, TCN_HIDDEN), R), zero=True)              # transposed activation operand
        w.sTA, w.sTB = w.tA.shape[1] * R, w.tB.shape[1] * R
        h2b = ws("h2b", (3, B, Tp, TCN_HIDDEN))
        # block i reads its upstream gradient dXL[i + 1] and writes dXL[i]; a2L[i] = GN2(y2), h2L[i] = gradient of its conv1x1 output
        if p.tn_ok:      # read by the side stream later: one buffer per TCN block, so the main chain never waits for it inside a step
            w.dXL = [ws(f"dX_{i}", (3, B, Tp, ldC)) for i in range(9)]
            w.a2L = [ws(f"a2_{i}", (3, B, Tp, TCN_HIDDEN), zero=True) for i in range(8)]
            w.h2L = [ws(f"h2b_{i}", (3, B, Tp, TCN_HIDDEN)) for i in range(8)]
        else:
            w.slab2 = ws("slab2", (3 * p.S2 * max(p.Cr * TCN_HIDDEN, TCN_HIDDEN * ldC, p.Fr * ldC),), torch.float32)
            dXa, dXb = ws("dXa", (3, B, Tp, ldC)), ws("dXb", (3, B, Tp, ldC))
            w.dXL = [dXb if i % 2 else dXa for i in range(9)]                 # everything is consumed in line: two buffers take turns
            w.a2L, w.h2L = [d["a2"]] * 8, [h2b] * 8
        # column sums per 128-row tile from the producing GEMMs' epilogues, per TCN block: the fused middle backward adds them up
        w.cpL = list(ws("colpart", (8, 3, R // 128, ldC), torch.float32)) if p.cs_ok else [None] * 8
        return w

    def _fc_wgrad(self, d, p, w, dpre_fb, slab):
        """fc_output_layer parameter gradients (bias: column sums; weight: two transposes + the NT split-K product -- F and C
        are not multiples of the TN kernel's tiles)"""
        F, ldF, R = self.F, self.ldF, d["B"] * d["Tp"]
        H.colsum(self.prec, dpre_fb, self.g("fb_model.fc_output_layer.bias"), R, F, ldF, R * ldF, self.sP, 3,
                 lambda n: self._ws("cs_fc", (n,), torch.float32), H.stream())
        self._wgrad(d, p, w, "fb_model.fc_output_layer.weight", A=(dpre_fb, F, ldF), rows=(p.Fr, F), B=(d["X"][8], self.ldC),
                    ncols=self.C, slab=slab, relu_b=1)

    def _bwd_fc(self, d, p, w, dpre_fb):
        """4. fc_output_layer backward -> dXL[8], the upstream gradient of TCN block 7"""
        ldC, ldF, R = self.ldC, self.ldF, d["B"] * d["Tp"]
        if not p.tn_ok:
            self._fc_wgrad(d, p, w, dpre_fb, w.slab2)     # tA / tB / slab2 are re-used by the TCN blocks: the product stays in line
        gemm_nt(self.prec, EPI_MASK_POS, A=(dpre_fb, ldF, R * ldF), B=(self.WfcT, ldF, ldC * ldF), C=(w.dXL[8], ldC, R * ldC),
                res=(d["X"][8], ldC, R * ldC), R=R, N=ldC, K=ldF, Tp=d["Tp"], Tv=d["Tv"], Nv=self.C, batch=3, colpart=w.cpL[7],
                stream=H.stream())

    def _tcn_mid_finish(self, d, p, w, Pmid, lo, hi):
        """finishing pass of the fused middle backwards of blocks lo .. hi-1: their partial rows summed into the parameter gradients"""
        pre, ldC, R = f"fb_model.sequence_model.{lo}.", self.ldC, d["B"] * d["Tp"]
        lay = self.fp.off["fb_model.sequence_model.1.conv1x1.weight"][0] - self.fp.off["fb_model.sequence_model.0.conv1x1.weight"][0]
        H.call("nppc_tcn_mid_bwd_finish", Pmid[lo], Pmid.shape[1], w.cpL[lo], 3 * (R // 128) * ldC, R // 128, ldC, self.C,
               *[self.g(pre + n) for n in TCN_MID_GRADS], self.g(pre + "sconv.bias") if p.cs_ok else None,
               d["B"], TCN_HIDDEN, self.sP, lay, 3, hi - lo, H.stream())

    def _tcn_wgrad_parity(self, d, p, w, i):
        """the two weight gradients of TCN block i where the TN GEMM does not apply (fp32 parity mode, row counts no multiple of
        64 * S2), in line on the main stream: sconv.weight [C][512] from (dXo, a2), conv1x1.weight [512][C] from (dpre1, Xin)"""
        C, ldC, pre = self.C, self.ldC, f"fb_model.sequence_model.{i}."
        self._wgrad(d, p, w, pre + "sconv.weight", A=(w.dXL[i + 1], ldC, ldC), rows=(p.Cr, C), B=(w.a2L[i], TCN_HIDDEN),
                    ncols=TCN_HIDDEN, slab=w.slab2)
        self._wgrad(d, p, w, pre + "conv1x1.weight", A=(w.h2L[i], TCN_HIDDEN, TCN_HIDDEN), rows=(TCN_HIDDEN, TCN_HIDDEN),
                    B=(d["X"][i], ldC), ncols=C, slab=w.slab2)

    def _announce_blocks_7_4(self, G):
        for br in BRANCHES:
            a = self.fp.off[f"fb_model{br}.sequence_model.4.conv1x1.weight"][0]
            b, shp = self.fp.off[f"fb_model{br}.sequence_model.7.sconv.bias"]
            self.grad_range_hook(G, a, b + int(np.prod(shp)))

    def _bwd_tcn(self, d, p, w, G):
        """5. TCN blocks in reverse -> dXL[0], the gradient of the TCN input X[0]"""
        s, prec, B, Tp, Tv, C, ldC, sP = H.stream(), self.prec, d["B"], d["Tp"], d["Tv"], self.C, self.ldC, self.sP
        R, sAct = B * Tp, B * Tp * TCN_HIDDEN
        h1b =self._ws("h1b", (3, B, Tp, TCN_HIDDEN))
        Smid = self._ws("Smid", (3, B, TCN_HIDDEN // 64, 8), torch.float64)      # channel-group shares of the per-sample sums
        # partial rows of the fused middle backward, one set per TCN block: their finishing pass (sum over the samples into the
        # parameter gradients) runs as ONE launch for all eight blocks behind the loop -- or as two (blocks 7..4, then 3..0) when the
        # data-parallel exchange sends blocks 7..4 early.  Eight 5-us launches each waited up to 0.5 ms for CUs beside the
        # weight-gradient GEMMs of the side queue (profiles/r03_bench_c2_bf16_windows.txt)
        Pmid = self._ws("Pmid", (8, H.mid_bwd_part_elems(B, TCN_HIDDEN, Tp, 3)), torch.float32)
        for i in range(7, -1, -1):
            pre = f"fb_model.sequence_model.{i}."
            dXo, dXi, a2, h2b = w.dXL[i + 1], w.dXL[i], w.a2L[i], w.h2L[i]
            if not p.cs_ok:                   # no column sums from the producing GEMM: a pass over dXo for the sconv bias gradient
                H.colsum(prec, dXo, self.g(pre + "sconv.bias"), R, C, ldC, R * ldC, sP, 3,
                         lambda n: self._ws("cs_sconv", (n,), torch.float32), s)
            # dA2 = dXo W2  (gradient of the normalised depthwise output)
            gemm_nt(prec, EPI_PLAIN, A=(dXo, ldC, R * ldC), B=(self.W2T[i], ldC, TCN_HIDDEN * ldC), C=(h1b, TCN_HIDDEN, sAct),
                    R=R, N=TCN_HIDDEN, K=ldC, Tp=Tp, Tv=Tv, Nv=TCN_HIDDEN, batch=3, stream=s)
            # GroupNorm-2, PReLU-2, depthwise conv, GroupNorm-1, PReLU-1 backward in one reduce + one apply pass: h1b -> h2b
            # (= gradient of the conv1x1 output) with every parameter gradient of those stages and the conv1x1 bias gradient;
            # the reduce pass also leaves a2 = GN2(y2), the operand of the sconv weight gradient
            H.call("nppc_tcn_mid_bwd", prec, h1b, d["y2"][i], d["y1"][i], d["stats"][i, 0], d["stats"][i, 1], Smid, Pmid[i],
                   self.p(pre + "norm1.weight"), self.p(pre + "norm1.bias"), self.p(pre + "norm2.weight"), self.p(pre + "norm2.bias"),
                   self.p(pre + "depthwise_conv.weight"), self.p(pre + "prelu1.weight"), self.p(pre + "prelu2.weight"), a2, h2b,
                   *[self.g(pre + n) for n in TCN_MID_GRADS], w.cpL[i], R // 128, ldC, C, self.g(pre + "sconv.bias") if p.cs_ok else None,
                   B, TCN_HIDDEN, Tp, Tv, TCN_DILATIONS[i], 1e-8, sAct, B * 2, sP, 3, 0, s)
            if i == 4 and p.early:
                self._tcn_mid_finish(d, p, w, Pmid, 4, 8)     # blocks 7..4 are handed to the exchange below: their gradients must be final
            # sconv weight gradient dW2[c][k] = sum_r dXo[r][c] * a2[r][k] and conv1x1 weight gradient dW1[k][c] = sum_r
            # dpre1[r][k] * Xin[r][c] (the conv1x1 bias gradient came out of the fused kernel)
            if not p.tn_ok:
                self._tcn_wgrad_parity(d, p, w, i)
            elif i == 0 or (i == 4 and p.early):
                # all blocks x branches of a kind in ONE grouped launch on the side queue, issued once the main chain has produced the
                # operands of the last block of the group -- block 0, or block 4 and then block 0 when blocks 7..4 leave early
                blocks = tuple(range(3 if p.early and i == 0 else 7, i - 1, -1))
                self._on_side(lambda: self._tcn_wgrad_grouped(d, w, G, blocks))
            # conv1x1 input gradient + the residual path; its column sums are block i-1's sconv bias gradient
            gemm_nt(prec, EPI_RESIDUAL, A=(h2b, TCN_HIDDEN, sAct), B=(self.W1T[i], TCN_HIDDEN, ldC * TCN_HIDDEN), C=(dXi, ldC, R * ldC),
                    res=(dXo, ldC, R * ldC), R=R, N=ldC, K=TCN_HIDDEN, Tp=Tp, Tv=Tv, Nv=C, batch=3,
                    colpart=w.cpL[i - 1] if i > 0 else None, stream=s)
            if i == 4 and p.early:            # TCN blocks 7..4 of every branch are final once both queues have passed this point
                self._on_side(lambda: self._announce_blocks_7_4(G))
        self._tcn_mid_finish(d, p, w, Pmid, 0, 4 if p.early else 8)
        return w.dXL[0]

    def _bwd_tsse(self, d, dX0, dx, Dsb):
        """6. TSSE attention backward (parameter gradients only: the maps are data)"""
        s, B, T, Tp, F, ldC = H.stream(), d["B"], d["T"], d["Tp"], self.F, self.ldC
        if self.nm == 1:
            # the restorer's sub-band rows unfold the attention-scaled magnitude X[0][0] (fullsubnet_plus.py:200-204), a
            # trainable tensor: the gradient of those columns joins the TCN-input gradient of branch 0 (the direction net
            # unfolds the raw magnitude, a constant: nothing to add there)
            H.call("nppc_subband_unfold_bwd", self.prec, dx, d["sbscale"], Dsb, self.mult, dX0[0], ldC, B, F, Tp, d["Tv"], self.nb,
                   self.G, self.KX, s)
        sv = d["tsse_saved"]
        n_ws = ctypes.c_long()
        H.call("nppc_tsse_bwd_ws_elems", 3 * self.nm, B, F, self.ks[0], self.ks[1], self.ks[2], ctypes.byref(n_ws))
        dsg = self._ws("dsg", (n_ws.value,), torch.float32)      # per map: dsg | da2 | da1 | per-sample contributions (csrc/spec.hip)
        wts = [self.p(n) for n in TSSE_PARAMS if n.endswith(".weight")]      # the weights of the three convs, the three Linears
        H.call("nppc_tsse_bwd_maps", self.prec, dX0, B * Tp * ldC, H.ptr_array(d["maps"]), 3 * self.nm, d["rs"], *wts[:3],
               self.ks[0], self.ks[1], self.ks[2], *wts[3:], self.sAtt, sv["ns"], sv["pre"], sv["sq"], sv["h1"], sv["sg"], dsg,
               *[self.g(n) for n in TSSE_PARAMS], B, F, T, self.la, Tp, ldC, s)

    def _bwd_fc_wgrad_join(self, d, p, w, dpre_fb):
        """7. the deferred fc_output_layer weight gradient, and the join of the weight-gradient stream"""
        if p.tn_ok:
            # bf16: the product waits until the END of the main chain -- the side queue (LSTM + TCN weight gradients) is the longer
            # one, the main queue would idle in front of the join -- with a slab of its own
            self._fc_wgrad(d, p, w, dpre_fb, self._ws("slab_fc", (3 * p.S2 * p.Fr * self.ldC,), torch.float32))
        if self.defer_join:
            self.join_pending = True          # joined (join_side) before anything reads the gradient
            FSNEngine._unjoined[id(self)] = self
        else:
            torch.cuda.current_stream().wait_stream(self._side)       # join the weight-gradient stream

    def side_stream(self):
        return self._side

    def prepack_on_side(self):
        """re-pack the (just updated) weights on the side stream behind everything the current stream has been given so far;
        the caller joins (join_side) before the packed copies are used and before the next cooperative LSTM launch"""
        self._on_side(self.pack_weights)
        self.join_pending = True
        FSNEngine._unjoined[id(self)] = self

    def join_side(self):
        """make the current stream wait for this engine's side-stream work (weight gradients of the last backward in
        defer_join mode, re-packed weights); idempotent"""
        if self.join_pending:
            torch.cuda.current_stream().wait_stream(self._side)
            self.join_pending = False
            FSNEngine._unjoined.pop(id(self), None)

    @staticmethod
    def join_all():
        """make the current stream wait for the side-stream work of EVERY engine (before a cooperative LSTM launch)"""
        for e in list(FSNEngine._unjoined.values()):
            e.join_side()
