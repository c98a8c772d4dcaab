"""Launch sequence of the inpainting U-Net on the HIP kernels of csrc/unet.hip (no torch compute ops).

Mirrors UNet.forward (nppc_audio/inpainting/networks/unet.py:277-290) block by block on haloed NHWC
activations: one `UNetEngine` owns the packed weights, the activation / gradient buffers of every
resolution level and the launch order of forward and backward.  The frozen restorer runs with its
BatchNorm folded into the convolution epilogue (eval mode); the direction U-Net runs in train mode
(batch statistics, running-buffer update) and keeps what its backward needs; so does the restorer while it is
trained (InpaintingTrainer), with its nn.Dropout layers active in the differentiated pass.

Every per-convolution decision is a field of its `ConvPlan` (made once, in __init__); an activation travels as a `_View`
(tensor, ld) that is split only in the line that builds a launch's argument list.
"""

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _hip as H
from .engine import FlatParams, rup

LEAK = 0.2
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# (block, path of the double_conv inside it, in channels (None = net input), out channels, level)
PLAN = (("inc", "conv.conv", None, 64, 0), ("down1", "mpconv.1.conv", 64, 128, 1), ("down2", "mpconv.1.conv", 128, 256, 2),
        ("down3", "mpconv.1.conv", 256, 512, 3), ("down4", "mpconv.1.conv", 512, 512, 4), ("up1", "conv.conv", 1024, 256, 3),
        ("up2", "conv.conv", 512, 128, 2), ("up3", "conv.conv", 256, 64, 1), ("up4", "conv.conv", 128, 64, 0))
N_DOWN = 5          # PLAN[:N_DOWN] is the encoder; an up block reads the block before it in PLAN and the skip of its own level
IN_LD = 64          # the 1- or 2-channel net input is staged into a 64-wide zero-padded pixel row
OUT_LD = 64         # so is the K-channel output of the 1x1 convolution
DROP_BLOCKS = ("down3", "down4", "up1", "up2")    # double_convs that end in nn.Dropout (unet.py:254-257)


PROFILE = None      # bench hook: list of (kind, algorithmic flops, start event, end event)


class _timed:
    """records a HIP-event pair on the current stream around the launches inside the block (bench only)"""

    def __init__(self, kind, flops):
        self.kind, self.flops = kind, flops

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if PROFILE is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROFILE.append((self.kind, self.flops, self.e0, e1))


class ConvPlan(NamedTuple):
    """what is decided about one convolution, once (UNetEngine.__init__); forward and backward read the same fields"""
    name: str             # parameter prefix: <name>.weight, <name>.bias
    bn: Optional[str]     # prefix of the BatchNorm behind it (None: outc.conv)
    cin: int
    cout: int
    ks: int
    cinp: int             # K of the forward GEMM: the input row width (a multiple of 32)
    np_: int              # N of the forward GEMM
    kind: str             # "thin3" / "thin1": direct kernels on the fp32 parameter tensor (csrc/unet.hip); "tiled": implicit GEMM
    needs_wb: bool        # the input gradient runs on the tiled kernel: keep the transposed pack
    flops_per_pixel: int

    @classmethod
    def make(cls, name, bn, cin, cout, ks, trainable):
        if ks == 3 and cin <= 2 and cout <= 64 and cout % 8 == 0:
            kind = "thin3"    # first layer: memory-bound, 18 MACs per output
        elif ks == 1 and cin == 64 and cout <= 8:
            kind = "thin1"
        else:
            kind = "tiled"
        return cls(name, bn, cin, cout, ks, IN_LD if cin < 32 else cin, rup(cout, 64), kind,
                   trainable and not name.startswith("inc.conv.conv.0"), 2 * cin * cout * ks * ks)


class _View(NamedTuple):
    """an activation operand: pixel rows of `ld` elements from t[0] on -- a haloed NHWC matrix or a channel slice of one"""
    t: torch.Tensor
    ld: int

    @classmethod
    def haloed(cls, rows, ld, guard_before, guard_after, dtype, device):
        """[rows][ld] inside a zeroed allocation with guard rows on both sides"""
        store = torch.zeros((guard_before + rows + guard_after) * ld, dtype=dtype, device=device)
        return cls(store[guard_before * ld:], ld)

    def at(self, coff):
        return _View(self.t[coff:], self.ld)


class SavedBlock(NamedTuple):
    """what the backward of one double_conv reads"""
    x: _View
    raw_a: _View
    act_a: _View
    raw_b: _View
    out: _View
    ss_a: torch.Tensor
    ss_b: torch.Tensor
    level: int


class SavedPass(NamedTuple):
    blocks: dict                   # block -> SavedBlock
    pools: dict                    # level -> arg-max bytes of the pooling into it
    u4: _View
    mask: torch.Tensor
    drop: Optional[tuple]          # (p, seed, pass_id) of the pass's nn.Dropout layers


_NO_VIEW = (None, 0)


def conv_fwd(prec, *, A, Wp, C, bias=None, fold=None, B, hw, Cin, Cout, Np, ks, stream):
    """C = conv(A, Wp) (+ bias) (`nppc_conv_fwd`): Cin = the row width of A the pack consumes, Cout = output channels stored,
    Np = N of the pack.  fold = (scale, shift): eval-mode BatchNorm + LeakyReLU in the epilogue.  A, C: views."""
    H.call("nppc_conv_fwd", prec, *A, Wp, *C, bias, *(fold or (None, None)), LEAK, B, *hw, Cin, Cout, Np, ks, stream)


def bn_bwd(prec, *, dyA, dyB=None, Y, X, ss, S, dX, dgamma, dbeta, C, B, hw, drop=None, stream):
    """backward of LeakyReLU(BatchNorm(X)) = Y for the gradient dyA (+ dyB) (`nppc_bn_bwd`); drop = (p, seed, Philox stream):
    Y went through nn.Dropout in place, whose keep bits the kernel regenerates (`nppc_bn_bwd_dropout`).  dy*, Y, X, dX: views."""
    front = (prec, *dyA, *(dyB or _NO_VIEW), *Y, *X, ss, S, *dX, dgamma, dbeta, C, B, *hw, LEAK)
    if drop is None:
        H.call("nppc_bn_bwd", *front, stream)
    else:
        H.call("nppc_bn_bwd_dropout", *front, *drop, stream)


class UNetEngine:
    def __init__(self, module, in_ch, out_ch, prec, trainable):
        H.require_gpu()
        self.mod = module
        self.prec = prec
        self.dtype = H.dtype_of(prec)
        self.in_ch, self.out_ch = in_ch, out_ch
        self.trainable = trainable
        self.dev = next(module.parameters()).device
        self.fp = FlatParams(module, self.dev)
        self.bufs = {}
        self.scratch = {}
        self.geo = None
        self._packed_version = None
        self._gsel = 0
        self._gbufs = [None, None]
        self.blocks = {}                     # block -> the plans of its two 3x3 convolutions
        for blk, path, cin, cout, _ in PLAN:
            cin = in_ch if cin is None else cin
            self.blocks[blk] = (ConvPlan.make(f"{blk}.{path}.0", f"{blk}.{path}.1", cin, cout, 3, trainable),
                                ConvPlan.make(f"{blk}.{path}.3", f"{blk}.{path}.4", cout, cout, 3, trainable))
        self.head = ConvPlan.make("outc.conv", None, PLAN[-1][3], out_ch, 1, trainable)
        self.convs = [c for pair in self.blocks.values() for c in pair] + [self.head]     # forward order
        self.wf, self.wb = {}, {}
        self._buffers = dict(module.named_buffers())

    # ------------------------------------------------------------------------------------------ parameters
    def p(self, name):
        return self.fp.view(name)

    def g(self, name):
        return self._grad.narrow(0, self.fp.off[name][0], int(np.prod(self.fp.off[name][1])))

    def bnbuf(self, name):
        return self._buffers[name]

    def pack_weights(self, train):
        """fp32 parameters -> packed bf16/f32 GEMM operands (forward: [Np][taps*Cinp], input-gradient:
        [Cinp][taps*Np]).  Re-done whenever a parameter or BatchNorm buffer was written since the last pack."""
        ver = (self.fp.version(), sum(b._version for b in self._buffers.values()), bool(train))
        if self._packed_version == ver:
            return
        s = H.stream()
        for c in self.convs:
            nt = c.ks * c.ks
            if c.name not in self.wf:
                self.wf[c.name] = torch.empty(c.np_ * nt * c.cinp, dtype=self.dtype, device=self.dev)
                self.wb[c.name] = torch.empty(c.cinp * nt * c.np_, dtype=self.dtype, device=self.dev) if c.needs_wb else None
            H.call("nppc_conv_pack", self.prec, self.p(c.name + ".weight"), self.wf[c.name], self.wb[c.name], c.cout, c.cin, c.ks,
                   c.np_, c.cinp, c.cinp, c.np_, s)
        if not train:
            # eval-mode BatchNorm folds into a per-channel scale / shift applied in the convolution epilogue
            self.ss = {}
            for c in self.convs[:-1]:
                ss = torch.empty(4 * c.cout, dtype=torch.float32, device=self.dev)
                H.call("nppc_bn_finalize", None, self.p(c.bn + ".weight"), self.p(c.bn + ".bias"), self.bnbuf(c.bn + ".running_mean"),
                       self.bnbuf(c.bn + ".running_var"), ss, c.cout, 1.0, BN_EPS, BN_MOMENTUM, 0, s)
                self.ss[c.name] = ss
        self._packed_version = ver

    # ------------------------------------------------------------------------------------------ buffers
    def _setup(self, B, F, T):
        if self.geo == (B, F, T):
            return
        self.geo = (B, F, T)
        self.bufs = {}
        self.scratch = {}
        self.lv = []
        h, w = F, T
        for _ in range(5):
            if h < 1 or w < 1:
                raise ValueError(f"spectrogram {F}x{T} is too small for four 2x2 poolings")
            self.lv.append((h, w))
            h, w = h // 2, w // 2
        self.P = [B * (h + 2) * (w + 2) for h, w in self.lv]
        self.ksplit = [int(min(64, max(1, p // 1024))) for p in self.P]   # 64 slices x 9 taps already fill the chip; more only costs reduction traffic
        self.ksplit = [k // 8 * 8 if k >= 8 else k for k in self.ksplit]     # multiples of 8: XCD-aware tile order
        self.st = torch.zeros(2 * 1024, dtype=torch.float64, device=self.dev)

    def buf(self, tag, level, ld):
        """the haloed activation / gradient matrix `tag` of a level, as a view"""
        key = (tag, level, ld)
        b = self.bufs.get(key)
        if b is None:
            h, w = self.lv[level]
            gb = w + 3 + 1
            ga = 64 * self.ksplit[level] + 128 + w + 4
            b = self.bufs[key] = _View.haloed(self.P[level], ld, gb, ga, self.dtype, self.dev)
        return b

    def _scratch(self, name, n, dtype):
        """the scratch buffer `name` with room for n elements, grown on demand.  Every name has a buffer of its own (kernels of
        one step read several at once): "slabs" split-K weight-gradient partials, "thin_part" partials of the thin weight
        gradients, "statpart" per-tile column sums of a convolution's output, "statscr" their fp64 reduction, "idx" pooling
        arg-max bytes nobody reads (eval), "pool_idx<level>" those the backward reads"""
        t = self.scratch.get(name)
        if t is None or t.numel() < n:
            t = self.scratch[name] = torch.empty(n, dtype=dtype, device=self.dev)
        return t

    def _timed(self, kind, c, level):
        h, w = self.lv[level]
        return _timed(kind, float(self.geo[0] * h * w * c.flops_per_pixel))

    # ------------------------------------------------------------------------------------------ forward
    def _conv(self, c, x, y, level, fold, stats=False):
        """stats=True (train-mode BatchNorm follows): returns the per-tile column sums of the stored output when the tiled kernel
        runs (they replace the statistics pass over the tensor), else None"""
        B = self.geo[0]
        h, w = self.lv[level]
        if c.ks == 3 and c.cinp != x.ld:
            raise RuntimeError(f"{c.name}: input row width {x.ld} != packed K {c.cinp}")
        bias = self.p(c.name + ".bias")
        ss = self.ss[c.name] if fold else None
        with self._timed("conv_fwd", c, level):
            if (stats and not fold and c.kind == "tiled" and c.ks == 3
                    and c.cinp % (64 if self.prec == H.PREC_BF16 else 32) == 0):
                ntiles = (self.P[level] + 127) // 128
                part = self._scratch("statpart", max(ntiles * 2 * c.np_, (self.P[0] + 127) // 128 * 2 * 128), torch.float32)
                H.call("nppc_conv_fwd_stats", self.prec, *x, self.wf[c.name], *y, bias, B, h, w, c.cinp, c.cout, c.np_, c.ks, part,
                       H.stream())
                return (part, c.np_)
            if c.kind == "thin3":
                H.call("nppc_conv3x3_thin_fwd", self.prec, *x, self.p(c.name + ".weight"), bias, ss, ss[c.cout:] if fold else None,
                       LEAK, *y, B, h, w, c.cin, c.cout, H.stream())
            elif c.kind == "thin1" and not fold:
                H.call("nppc_conv1x1_thin_fwd", self.prec, *x, self.p(c.name + ".weight"), bias, *y, B, h, w, c.cin, c.cout,
                       H.stream())
            else:
                conv_fwd(self.prec, A=x, Wp=self.wf[c.name], C=y, bias=bias, fold=(ss, ss[c.cout:]) if fold else None, B=B,
                         hw=(h, w), Cin=c.cinp, Cout=c.cout, Np=c.np_, ks=c.ks, stream=H.stream())

    def _bn_train(self, c, raw, y, level, parts=None):
        """batch statistics -> scale/shift (+ running update) -> LeakyReLU, output possibly a channel slice.
        parts: (per-tile column sums left by the convolution's epilogue, their row width) or None (a pass over `raw`)"""
        B = self.geo[0]
        h, w = self.lv[level]
        s = H.stream()
        st = self.st[:2 * c.cout]
        if parts is not None:
            H.call("nppc_bn_stats_from_parts", parts[0], B, h, w, parts[1], c.cout, st,
                   self._scratch("statscr", 2 * 1024 * 128, torch.float64), s)
        else:
            st.zero_()
            H.call("nppc_bn_stats", self.prec, *raw, self.P[level], c.cout, st, s)
        ss = torch.empty(4 * c.cout, dtype=torch.float32, device=self.dev)
        H.call("nppc_bn_finalize", st, self.p(c.bn + ".weight"), self.p(c.bn + ".bias"), self.bnbuf(c.bn + ".running_mean"),
               self.bnbuf(c.bn + ".running_var"), ss, c.cout, float(B * h * w), BN_EPS, BN_MOMENTUM, 1, s)
        self.bnbuf(c.bn + ".num_batches_tracked").add_(1)
        H.call("nppc_bn_act", self.prec, *raw, *y, ss, c.cout, B, h, w, LEAK, s)
        return ss

    def _double_conv(self, blk, level, x, out, train, saved):
        """(conv3x3 -> BatchNorm -> LeakyReLU) x 2 (tmp_utils.py:8-37); `out` may be a channel slice of a concat buffer"""
        ca, cb = self.blocks[blk]
        if not train:
            mid = self.buf("act_a", level, ca.cout)
            self._conv(ca, x, mid, level, True)
            self._conv(cb, mid, out, level, True)
            return
        raw_a, act_a, raw_b = (self.buf(f"{blk}.{tag}", level, ca.cout) for tag in ("raw_a", "act_a", "raw_b"))
        ss_a = self._bn_train(ca, raw_a, act_a, level, self._conv(ca, x, raw_a, level, False, stats=True))
        ss_b = self._bn_train(cb, raw_b, out, level, self._conv(cb, act_a, raw_b, level, False, stats=True))
        saved[blk] = SavedBlock(x, raw_a, act_a, raw_b, out, ss_a, ss_b, level)

    @staticmethod
    def _drop_stream(pass_id, blk):
        """Philox stream of block `blk` in stochastic pass `pass_id` (shared by the forward and the fused backward)"""
        return int(pass_id) * len(DROP_BLOCKS) + DROP_BLOCKS.index(blk)

    def _dropout(self, blk, x, cout, level, dropout):
        """nn.Dropout at the end of the block's double_conv (tmp_utils.py:28-29), in place.  In a train-mode pass the
        backward regenerates the same keep bits (nppc_bn_bwd_dropout): nothing is stored for it"""
        if not dropout or blk not in DROP_BLOCKS:
            return
        keep = None
        if dropout.get("tap") is not None:
            keep = torch.empty(self.P[level] * cout, dtype=torch.uint8, device=self.dev)
            dropout["tap"][blk] = (keep, level, cout)
        H.call("nppc_dropout", self.prec, *x, self.P[level], cout, float(dropout["p"]), int(dropout["seed"]),
               self._drop_stream(dropout["pass_id"], blk), keep, H.stream())

    def forward(self, shape, maps, map_bstride, mask, out, out_pstride, xin=None, xin_bstride=0, train=False, dropout=None):
        """dropout: None or dict(p, seed, pass_id[, tap]) -- MC-dropout passes (utils.py:334-338, 561-577) and the
        restorer's training passes (restoration_trainer.py: nn.Dropout(0.2) in train mode, differentiated).
        maps: list of fp32 tensors holding [B][F*T] planes with batch stride `map_bstride` (the net's input
        channels); mask [B,T] fp32.  Writes out[(b*K+k)*out_pstride + f*T + t]:
          xin is None : U-Net(maps) * (1 - mask)                      (pc_wrapper.py:77-83)
          xin given   : xin * mask + U-Net(maps) * (1 - mask)         (RestorationWrapper, unet.py:299-312)"""
        B, F, T = shape
        self._setup(B, F, T)
        self.pack_weights(train)
        s = H.stream()
        x = self.buf("in", 0, IN_LD)
        for c, m in enumerate(maps):
            H.call("nppc_unet_stage_map", self.prec, m, map_bstride, *x, c, B, F, T, s)
        saved = {} if train else None
        cat = {0: self.buf("cat", 0, 128), 1: self.buf("cat", 1, 256), 2: self.buf("cat", 2, 512), 3: self.buf("cat", 3, 1024)}
        pools = {}
        for blk, _, _, cout, level in PLAN[:N_DOWN]:
            cin = self.blocks[blk][0].cin
            if level > 0:
                ph, pw = self.lv[level - 1]
                pooled = self.buf("pool", level, cin)
                if train:
                    idx = pools[level] = self._scratch(f"pool_idx{level}", self.P[level] * cin, torch.uint8)
                else:
                    idx = self._scratch("idx", self.P[level] * cin, torch.uint8)
                H.call("nppc_maxpool2", self.prec, *x, *pooled, idx, cin, B, ph, pw, s)
                x = pooled
            y = cat[level] if level < 4 else self.buf("x5", 4, cout)     # a skip goes to channels [0, cout) of the concat buffer
            self._double_conv(blk, level, x, y, train, saved)
            self._dropout(blk, y, cout, level, dropout)
            x = y
        for i in range(N_DOWN, len(PLAN)):
            blk, _, cin, cout, level = PLAN[i]
            prev_c, prev_level = PLAN[i - 1][3:]
            hi, wi = self.lv[prev_level]
            ht, wt = self.lv[level]
            H.call("nppc_upsample2", self.prec, *x, *cat[level].at(cin - prev_c), prev_c, B, hi, wi, ht, wt, s)
            u = self.buf(blk + ".out", level, cout)
            self._double_conv(blk, level, cat[level], u, train, saved)
            self._dropout(blk, u, cout, level, dropout)
            x = u
        raw_o = self.buf("raw_o", 0, OUT_LD)
        self._conv(self.head, x, raw_o, 0, False)
        H.call("nppc_unet_out", self.prec, *raw_o, mask, xin, xin_bstride, out, out_pstride, self.out_ch, B, F, T,
               0 if xin is None else 1, s)
        if train:
            drop = (float(dropout["p"]), int(dropout["seed"]), int(dropout["pass_id"])) if dropout else None
            self.saved = SavedPass(saved, pools, x, mask, drop)

    # ------------------------------------------------------------------------------------------ backward
    def _grad_buffer(self):
        """two flat gradient buffers used alternately, so a gradient still referenced by the caller (or by a
        parameter's .grad) is never overwritten by the next backward"""
        self._gsel ^= 1
        if self._gbufs[self._gsel] is None:
            self._gbufs[self._gsel] = torch.zeros_like(self.fp.flat)
        self._grad = self._gbufs[self._gsel]
        self.fp.grad = self._grad
        return self._grad

    def _wgrad(self, c, dy, x, level):
        """dW[co][ci][tap] = sum_p dY[p][co] * X[p + off(tap)][ci]"""
        B = self.geo[0]
        h, w = self.lv[level]
        M, N = dy.ld, x.ld
        S = self.ksplit[level]
        s = H.stream()
        with self._timed("conv_wgrad", c, level):
            if c.kind != "tiled":
                part = self.scratch.get("thin_part")
                if part is None:                     # the library is asked for the size once
                    part = self._scratch("thin_part", H.conv_thin_part_elems(), torch.float32)
                H.call("nppc_conv3x3_thin_wgrad" if c.kind == "thin3" else "nppc_conv1x1_thin_wgrad", self.prec, *dy, *x, part,
                       self.g(c.name + ".weight"), B, h, w, c.cin, c.cout, s)
                return
            slabs = self._scratch("slabs", c.ks * c.ks * S * rup(M, 128) * N, torch.float32)
            H.call("nppc_conv_wgrad", self.prec, *dy, *x, slabs, M, N, B, h, w, c.ks, S, s)
            H.call("nppc_conv_wgrad_reduce", self.prec, slabs, S, M, N, self.g(c.name + ".weight"), c.cout, c.cin, c.ks, s)

    def _conv_bwd_data(self, c, dy, dx, level):
        """dX = transposed convolution of dY: the forward kernel on the flipped / transposed pack"""
        B = self.geo[0]
        h, w = self.lv[level]
        with self._timed("conv_bwd_data", c, level):
            if c.kind == "thin1":
                H.call("nppc_conv1x1_thin_bwd_data", self.prec, *dy, self.p(c.name + ".weight"), *dx, B, h, w, c.cin, c.cout,
                       H.stream())
            else:
                conv_fwd(self.prec, A=dy, Wp=self.wb[c.name], C=dx, B=B, hw=(h, w), Cin=c.np_, Cout=c.cin, Np=c.cinp, ks=c.ks,
                         stream=H.stream())

    def _double_conv_bwd(self, blk, dyA, dyB, need_dx):
        """gradient dyA (+ dyB, or None) of the block's output -> parameter gradients; returns the gradient of its input
        (need_dx) or None"""
        sv = self.saved.blocks[blk]
        ca, cb = self.blocks[blk]
        level, cout = sv.level, ca.cout
        common = dict(S=self.st[:2 * cout], C=cout, B=self.geo[0], hw=self.lv[level], stream=H.stream())
        draw = self.buf("draw", level, cout)
        drop = self.saved.drop
        if drop is not None and blk in DROP_BLOCKS:
            # the block output went through nn.Dropout in place: its keep bits are regenerated inside the BatchNorm backward
            p, seed, pass_id = drop
            drop = (p, seed, self._drop_stream(pass_id, blk))
        else:
            drop = None
        bn_bwd(self.prec, dyA=dyA, dyB=dyB, Y=sv.out, X=sv.raw_b, ss=sv.ss_b, dX=draw, dgamma=self.g(cb.bn + ".weight"),
               dbeta=self.g(cb.bn + ".bias"), drop=drop, **common)
        self._wgrad(cb, draw, sv.act_a, level)
        dact = self.buf("dact", level, cout)
        self._conv_bwd_data(cb, draw, dact, level)
        bn_bwd(self.prec, dyA=dact, Y=sv.act_a, X=sv.raw_a, ss=sv.ss_a, dX=draw, dgamma=self.g(ca.bn + ".weight"),
               dbeta=self.g(ca.bn + ".bias"), **common)
        self._wgrad(ca, draw, sv.x, level)
        # the bias of a convolution that feeds a BatchNorm has an exactly zero gradient (the batch mean absorbs it);
        # the flat gradient buffer is zeroed at the start of backward, so nothing to write
        if not need_dx:
            return None
        dx = self.buf("dx", level, sv.x.ld)
        self._conv_bwd_data(ca, draw, dx, level)
        return dx

    def backward(self, dout, dout_pstride):
        """dout: gradient wrt the masked output, planes [(b*K+k)*dout_pstride + f*T + t] -> flat parameter gradient"""
        B, F, T = self.geo
        s = H.stream()
        grad = self._grad_buffer()
        grad.zero_()
        K = self.out_ch
        d_rawo = self.buf("d_rawo", 0, OUT_LD)
        H.call("nppc_unet_out_bwd", self.prec, dout, dout_pstride, self.saved.mask, *d_rawo, K, B, F, T, s)
        bias_acc = torch.zeros(OUT_LD, dtype=torch.float32, device=self.dev)
        H.colsum(self.prec, d_rawo.t, bias_acc, self.P[0], OUT_LD, OUT_LD, 0, 0, 1,
                 lambda n: torch.empty(n, dtype=torch.float32, device=self.dev), s)
        self.g("outc.conv.bias").copy_(bias_acc[:K])
        self._wgrad(self.head, d_rawo, self.saved.u4, 0)
        dy = self.buf("d_u", 0, self.head.cin)
        self._conv_bwd_data(self.head, d_rawo, dy, 0)
        skips = {}
        for i in range(len(PLAN) - 1, N_DOWN - 1, -1):
            blk, _, cin, _, level = PLAN[i]
            prev_c, prev_level = PLAN[i - 1][3:]
            dcat = self._double_conv_bwd(blk, dy, None, True)              # [P_level][cin]
            skips[level] = dcat                                            # channels [0, cin - prev_c): gradient of the skip
            hi, wi = self.lv[prev_level]
            ht, wt = self.lv[level]
            dy = self.buf("d_up", prev_level, prev_c)
            H.call("nppc_upsample2_bwd", self.prec, *dcat.at(cin - prev_c), *dy, prev_c, B, hi, wi, ht, wt, s)
        # encoder, deepest first: gradient = (upsample / pooling branch) + (skip branch); dy is d x5 here
        dskip = None
        for blk, _, _, _, level in reversed(PLAN[:N_DOWN]):
            cin = self.blocks[blk][0].cin
            dx = self._double_conv_bwd(blk, dy, dskip, level > 0)          # the first layer needs no input gradient
            if level == 0:
                break
            ph, pw = self.lv[level - 1]
            dy = self.buf("d_pool", level - 1, cin)
            H.call("nppc_maxpool2_bwd", self.prec, *dx, self.saved.pools[level], *dy, cin, B, ph, pw, s)
            dskip = skips[level - 1]
        return grad
