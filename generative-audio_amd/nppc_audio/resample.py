"""torchaudio's default resampler (Hann-windowed sinc, `torchaudio.transforms.Resample(orig_freq, new_freq)`) for ragged
batches, on the device (csrc/resample.hip; specification tests/resample_ref.py).

Both of the reference's datasets resample with it (dataset/audio_dataset.py:85-88, dataset/audio_dataset_inpainting.py:
140-146).  With orig / new the two rates reduced by their gcd:

    base  = min(orig, new) * rolloff            width = ceil(lowpass_filter_width * orig / base)         Klen = 2 width + orig
    t     = clamp((-p / new + (k - width) / orig) * base, -lpw, lpw)           p in [0, new), k in [0, Klen)
    kern[p][k] = (base / orig) sinc(pi t) cos(pi t / (2 lpw))^2                in fp64, cast to fp32
    y[i new + p] = sum_k xpad[i orig + k] kern[p][k]                           xpad = width zeros, x, width + orig zeros

cut to ceil(new len / orig) outputs.  Every clamped tap is exactly 0.0f after the cast and the others are one contiguous run
per phase, so the device table holds (k0, count, taps) per phase: 23.7 KB where the full 160 x 475 bank is 304 KB.  `support`
and `map_gap` read that table to say which outputs depend on which inputs; RecordingRestorer uses them to restore a
recording at its own rate (inpainting/restore.py).

The hot path is the HIP kernel.  backend="host" is the same formula as torch.nn.functional.conv1d with the full bank on the
CPU, for machines without a device and for the CPU tests; it is chosen explicitly or by "auto" when there is no device,
never because a kernel is missing.
"""
import ctypes
import math
from typing import NamedTuple

import torch

from . import _hip as H

__all__ = ["resample", "Resample", "sinc_table", "support", "map_gap", "out_length", "SincTable", "TILES"]

TILES = (1024, 512, 256, 128, 64)        # outputs per workgroup, the largest whose LDS fits is taken


class SincTable(NamedTuple):
    orig: int            # reduced rates
    new: int
    width: int
    klen: int
    k0: torch.Tensor     # [new] int64: first live tap of each phase
    count: torch.Tensor  # [new] int64: how many
    maxcount: int
    stride: int          # words per row of `packed`
    packed: torch.Tensor  # [new, stride] int32 (host): k0, count, the taps' bits, zeros
    tile: int            # outputs per workgroup the kernel runs this ratio with (0: the table does not fit)
    lds_bytes: int
    lowpass_filter_width: int
    rolloff: float


def _reduced(orig_freq, new_freq):
    if isinstance(orig_freq, bool) or isinstance(new_freq, bool) or int(orig_freq) != orig_freq or int(new_freq) != new_freq:
        raise ValueError(f"orig_freq {orig_freq!r}, new_freq {new_freq!r}: the rates are integers")
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"orig_freq {orig_freq}, new_freq {new_freq}: the rates are positive")
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def out_length(n, orig_freq, new_freq):
    """ceil(new n / orig): how many samples `n` samples at orig_freq become"""
    orig, new = _reduced(orig_freq, new_freq)
    return -(-new * int(n) // orig)


def _full_bank(orig, new, lowpass_filter_width, rolloff):
    """-> (kern [new, Klen] fp64, clamped [new, Klen] bool, width): torchaudio's _get_sinc_resample_kernel, Hann"""
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = t * base
    clamped = (t <= -lowpass_filter_width) | (t >= lowpass_filter_width)
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base / orig
    kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * scale
    return kern, clamped, width


_TABLES = {}


def sinc_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann"):
    """The compressed bank of a ratio (cached): SincTable.  No GPU.  ValueError for rates that are not positive integers,
    for any method but the Hann one (the Kaiser window's clamped taps are not zero) and for a lowpass_filter_width below 1."""
    if resampling_method != "sinc_interp_hann":
        raise ValueError(f"resampling_method = {resampling_method!r}: only 'sinc_interp_hann' is built")
    orig, new = _reduced(orig_freq, new_freq)
    if int(lowpass_filter_width) != lowpass_filter_width or lowpass_filter_width < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"lowpass_filter_width {lowpass_filter_width!r}, rolloff {rolloff!r}: want an integer >= 1 and "
                         "a rolloff in (0, 1]")
    key = (orig, new, int(lowpass_filter_width), float(rolloff))
    if key in _TABLES:
        return _TABLES[key]
    width = math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))
    klen = 2 * width + orig
    if not shape(orig, new, width, 1, TILES[-1])["fits"]:
        # even one tap per phase and the smallest tile are too much: say so without building a bank of new x Klen doubles
        none = torch.zeros(0, dtype=torch.int64)
        tab = SincTable(orig, new, width, klen, none, none, 0, 3, torch.zeros(0, 3, dtype=torch.int32), 0, 0,
                        int(lowpass_filter_width), float(rolloff))
        _TABLES[key] = tab
        return tab
    kern, _, width = _full_bank(orig, new, int(lowpass_filter_width), float(rolloff))
    k32 = kern.float()
    nz = k32 != 0
    ar = torch.arange(klen)
    k0 = torch.where(nz, ar, klen).min(1).values
    k1 = torch.where(nz, ar, -1).max(1).values + 1
    count = (k1 - k0).clamp(min=0)
    k0 = torch.where(count > 0, k0, torch.zeros_like(k0))
    maxcount = max(int(count.max()), 1)
    stride = (2 + maxcount) | 1
    packed = torch.zeros(new, stride, dtype=torch.int32)
    packed[:, 0], packed[:, 1] = k0.int(), count.int()
    cols = k0[:, None] + torch.arange(maxcount)[None]
    live = torch.arange(maxcount)[None] < count[:, None]
    taps = torch.where(live, k32.gather(1, cols.clamp(max=klen - 1)), torch.zeros(()))
    packed[:, 2:2 + maxcount] = taps.view(torch.int32)
    tile, lds = 0, 0
    for cand in TILES:
        sh = shape(orig, new, width, maxcount, cand)
        if sh["fits"]:
            tile, lds = cand, sh["lds_bytes"]
            break
    tab = SincTable(orig, new, width, klen, k0, count, maxcount, stride, packed, tile, lds, int(lowpass_filter_width),
                    float(rolloff))
    _TABLES[key] = tab
    return tab


def shape(orig, new, width, maxcount, tile):
    """nppc_resample_sinc_shape (host only): {'stride', 'table_bytes', 'span_elems', 'lds_bytes', 'fits'}"""
    st, fits = H.c_i(), H.c_i()
    tb, sp, lds = H.c_l(), H.c_l(), H.c_l()
    H.call("nppc_resample_sinc_shape", int(orig), int(new), int(width), int(maxcount), int(tile), ctypes.byref(st),
           ctypes.byref(tb), ctypes.byref(sp), ctypes.byref(lds), ctypes.byref(fits))
    return {"stride": st.value, "table_bytes": tb.value, "span_elems": sp.value, "lds_bytes": lds.value,
            "fits": bool(fits.value)}


def support(j, table):
    """the half-open range of input samples that the live taps of output j = i new + p touch:
    [i orig - width + k0[p], + count[p]) (it may reach below 0 or past the input: zeros there)"""
    i, p = divmod(int(j), table.new)
    a = i * table.orig - table.width + int(table.k0[p])
    return a, a + int(table.count[p])


def map_gap(s, e, table, out_len=None):
    """the smallest [a, b) of outputs that contains every output whose support meets the inputs [s, e), clipped to
    [0, out_len) when out_len is given.  Outputs outside [a, b) do not depend on the samples of [s, e) at all.  An empty
    result (nothing inside the clip meets the gap) is (a, a)."""
    s, e = int(s), int(e)
    if e <= s:
        raise ValueError(f"gap ({s}, {e}) is empty")
    t = table
    i_lo = max((s + t.width - t.klen) // t.orig, 0)
    i_hi = max((e + t.width) // t.orig + 1, i_lo)
    i = torch.arange(i_lo, i_hi + 1, dtype=torch.int64)[:, None]
    lo = i * t.orig - t.width + t.k0[None]
    hi = lo + t.count[None]
    j = i * t.new + torch.arange(t.new, dtype=torch.int64)[None]
    meets = (hi > s) & (lo < e) & (t.count[None] > 0)
    if out_len is not None:
        meets &= j < int(out_len)
    if not bool(meets.any()):
        a = int(j.min()) if out_len is None else min(int(j.min()), int(out_len))
        return a, a
    hit = j[meets]
    return int(hit.min()), int(hit.max()) + 1


def _host_bank(table):
    """the full fp32 bank [new, 1, Klen] scattered back from the compressed rows"""
    bank = torch.zeros(table.new, table.klen, dtype=torch.float32)
    taps = table.packed[:, 2:2 + table.maxcount].contiguous().view(torch.float32)
    cols = table.k0[:, None] + torch.arange(table.maxcount)[None]
    live = torch.arange(table.maxcount)[None] < table.count[:, None]
    bank[torch.arange(table.new)[:, None].expand_as(cols)[live], cols[live]] = taps[live]
    return bank[:, None]


def _host_one(x, table, bank):
    """x [L] fp32 (host) -> [ceil(new L / orig)]: F.pad, F.conv1d with stride orig, transpose, cut (torchaudio's
    _apply_sinc_resample_kernel)"""
    n = x.numel()
    target = -(-table.new * n // table.orig)
    if n == 0:
        return x.new_zeros(0)
    xp = torch.nn.functional.pad(x[None, None], (table.width, table.width + table.orig))
    y = torch.nn.functional.conv1d(xp, bank, stride=table.orig)          # [1, new, frames]
    return y.transpose(1, 2).reshape(-1)[:target].contiguous()


def _unsupported(table, orig_freq, new_freq):
    return ValueError(f"resampling {orig_freq} -> {new_freq} reduces to {table.orig}/{table.new}: a table of {table.new} "
                      f"phases and an input span of {table.klen} samples or more do not fit the kernel's LDS budget")


def _resample_table(x, table, lengths, backend, freqs=None):
    if backend not in ("auto", "host", "hip"):
        raise ValueError(f"backend = {backend!r}: 'auto', 'hip' or 'host'")
    if x.dim() not in (1, 2):
        raise ValueError(f"x {tuple(x.shape)}: want [L] or [B, L]")
    if lengths is not None and x.dim() != 2:
        raise ValueError("lengths go with a batch [B, L]")
    if table.tile == 0:
        raise _unsupported(table, *(freqs or (table.orig, table.new)))
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "host"
    x2 = x if x.dim() == 2 else x[None]
    B, Lx = x2.shape
    if lengths is None:
        lens = [Lx] * B
    else:
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(lens) != B or any(v < 0 or v > Lx for v in lens):
            raise ValueError(f"lengths {lens} do not fit x {tuple(x2.shape)}")
    outs = [-(-table.new * v // table.orig) for v in lens]
    max_out = max(outs) if outs else 0
    if backend == "host":
        xh = x2.detach().cpu().float()
        bank = _host_bank(table)
        y = torch.zeros(B, max_out, dtype=torch.float32)
        for b in range(B):
            y[b, :outs[b]] = _host_one(xh[b, :lens[b]], table, bank)
    else:
        H.require_gpu()
        xd = x2.detach()
        if not xd.is_cuda:
            xd = xd.cuda()
        xd = xd.float()
        if xd.stride(1) != 1 or (B > 1 and (xd.stride(0) < Lx or (lengths is None and xd.stride(0) != Lx))):
            xd = xd.contiguous()                        # rows of a wider buffer are taken as they are when lengths say so
        y = torch.empty(B, max_out, dtype=torch.float32, device=xd.device)
        if B and max_out:
            lens_d = None if lengths is None else torch.tensor(lens, dtype=torch.int64).to(xd.device)
            tab_d = _device_table(table, xd.device)
            for b0 in range(0, B, 65535):
                nb = min(65535, B - b0)
                H.call("nppc_resample_sinc", H.c_p(xd[b0:].data_ptr()), Lx if B == 1 else xd.stride(0),
                       None if lens_d is None else H.c_p(lens_d[b0:].data_ptr()), nb, tab_d, table.orig, table.new,
                       table.width, table.maxcount, table.tile, H.c_p(y[b0:].data_ptr()), max_out, H.stream())
    if lengths is not None:
        return y, torch.tensor(outs, dtype=torch.int64)
    return y if x.dim() == 2 else y[0]


_DEVICE_TABLES = {}


def _device_table(table, device):
    """the packed table on `device`, uploaded once per ratio and device"""
    key = (table.orig, table.new, table.lowpass_filter_width, table.rolloff, str(device))
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = table.packed.to(device)
    return _DEVICE_TABLES[key]


def resample(x, orig_freq, new_freq, lengths=None, backend="auto", lowpass_filter_width=6, rolloff=0.99,
             resampling_method="sinc_interp_hann"):
    """x [L] or [B, L] fp32 at orig_freq -> at new_freq, as torchaudio.functional.resample does at its defaults.
      lengths (list or int64 tensor [B]; a device tensor costs one host read): the batch is ragged, item b has lengths[b]
      samples and what x holds past them is never read -> (y [B, max_out], out_lengths [B] int64 on the host), y zero
      past each item's ceil(new len / orig) samples.
      backend: 'hip' (one launch per batch; the result is on the device, a host input is uploaded), 'host' (F.conv1d with
      the full bank on the CPU, item by item), 'auto' = 'hip' when there is a device.
    Equal rates return x itself (and the lengths given), with no launch.  ValueError before any launch: rates that are not
    positive integers, a method other than the Hann one, a reduced ratio whose table does not fit the kernel's LDS budget
    (16000 -> 44101, say), lengths that do not fit x."""
    table = sinc_table(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method)
    if table.orig == table.new:
        if lengths is None:
            return x
        return x, torch.as_tensor(lengths, dtype=torch.int64).cpu()
    return _resample_table(x, table, lengths, backend, freqs=(orig_freq, new_freq))


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) at its defaults: forward(waveform [..., L]) -> [..., L']; the
    compressed table is built at construction and uploaded once per device (_device_table)"""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6,
                 rolloff=0.99, backend="auto"):
        super().__init__()
        self.orig_freq, self.new_freq, self.backend = int(orig_freq), int(new_freq), backend
        self.table = sinc_table(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method)
        if self.table.orig != self.table.new and self.table.tile == 0:
            raise _unsupported(self.table, orig_freq, new_freq)

    def forward(self, waveform, lengths=None):
        if self.table.orig == self.table.new:
            return waveform if lengths is None else (waveform, torch.as_tensor(lengths, dtype=torch.int64).cpu())
        lead = waveform.shape[:-1]
        x = waveform.reshape(-1, waveform.shape[-1]) if waveform.dim() != 2 else waveform
        out = _resample_table(x, self.table, lengths, self.backend, (self.orig_freq, self.new_freq))
        if lengths is not None:
            return out
        return out.reshape(*lead, out.shape[-1])
