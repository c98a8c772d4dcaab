"""Curve sheets (f0 contours over frames) drawn and written as PNG (csrc/curve_core.h + csrc/curve_png.hip, DESIGN.md
section 8m; specification tests/curve_ref.py).

`values` [N, T] float32 holds one curve per row, NaN where a frame has no point (pYIN's unvoiced frames).  A `CurveSheet`
stacks `Panel`s over the frames [t0, t1) of one item's window (`windows` int32 [N_items, 4]: t0, t1, marker 0, marker 1 in
curve frames, the layout of spectrogram_png.windows_from_mask; default the whole clip without markers).  A `Panel` draws its
`Curve`s, later ones over earlier ones, inside a one-pixel axes box with grid lines at `yticks` and every `xtick_every`
frames, tick labels in a 5 x 7 bitmap font (0-9 . - and the space) and a legend column of (colour, text) entries.  The
drawing rule is integer arithmetic on fp32-quantised rows, stated once in csrc/curve_core.h: the device, the serial host
renderer and the restatement give the same pixels.

`render_png(values, sheets)` goes from the contours to PNG bytes in one device call (three launches to draw, then the
encoder of png.py); backend "host" draws with the serial renderer and encodes on the host pool.  Not drawn: anti-aliasing,
line alpha (paint order stands in), titles, axis names, letters, log axes.  No pixel parity with matplotlib is claimed.
"""
import ctypes
import math
import os
import struct
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip as H
from . import png

FONT = "0123456789.- "            # glyph codes 0..12 (curve_font_row of csrc/curve_core.h)
LDS_ROWS = 16384                  # CURVE_LDS_ROWS: curves of a panel x (window + 2)
MAX_PANELS, MAX_CHARS, MAX_WIDTH, MAX_SX, MAX_GLYPH_SCALE = 64, 16, 5, 64, 8
INK, GRID, MARKER, BACKGROUND = 250, 251, 254, 255
NAN = float("nan")
# what the measurement of tools/bench_curve_png.py says about backend="auto" of render_png (profiles/curve_png_bench.json)
AUTO_IS_DEVICE = True


def plot_palette(grid=(204, 204, 204), marker=(255, 0, 0), background=(255, 255, 255)):
    """256 x 3 uint8: 0..249 viridis (png.py's table at rint(i 253 / 249)), 250 black (reference curve, box, glyphs), 251 the
    grid grey, 252 and 253 background, 254 the marker, 255 the background"""
    vir = png.palette("viridis")[:254]
    out = np.empty((256, 3), np.uint8)
    out[:250] = vir[np.rint(np.arange(250) * 253.0 / 249.0).astype(np.int64)]
    out[250], out[251], out[252], out[253], out[254], out[255] = (0, 0, 0), grid, background, background, marker, background
    return out


def alpha_colours(A):
    """palette indices of A variations: rint(linspace(0, 249, A)), for the reference's viridis(linspace(0, 1, A))"""
    return [int(v) for v in np.rint(np.linspace(0.0, 249.0, int(A)))]


def label(v):
    """a tick value as the font can write it: two decimals at most, trailing zeros dropped"""
    s = f"{float(v):.2f}".rstrip("0").rstrip(".")
    return "0" if s in ("-0", "") else s


@dataclass
class Curve:
    row: int                          # row of values
    colour: int                       # palette index
    width: int = 1                    # 1..5 pixels

    def __post_init__(self):
        if not 1 <= self.width <= MAX_WIDTH or not 0 <= self.colour <= 255 or self.row < 0:
            raise ValueError(f"a curve has a row >= 0, a colour in 0..255 and a width in 1..{MAX_WIDTH}")


@dataclass
class Panel:
    curves: Sequence[Curve]
    ymin: float = NAN                 # both NaN: autoscale to the finite values of the panel's curves inside the window
    ymax: float = NAN
    yticks: Sequence[float] = ()
    xtick_every: Optional[int] = None     # frames between vertical grid lines (and x labels), counted from frame 0 of the clip
    x_unit: float = 1.0               # an x label reads label(t * x_unit)
    markers: bool = False
    legend: Sequence[Tuple[int, str]] = ()

    def __post_init__(self):
        auto = math.isnan(self.ymin) and math.isnan(self.ymax)
        if not auto and not self.ymax > self.ymin:
            raise ValueError("a panel's range is ymin < ymax, or both NaN")
        if self.xtick_every is not None and int(self.xtick_every) < 1:
            raise ValueError("xtick_every is a positive number of frames, or None")
        for _, text in self.legend:
            _codes(text)


@dataclass
class CurveSheet:
    item: int
    panels: Sequence[Panel]
    sx: int = 1
    plot_height: int = 64
    glyph_scale: int = 1
    n_panels: int = field(init=False, default=0)

    def __post_init__(self):
        self.n_panels = len(self.panels)
        if not 1 <= self.n_panels <= MAX_PANELS:
            raise ValueError(f"a sheet stacks 1..{MAX_PANELS} panels")
        if not (1 <= self.sx <= MAX_SX and 1 <= self.plot_height <= png.MAX_DIM and 1 <= self.glyph_scale <= MAX_GLYPH_SCALE):
            raise ValueError(f"sx in 1..{MAX_SX}, plot_height in 1..{png.MAX_DIM}, glyph_scale in 1..{MAX_GLYPH_SCALE}")


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _codes(text):
    if len(text) > MAX_CHARS or any(ch not in FONT for ch in text):
        raise ValueError(f"a label is at most {MAX_CHARS} characters of {FONT!r}; got {text!r}")
    packed = [0, 0]
    for k, ch in enumerate(text):
        packed[k // 8] |= FONT.index(ch) << (4 * (k % 8))
    return [p - (1 << 32) if p >= 1 << 31 else p for p in packed]


def _tables(sheets, N, T):
    """the four int32 tables of include/nppc_hip.h"""
    sheet, panel, curve, stamp = [], [], [], []
    for s in sheets:
        sheet.append((s.item, len(panel), s.n_panels, s.sx, s.plot_height, s.glyph_scale, 0, 0))
        for p in s.panels:
            auto = math.isnan(p.ymin) and math.isnan(p.ymax)
            ymin, scale = (0.0, 0.0) if auto else (float(np.float32(p.ymin)), float(np.float32(s.plot_height / (p.ymax - p.ymin))))
            first_curve, first_stamp = len(curve), len(stamp)
            for c in p.curves:
                if not 0 <= c.row < N:
                    raise ValueError(f"curve row {c.row} of {N}")
                curve.append((c.row, c.colour, c.width, 0))
            for v in p.yticks:
                text = label(v)
                stamp.append((0, _bits(float(np.float32(v))), 0, len(text), *_codes(text), 0, 0))
            every = int(p.xtick_every) if p.xtick_every is not None else 0
            if every:
                for t in range(0, T, every):
                    text = label(t * p.x_unit)
                    stamp.append((1, t, 0, len(text), *_codes(text), 0, 0))
            for n, (colour, text) in enumerate(p.legend):
                if not 0 <= int(colour) <= 255:
                    raise ValueError("a legend colour is a palette index")
                stamp.append((2, n, int(colour), len(text), *_codes(text), 0, 0))
            panel.append((first_curve, len(p.curves), int(auto) | 2 * int(p.markers), _bits(ymin), _bits(scale), first_stamp,
                          len(stamp) - first_stamp, every))
    arr = lambda rows, w: np.ascontiguousarray(np.array(rows, np.int64).astype(np.int32).reshape(-1, w))
    return arr(sheet, 8), arr(panel, 8), arr(curve, 4), arr(stamp, 8)


def shape(tabs, N, T, i, frames):
    """(W, H, left margin, right margin, plot width, most curves of a panel) of sheet i at a window of `frames` frames:
    nppc_curve_shape, the layout function the renderers run"""
    sheet, panel, curve, stamp = tabs
    W, Hh, m = ctypes.c_long(), ctypes.c_long(), (ctypes.c_int * 4)()
    H.call("nppc_curve_shape", sheet.ctypes.data, len(sheet), panel.ctypes.data, len(panel), curve.ctypes.data or None, len(curve),
           stamp.ctypes.data if len(stamp) else None, len(stamp), N, T, i, frames, ctypes.byref(W), ctypes.byref(Hh), m)
    return (W.value, Hh.value, *m)


def _prepare(values, sheets, windows, max_frames):
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2 or min(values.shape) < 1:
        raise ValueError("values is a float32 tensor [N, T]")
    N, T = values.shape
    sheets = list(sheets)
    if not sheets:
        raise ValueError("render: no sheet")
    if windows is None:
        n_items = max(s.item for s in sheets) + 1
        windows = torch.tensor([[0, T, -1, -1]] * n_items, dtype=torch.int32)
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 4:
        raise ValueError("windows is an int32 tensor [N_items, 4]")
    n_items = windows.shape[0]
    for s in sheets:
        if not 0 <= s.item < n_items:
            raise ValueError(f"item {s.item} of {n_items}")
    frames = T if max_frames is None else max(1, min(int(max_frames), T))
    for s in sheets:
        most = max(len(p.curves) for p in s.panels)
        if most * (frames + 2) > LDS_ROWS:
            raise ValueError(f"render: {most} curves over a window of up to {frames} frames; curves x (window + 2) may not exceed "
                             f"{LDS_ROWS}, the rows a workgroup stages in LDS")
    tabs = _tables(sheets, N, T)
    dims = []
    for i in range(len(sheets)):
        try:
            w, h = shape(tabs, N, T, i, frames)[:2]
        except RuntimeError:
            raise ValueError(f"render: sheet {i} is wider or higher than {png.MAX_DIM} pixels or has more than 2^26") from None
        dims.append((w, h))
    allow = np.array([w * h for w, h in dims], np.int64)
    off = np.concatenate([[0], np.cumsum((allow + 3) & ~3)])                      # every image starts a 32-bit word
    meta = np.zeros((len(sheets), 4), np.int64)
    meta[:, 0], meta[:, 3] = off[:-1], allow
    return dict(values=values.contiguous(), N=N, T=T, tabs=tabs, win=windows.contiguous(), n_items=n_items, dims=dims, meta=meta,
                total=int(off[-1]), nimg=len(sheets), max_panels=max(s.n_panels for s in sheets))


def _check_fit(meta, what):
    if (meta[:, 1] < 1).any():
        raise ValueError(f"{what}: sheet {int(np.flatnonzero(meta[:, 1] < 1)[0])} has an empty window, or one wider than max_frames")


def _on_device(backend, values):
    if backend not in ("auto", "hip", "host"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'host', got {backend!r}")
    if backend == "hip":
        H.require_gpu()
    return backend == "hip" or (backend == "auto" and AUTO_IS_DEVICE and values.is_cuda)


def _views(pix, meta):
    return [pix[int(m[0]):int(m[0] + m[1] * m[2])].view(int(m[2]), int(m[1])) for m in meta]


def _render_host(d):
    """the serial renderer over host copies, one sheet per call on the host pool of png.py (a sheet's row of the sheet table
    and of meta are its own; the other tables are shared and read only) -> list of uint8 [H, W] host tensors"""
    values = np.ascontiguousarray(d["values"].detach().cpu().numpy())
    win = np.ascontiguousarray(d["win"].cpu().numpy())
    sheet, panel, curve, stamp = d["tabs"]
    meta, pix, rng = d["meta"].copy(), np.empty(d["total"], np.uint8), np.empty(2 * len(panel), np.float32)

    def one(i):                                                                   # ctypes releases the GIL
        H.call("nppc_curve_render_host", values.ctypes.data, d["N"], d["T"], sheet.ctypes.data + i * sheet.strides[0], 1,
               panel.ctypes.data, len(panel), curve.ctypes.data or None, len(curve), stamp.ctypes.data if len(stamp) else None,
               len(stamp), win.ctypes.data, d["n_items"], rng.ctypes.data, meta.ctypes.data + i * meta.strides[0], pix.ctypes.data,
               pix.size)

    with ThreadPoolExecutor(max_workers=max(1, min(png.HOST_THREADS, os.cpu_count() or 1, d["nimg"]))) as ex:
        list(ex.map(one, range(d["nimg"])))
    _check_fit(meta, "render")
    return _views(torch.from_numpy(pix), meta)


def _device_args(d):
    dev = d["values"].device
    up = lambda a: torch.from_numpy(a).to(dev)
    sheet, panel, curve, stamp = d["tabs"]
    t = dict(sheet=up(sheet), panel=up(panel), curve=up(curve) if len(curve) else torch.zeros(4, dtype=torch.int32, device=dev),
             stamp=up(stamp) if len(stamp) else None, win=d["win"].to(dev), meta=up(d["meta"]),
             rng=torch.empty(2 * len(panel), dtype=torch.float32, device=dev), pix=torch.empty(d["total"], dtype=torch.uint8, device=dev))
    args = (d["values"], d["N"], d["T"], t["sheet"], len(sheet), t["panel"], len(panel), t["curve"], len(curve), t["stamp"], len(stamp),
            t["win"], d["n_items"], d["max_panels"], t["rng"], t["meta"], t["pix"], d["total"])
    return t, args


def render_indices(values, sheets, windows=None, max_frames=None, backend="auto"):
    """the index images of the sheets: a list of uint8 [H, W] tensors, on the device for device values (backend "auto" or
    "hip"), on the host for backend "host".  max_frames: the widest window there can be (default T), which sizes the
    workspace.  ValueError before any launch for curves x (window + 2) beyond 16384 per panel and for images beyond
    png.MAX_DIM or png.MAX_PIXELS."""
    d = _prepare(values, sheets, windows, max_frames)
    _on_device(backend, values)                                                   # the backend's name
    if backend == "host" or (backend == "auto" and not values.is_cuda):
        return _render_host(d)
    H.require_gpu()
    t, args = _device_args(d)
    with torch.cuda.device(values.device):
        H.call("nppc_curve_render", *args, H.stream())
    meta = t["meta"].cpu().numpy()
    _check_fit(meta, "render_indices")
    return _views(t["pix"], meta)


def render_png(values, sheets, windows=None, palette=None, max_frames=None, backend="auto"):
    """the sheets as PNG files: a list of bytes, one per sheet.  On the device one call draws and encodes the batch; backend
    "host" gives the same bytes from the serial renderer and encoder.  palette: 256 x 3, default plot_palette()."""
    pal = png._palette(plot_palette() if palette is None else palette)
    d = _prepare(values, sheets, windows, max_frames)
    if not _on_device(backend, values):
        return png.encode_indexed(_render_host(d), pal, backend="host")
    H.require_gpu()
    t, args = _device_args(d)
    work = png.EncodeWork(d["dims"], values.device)
    with torch.cuda.device(values.device):
        H.call("nppc_curve_render_png", *args, *work.args(pal), H.stream())
        files = work.files()
    if any(not f for f in files):
        _check_fit(t["meta"].cpu().numpy(), "render_png")
    return files


def pitch_sheets(B, K, alphas, T, x_unit, reference_label=True, individual=True, sx=8, plot_height=240, fmin=80.0, fmax=400.0,
                 markers=True, glyph_scale=1, per_item=None):
    """the panels of plot_pitch_comparison over contours stacked as values [B (1 + K A), T]: row b (1 + K A) the reference
    contour of item b (the clean one, or the enhanced one), row b (1 + K A) + 1 + k A + a direction k at alphas[a].
    -> (names, sheets): names[i] = (b, file below the item's directory) of sheets[i].  individual: one
    'pc_<k>_pitch.png' per direction, the reference contour in black at width 2 under the A variations in alpha_colours(A),
    with a legend of every second alpha; always one 'pitch_comparison.png', the reference panel and a panel per direction.
    y runs from fmin to fmax with ticks at every multiple of 100; x ticks about every half second (a whole number of frames).
    per_item: the rows of values per item (default 1 + K A; more when fewer directions are drawn than were tracked)."""
    A = len(alphas)
    colours = alpha_colours(A)
    per = 1 + K * A if per_item is None else int(per_item)
    yticks = [float(v) for v in range(int(math.ceil(fmin / 100.0)) * 100, int(fmax) + 1, 100)]
    every = max(1, int(round(0.5 / x_unit)))
    common = dict(ymin=float(fmin), ymax=float(fmax), yticks=yticks, xtick_every=every, x_unit=x_unit, markers=markers)
    legend = [(colours[a], label(alphas[a])) for a in range(0, A, 2)]
    names, sheets = [], []
    for b in range(B):
        ref = Curve(b * per, INK, 2)
        direction = lambda k: Panel([ref] + [Curve(b * per + 1 + k * A + a, colours[a]) for a in range(A)], legend=legend, **common)
        if individual:
            for k in range(K):
                names.append((b, f"pc_{k + 1}_pitch.png"))
                sheets.append(CurveSheet(b, [direction(k)], sx, plot_height, glyph_scale))
        names.append((b, "pitch_comparison.png"))
        sheets.append(CurveSheet(b, [Panel([ref], **common)] + [direction(k) for k in range(K)], sx, plot_height, glyph_scale))
    return names, sheets


def stack_contours(pitch):
    """the dict of pitch.contours_of_variations -> values [B (1 + K A), T] float32, the rows pitch_sheets names"""
    f0c, f0 = pitch["f0_clean"], pitch["f0"]
    B, K, A, T = f0.shape
    return torch.cat([f0c.reshape(B, 1, T), f0.reshape(B, K * A, T)], dim=1).reshape(B * (1 + K * A), T).float().contiguous()
