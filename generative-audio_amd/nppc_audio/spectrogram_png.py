"""Spectrogram sheets drawn and written as PNG on the device (csrc/spec_png.hip; specification
tests/png_ref.py).

A `Sheet` is a grid of cells over the frames [t0, t1) of one item of a stacked tensor `planes` [B, NP, F, T] (real) or
[B, NP, 2, F, T] (complex).  A `Cell` shows g(P + alpha Q) for two planes (either may be absent) through a colour range
(vmin, vmax): index = clamp(floor((v - vmin) 254 / (vmax - vmin)), 0, 253), NaN 0; vmin = vmax = NaN autoscales to the
cell's finite values.  Index 254 is the gap marker, 255 the background of blank cells and gutters; frequency bin 0 is the
bottom row; every source pixel is sx x sy pixels.

`render_png` goes from the planes to PNG bytes in one device call (three launches to draw, a memset and four to encode, one
small host read, one copy of exactly the encoded bytes); neither an RGB image nor a full index image passes through the
host.  `render_indices` returns the index images.  Not drawn: titles, axes, tick labels, colour bars; the file name and the
sheet's fixed layout carry that.  No pixel parity with matplotlib's figures is claimed.
"""
import math
import struct
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _hip as H
from . import png

G = {"identity": 0, "abs": 1, "db": 2}
NAN = float("nan")


@dataclass
class Cell:
    p: Optional[int] = None           # plane of P, or None
    q: Optional[int] = None           # plane of Q, or None
    alpha: float = 1.0
    g: str = "identity"               # "identity", "abs" or "db" (20 log10(|z| + 1e-8), complex planes)
    vmin: float = NAN                 # both NaN: autoscale
    vmax: float = NAN
    markers: bool = False             # the gap's first frame and the one past its last, dashed, in index 254


@dataclass
class Sheet:
    item: int
    cells: List[List[Optional[Cell]]]           # rows of equal length; None is a blank cell
    sx: int = 1
    sy: int = 1
    gutter: int = 0
    rows: int = field(init=False, default=0)
    cols: int = field(init=False, default=0)

    def __post_init__(self):
        self.rows, self.cols = len(self.cells), len(self.cells[0]) if self.cells else 0
        if not self.rows or not self.cols or any(len(r) != self.cols for r in self.cells):
            raise ValueError("a sheet is a non-empty grid of rows of equal length")
        if self.sx < 1 or self.sy < 1 or self.gutter < 0 or self.sx > 64 or self.sy > 64 or self.gutter > 1024:
            raise ValueError("sx, sy in 1..64 and gutter in 0..1024")


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _tables(sheets, NP, CH):
    img = np.zeros((len(sheets), 8), np.int32)
    cells = []
    for i, s in enumerate(sheets):
        img[i, :7] = (s.item, s.rows, s.cols, len(cells), s.sx, s.sy, s.gutter)
        for row in s.cells:
            for c in row:
                if c is None or (c.p is None and c.q is None):
                    cells.append((-1, -1, 0, 0, 0, 0, 0, i))
                    continue
                if c.g not in G or (c.g == "db" and CH != 2):
                    raise ValueError(f"g must be 'identity', 'abs' or, for complex planes, 'db'; got {c.g!r}")
                for pl in (c.p, c.q):
                    if pl is not None and not 0 <= pl < NP:
                        raise ValueError(f"plane {pl} of {NP}")
                auto = math.isnan(c.vmin) and math.isnan(c.vmax)
                if not auto and not c.vmax > c.vmin:
                    raise ValueError("a cell's range is vmin < vmax, or both NaN")
                vmin, scale = (0.0, 0.0) if auto else (float(np.float32(c.vmin)), float(np.float32(254.0 / (c.vmax - c.vmin))))
                cells.append((-1 if c.p is None else c.p, -1 if c.q is None else c.q, G[c.g], int(auto) | 2 * int(c.markers),
                              _bits(float(np.float32(c.alpha))), _bits(vmin), _bits(scale), i))
    return img, np.array(cells, np.int32).reshape(-1, 8)


def windows_from_mask(mask):
    """mask [B, T] (device, 0 inside the gap) -> int32 [B, 4]: t0, t1, marker 0, marker 1: the gap widened by its own length
    on each side and clamped to the clip; an item without a gap shows the whole clip, without markers"""
    H.require_gpu()
    mask = mask.detach().float().contiguous()
    if mask.dim() != 2:
        raise ValueError("windows_from_mask takes a mask [B, T]")
    win = torch.empty(mask.shape[0], 4, dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        H.call("nppc_spec_windows", mask, mask.shape[0], mask.shape[1], win, H.stream())
    return win


def _prepare(planes, sheets, windows, max_frames):
    H.require_gpu()
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.float32 or planes.dim() not in (4, 5) or not planes.is_cuda:
        raise ValueError("planes is a float32 device tensor [B, NP, F, T] or [B, NP, 2, F, T]")
    if planes.dim() == 4:
        planes = planes.unsqueeze(2)
    planes = planes.contiguous()
    B, NP, CH, F, T = planes.shape
    sheets = list(sheets)
    if not sheets or CH not in (1, 2) or min(B, NP, F, T) < 1:
        raise ValueError("render: no sheet, or an empty tensor")
    for s in sheets:
        if not 0 <= s.item < B:
            raise ValueError(f"item {s.item} of {B}")
    dev = planes.device
    if windows is None:
        windows = torch.tensor([[0, T, -1, -1]] * B, dtype=torch.int32, device=dev)
    if windows.dtype != torch.int32 or tuple(windows.shape) != (B, 4):
        raise ValueError("windows is an int32 tensor [B, 4]")
    windows = windows.to(dev).contiguous()
    frames = T if max_frames is None else min(int(max_frames), T)
    dims = [(s.cols * frames * s.sx + (s.cols - 1) * s.gutter, s.rows * F * s.sy + (s.rows - 1) * s.gutter) for s in sheets]
    for w, h in dims:
        if not (w <= png.MAX_DIM and h <= png.MAX_DIM and w * h <= png.MAX_PIXELS):
            raise ValueError(f"render: a sheet of up to {w} x {h} pixels (1..{png.MAX_DIM} each way, at most 2^26 pixels)")
    img, cells = _tables(sheets, NP, CH)
    allow = np.array([w * h for w, h in dims], np.int64)
    off = np.concatenate([[0], np.cumsum(allow)])
    meta = np.zeros((len(sheets), 4), np.int64)
    meta[:, 0], meta[:, 3] = off[:-1], allow
    d = dict(planes=planes, shape=(B, NP, CH, F, T), dims=dims, nimg=len(sheets), ncells=len(cells),
             img=torch.from_numpy(img).to(dev), cells=torch.from_numpy(cells).to(dev), win=windows,
             rng=torch.empty(len(cells) * 2, dtype=torch.float32, device=dev), meta=torch.from_numpy(meta).to(dev),
             pix=torch.empty(int(off[-1]), dtype=torch.uint8, device=dev), off=off, max_pixels=int(allow.max()))
    return d


def _render_args(d):
    return (d["planes"], *d["shape"], d["img"], d["nimg"], d["cells"], d["ncells"], d["win"], d["rng"], d["meta"], d["pix"],
            d["pix"].numel(), d["max_pixels"])


def _check_fit(meta, what):
    if (meta[:, 1] < 1).any():
        raise ValueError(f"{what}: sheet {int(np.flatnonzero(meta[:, 1] < 1)[0])} has an empty window, or one wider than max_frames")


def render_indices(planes, sheets, windows=None, max_frames=None):
    """the index images of the sheets: a list of uint8 device tensors [H, W] (ragged: a sheet is as wide as its item's
    window).  windows: int32 [B, 4] (windows_from_mask), default the whole clip; max_frames: the widest window there can be
    (default T), which sizes the workspace."""
    d = _prepare(planes, sheets, windows, max_frames)
    with torch.cuda.device(d["planes"].device):
        H.call("nppc_spec_render", *_render_args(d), H.stream())
    meta = d["meta"].cpu().numpy()
    _check_fit(meta, "render_indices")
    return [d["pix"][int(m[0]):int(m[0] + m[1] * m[2])].view(int(m[2]), int(m[1])) for m in meta]


def render_png(planes, sheets, windows=None, palette="viridis", max_frames=None):
    """the sheets as PNG files: a list of bytes, one per sheet, in one device call"""
    pal = png._palette(png.palette(palette) if isinstance(palette, str) else palette)
    d = _prepare(planes, sheets, windows, max_frames)
    work = png.EncodeWork(d["dims"], d["planes"].device)
    with torch.cuda.device(d["planes"].device):
        H.call("nppc_spec_render_png", *_render_args(d), *work.args(pal), H.stream())
        files = work.files()
    if any(not f for f in files):
        _check_fit(d["meta"].cpu().numpy(), "render_png")
    return files
