"""Restatement of the PNG writer and of the spectrogram renderer (csrc/png_core.h, csrc/spec_png.hip)
in plain Python, written from RFC 1951 (deflate), RFC 1950 (zlib) and the PNG specification.  zlib is used for crc32 and
adler32 only.

The file: signature, IHDR (8 bits, colour type 3), PLTE (256 entries), one IDAT, IEND.  Every scanline has filter type 2 (Up,
the row above row 0 being zeros); the filtered stream s has H (W + 1) bytes.  zlib header 78 01, one deflate block
(BFINAL = 1, BTYPE = 01), end code 256, padding, Adler-32 of s.  The token rule: s is split into maximal runs of equal bytes
(rows do not matter); a run of L bytes emits a literal, then while rem = L - 1 >= 3 a match of distance 1 and length
min(258, rem); the last rem < 3 bytes are literals.
"""
import struct
import zlib

import numpy as np

SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])


# ---- RFC 1951 section 3.2.2: canonical codes from code lengths; section 3.2.6: the fixed lengths ------------------------------
def canonical(lengths):
    count = {}
    for n in lengths:
        count[n] = count.get(n, 0) + 1
    count[0] = 0
    code, nxt = 0, {}
    for bits in range(1, max(lengths) + 1):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        out.append((nxt[n], n))
        nxt[n] += 1
    return out


FIXED = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)

# section 3.2.5: (code, extra bits, first length)
LENGTHS = []
_base = 3
for _i in range(28):
    _e = 0 if _i < 8 else (_i - 4) // 4
    LENGTHS.append((257 + _i, _e, _base))
    _base += 1 << _e
LENGTHS.append((285, 0, 258))
assert LENGTHS[8] == (265, 1, 11) and LENGTHS[27] == (284, 5, 227) and LENGTHS[20] == (277, 4, 67)


class Bits:
    """bytes filled from bit 0; Huffman codes most significant bit first, everything else least significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def plain(self, v, n):
        self.acc |= v << self.n
        self.n += n

    def huffman(self, sym):
        code, n = FIXED[sym]
        for i in range(n - 1, -1, -1):
            self.plain((code >> i) & 1, 1)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def filtered(idx):
    """the Up-filtered stream of a uint8 image [H, W]"""
    idx = np.asarray(idx, np.uint8)
    up = np.concatenate([np.zeros((1, idx.shape[1]), np.uint8), idx[:-1]])
    rows = np.concatenate([np.full((idx.shape[0], 1), 2, np.uint8), idx - up], axis=1)
    return rows.tobytes()


def tokens(s):
    """[('lit', v) | ('match', length)]"""
    out, i, n = [], 0, len(s)
    while i < n:
        j = i
        while j < n and s[j] == s[i]:
            j += 1
        out.append(("lit", s[i]))
        rem = j - i - 1
        while rem >= 3:
            m = min(258, rem)
            out.append(("match", m))
            rem -= m
        out.extend([("lit", s[i])] * rem)
        i = j
    return out


def deflate(s):
    b = Bits()
    b.plain(1, 1)                                                   # BFINAL
    b.plain(1, 2)                                                   # BTYPE = 01
    for kind, v in tokens(s):
        if kind == "lit":
            b.huffman(v)
        else:
            code, extra, first = [t for t in LENGTHS if t[2] <= v][-1] if v < 258 else LENGTHS[28]
            b.huffman(code)
            b.plain(v - first, extra)
            b.plain(0, 5)                                           # distance code 0 (distance 1), 5 bits, a Huffman code of zeros
    b.huffman(256)
    return b.bytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(idx, palette):
    idx = np.asarray(idx, np.uint8)
    h, w = idx.shape
    s = filtered(idx)
    z = b"\x78\x01" + deflate(s) + struct.pack(">I", zlib.adler32(s))
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)) +
            chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()) + chunk(b"IDAT", z) + chunk(b"IEND", b""))


def bound(w, h):
    n = h * (w + 1)
    return 8 + 25 + (12 + 768) + 12 + (2 + (3 + 9 * n + 7 + 7) // 8 + 4) + 12


def idat(png):
    """the payload of the one IDAT chunk"""
    at = 8
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        if kind == b"IDAT":
            return png[at + 8:at + 8 + n]
        at += 12 + n
    raise ValueError("no IDAT")


# ---- the context window ---------------------------------------------------------------------------------------------------------
def window(mask_row):
    """(t0, t1, marker 0, marker 1) of one item: mask_row [T], 0 inside the gap.  The gap [s, e) widened by its own length on
    each side, clamped to the clip; the markers stand at s and e.  No gap: the whole clip, no marker."""
    gap = np.flatnonzero(np.asarray(mask_row) == 0)
    n = len(mask_row)
    if gap.size == 0:
        return 0, n, -1, -1
    s, e = int(gap[0]), int(gap[-1]) + 1
    d = e - s
    return max(0, s - d), min(n, e + d), s, e


# ---- the renderer ---------------------------------------------------------------------------------------------------------------
def scale_of(vmin, vmax):
    return np.float32(254.0 / (float(vmax) - float(vmin)))


def cell_values(planes, b, cell, t0, t1, dtype):
    """g(P + alpha Q) [F, t1 - t0] of item b in `dtype`; planes [B, NP, CH, F, T]"""
    x = np.asarray(planes)
    alpha = dtype(np.float32(cell.alpha))
    v = None
    if cell.q is not None:
        v = alpha * x[b, cell.q, :, :, t0:t1].astype(dtype)                    # multiply
    if cell.p is not None:
        p = x[b, cell.p, :, :, t0:t1].astype(dtype)
        v = p if v is None else p + v                                         # then add
    if x.shape[2] == 1:
        return np.abs(v[0]) if cell.g == "abs" else v[0]
    if cell.g == "identity":
        return v[0]
    mag = np.sqrt(v[0] * v[0] + v[1] * v[1])
    return mag if cell.g == "abs" else dtype(20.0) * np.log10(mag + dtype(np.float32(1e-8)))


def cell_range(cell, v):
    """(vmin, scale) in fp32 of a cell whose values are v"""
    if np.isnan(cell.vmin) and np.isnan(cell.vmax):
        fin = v[np.isfinite(v)]
        if fin.size == 0 or fin.min() == fin.max():
            return np.float32(fin.min() if fin.size else 0.0), np.float32(0.0)
        lo, hi = np.float32(fin.min()), np.float32(fin.max())
        return lo, np.float32(254.0) / (hi - lo)
    return np.float32(cell.vmin), scale_of(cell.vmin, cell.vmax)


def levels(v, vmin, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.floor((v.astype(np.float32) - vmin) * scale)                   # subtract, multiply, floor: each fp32
    return np.where(x >= 0, np.minimum(x, 253), 0).astype(np.uint8)            # NaN: 0


def render(planes, sheet, win):
    """the index image [H, W] of one sheet; real planes exactly (fp32, operation by operation).  win = (t0, t1, m0, m1)"""
    x = np.asarray(planes, np.float32)
    if x.ndim == 4:
        x = x[:, :, None]
    F = x.shape[3]
    t0, t1, m0, m1 = win
    R, C = len(sheet.cells), len(sheet.cells[0])
    cw, ch, g = (t1 - t0) * sheet.sx, F * sheet.sy, sheet.gutter
    img = np.full((R * ch + (R - 1) * g, C * cw + (C - 1) * g), 255, np.uint8)
    for r, row in enumerate(sheet.cells):
        for c, cell in enumerate(row):
            if cell is None or (cell.p is None and cell.q is None):
                continue
            v = cell_values(x, sheet.item, cell, t0, t1, np.float32)
            lev = levels(v, *cell_range(cell, v))
            tile = np.repeat(np.repeat(lev[::-1], sheet.sy, axis=0), sheet.sx, axis=1)        # bin 0 at the bottom
            if cell.markers:
                rows = (np.arange(ch) // 4) % 2 == 0
                for m in (m0, m1):
                    if t0 <= m < t1:
                        tile[rows, (m - t0) * sheet.sx] = 254
            img[r * (ch + g):r * (ch + g) + ch, c * (cw + g):c * (cw + g) + cw] = tile
    return img


def positions(planes, b, cell, t0, t1):
    """fp64: (the position (v - vmin) 254 / (vmax - vmin) of every pixel of a cell [F, t1 - t0], bin 0 first; vmin; vmax)"""
    x = np.asarray(planes, np.float64)
    v = cell_values(x, b, cell, t0, t1, np.float64)
    if np.isnan(cell.vmin):
        fin = v[np.isfinite(v)]
        vmin, vmax = fin.min(), fin.max()
    else:
        vmin, vmax = float(cell.vmin), float(cell.vmax)
    return (v - vmin) * 254.0 / (vmax - vmin) if vmax > vmin else np.zeros_like(v), vmin, vmax
