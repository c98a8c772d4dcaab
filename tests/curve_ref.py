"""Restatement of the curve-sheet rule (csrc/curve_core.h) in numpy, written from the rule: it PAINTS
(background, grid, markers, then every curve's core pixels grown by its width, in order) where the renderers gather, and it
takes the sheets as nppc_audio.curve_png describes them, not the integer tables.

  quantisation   x = floor((v - ymin) * scale), each operation an fp32 operation of its own; NaN: no point; otherwise the
                 row is x clamped to [0, PH - 1] (a NaN x, from 0 * inf, is row 0); row 0 is the bottom pixel row
  autoscale      mn, mx of the finite values of the panel's curves in [t0, t1): ymin = mn, scale = fp32(PH) / (mx - mn);
                 mn == mx: ymin = mn - 0.5, scale = PH; none: ymin = 0, scale = PH
  columns        frame t: [(t - t0) sx, (t - t0 + 1) sx), point in column c(t) = (t - t0) sx + sx // 2
  segment        points (t, ra), (t + 1, rb): R(j) = ra + (rb - ra) j // sx; column c(t) + j, j in 0 .. sx - 1, lights R(j) and
                 the rows from it towards R(j + 1), short of R(j + 1); a point lights (c(t), ra); frames t0 - 1 and t1 take
                 part, columns outside [0, PW) are dropped before the width is applied
  width w        offsets -(w - 1) // 2 .. w // 2 in x and in rows (upwards), clipped to the plot area
"""
import numpy as np

FONT_CHARS = "0123456789.- "
FONT = [  # 7 rows per glyph, bit 4 the leftmost dot
    (0x0e, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0e), (0x04, 0x0c, 0x04, 0x04, 0x04, 0x04, 0x0e), (0x0e, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1f),
    (0x1e, 0x01, 0x01, 0x0e, 0x01, 0x01, 0x1e), (0x02, 0x06, 0x0a, 0x12, 0x1f, 0x02, 0x02), (0x1f, 0x10, 0x1e, 0x01, 0x01, 0x11, 0x0e),
    (0x06, 0x08, 0x10, 0x1e, 0x11, 0x11, 0x0e), (0x1f, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), (0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e),
    (0x0e, 0x11, 0x11, 0x0f, 0x01, 0x02, 0x0c), (0, 0, 0, 0, 0, 0x0c, 0x0c), (0, 0, 0, 0x1f, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0)]
INK, GRID, MARKER, BACKGROUND = 250, 251, 254, 255
LDS_ROWS = 16384
MAX_DIM, MAX_PIXELS = 16384, 1 << 26
F32 = np.float32


def label(v):
    s = f"{float(v):.2f}".rstrip("0").rstrip(".")
    return "0" if s in ("-0", "") else s


def position(v, ymin, scale):
    with np.errstate(all="ignore"):
        d = F32(v) - F32(ymin)
        return np.floor(F32(d * F32(scale)))


def row_of(v, ymin, scale, PH):
    if np.isnan(v):
        return None
    x = position(v, ymin, scale)
    return 0 if not x >= 0 else PH - 1 if x > PH - 1 else int(x)


def tick_row(v, ymin, scale, PH):
    x = position(v, ymin, scale)
    if not x >= 0 or not x <= PH:
        return None
    return min(int(x), PH - 1)


def panel_range(values, panel, t0, t1, PH):
    if not (np.isnan(panel.ymin) and np.isnan(panel.ymax)):
        return F32(panel.ymin), F32(PH / (panel.ymax - panel.ymin))
    seen = [values[c.row, t0:t1] for c in panel.curves]
    seen = np.concatenate(seen) if seen else np.zeros(0, F32)
    seen = seen[np.isfinite(seen)]
    if not seen.size:
        return F32(0.0), F32(PH)
    mn, mx = F32(seen.min()), F32(seen.max())
    if mn == mx:
        return F32(mn - F32(0.5)), F32(PH)
    return mn, F32(F32(PH) / F32(mx - mn))


def x_labels(panel, T):
    if not panel.xtick_every:
        return []
    return [(t, label(t * panel.x_unit)) for t in range(0, T, int(panel.xtick_every))]


def layout(sheet, frames, T):
    """-> dict(W, H, ML, MR, PW, tops, heights)"""
    g = sheet.glyph_scale
    max_y = max([len(label(v)) for p in sheet.panels for v in p.yticks], default=0)
    legends = [len(text) for p in sheet.panels for _, text in p.legend]
    ML = 6 * g * max_y + 2 * g if max_y else 0
    MR = 11 * g + 6 * g * max(legends) if legends else 0
    PW = frames * sheet.sx
    heights = [4 * g + sheet.plot_height + 2 + (9 * g if any(text for _, text in x_labels(p, T)) else 4 * g) for p in sheet.panels]
    tops = [int(v) for v in np.concatenate([[0], np.cumsum(heights)[:-1]])]
    return dict(W=ML + PW + 2 + MR, H=sum(heights), ML=ML, MR=MR, PW=PW, tops=tops, heights=heights)


def refused(sheet, frames, T):
    """why the renderers refuse the sheet, or None"""
    if max(len(p.curves) for p in sheet.panels) * (frames + 2) > LDS_ROWS:
        return "lds"
    L = layout(sheet, frames, T)
    if L["W"] > MAX_DIM or L["H"] > MAX_DIM or L["W"] * L["H"] > MAX_PIXELS:
        return "size"
    return None


def core_pixels(rows, t0, t1, sx, PW):
    """rows: {t: row} for the frames t0 - 1 .. t1 that hold a point -> set of (x, row)"""
    core = set()
    for t in range(t0 - 1, t1 + 1):
        if t not in rows:
            continue
        c, ra = (t - t0) * sx + sx // 2, rows[t]
        core.add((c, ra))
        if t + 1 in rows and t + 1 <= t1:
            rb = rows[t + 1]
            R = [ra + ((rb - ra) * j) // sx for j in range(sx + 1)]
            for j in range(sx):
                step = 1 if R[j + 1] > R[j] else -1
                for r in ([R[j]] if R[j + 1] == R[j] else range(R[j], R[j + 1], step)):
                    core.add((c + j, r))
    return {(x, r) for x, r in core if 0 <= x < PW}


def draw_text(img, text, g, x0, y0, band):
    """dots as g x g blocks in INK, clipped to the rows band = (first, one past last) and to the image"""
    for ci, ch in enumerate(text):
        glyph = FONT[FONT_CHARS.index(ch)]
        for gy in range(7):
            for gx in range(5):
                if (glyph[gy] >> (4 - gx)) & 1:
                    fill(img, INK, x0 + ci * 6 * g + gx * g, y0 + gy * g, g, g, band)


def fill(img, colour, x0, y0, w, h, band):
    ya, yb = max(y0, band[0]), min(y0 + h, band[1])
    xa, xb = max(x0, 0), min(x0 + w, img.shape[1])
    if ya < yb and xa < xb:
        img[ya:yb, xa:xb] = colour


def render(values, sheet, window):
    """values [N, T] float32 (numpy), a CurveSheet, window (t0, t1, marker0, marker1) -> uint8 [H, W]"""
    values = np.asarray(values, F32)
    T = values.shape[1]
    t0, t1, m0, m1 = window
    assert 0 <= t0 < t1 <= T
    L = layout(sheet, t1 - t0, T)
    g, sx, PH, PW, ML = sheet.glyph_scale, sheet.sx, sheet.plot_height, L["PW"], L["ML"]
    img = np.full((L["H"], L["W"]), BACKGROUND, np.uint8)
    for panel, top, hp in zip(sheet.panels, L["tops"], L["heights"]):
        band = (top, top + hp)
        ymin, scale = panel_range(values, panel, t0, t1, PH)
        bx0, bx1, by0 = ML, ML + PW + 1, top + 4 * g
        by1 = by0 + PH + 1
        ticks = [(tick_row(F32(v), ymin, scale, PH), label(v)) for v in panel.yticks]
        # the margins: stamps in the order y labels, x labels, legend; then the box
        for r, text in ticks:
            if r is not None:
                draw_text(img, text, g, ML - g - 6 * g * len(text), by0 + 1 + (PH - 1 - r) - 3 * g, band)
        for t, text in x_labels(panel, T):
            if t0 <= t < t1:
                cx = ML + 1 + (t - t0) * sx + sx // 2
                draw_text(img, text, g, cx - (6 * g * len(text) - g) // 2, by1 + 1 + g, band)
        for n, (colour, text) in enumerate(panel.legend):
            xs, ys = bx1 + 1 + 2 * g, by0 + g + 8 * g * n
            fill(img, colour, xs, ys, 7 * g, 7 * g, band)
            draw_text(img, text, g, xs + 8 * g, ys, band)
        img[by0, bx0:bx1 + 1] = img[by1, bx0:bx1 + 1] = INK
        img[by0:by1 + 1, bx0] = img[by0:by1 + 1, bx1] = INK
        # the plot area, rows counted from the bottom
        plot = np.full((PH, PW), BACKGROUND, np.uint8)
        for r, _ in ticks:
            if r is not None:
                plot[r, :] = GRID
        centre = lambda t: (t - t0) * sx + sx // 2
        if panel.xtick_every:
            for t in range(t0, t1):
                if t % int(panel.xtick_every) == 0:
                    plot[:, centre(t)] = GRID
        if panel.markers:
            from_top = np.arange(PH)
            dashed = PH - 1 - from_top[(from_top // 4) % 2 == 0]
            for m in (m0, m1):
                if t0 <= m < t1:
                    plot[dashed, centre(m)] = MARKER
        for c in panel.curves:
            rows = {}
            for t in range(max(t0 - 1, 0), min(t1 + 1, T)):
                r = row_of(values[c.row, t], ymin, scale, PH)
                if r is not None:
                    rows[t] = r
            w = c.width
            for x, r in core_pixels(rows, t0, t1, sx, PW):
                xa, xb = max(x - (w - 1) // 2, 0), min(x + w // 2, PW - 1)
                ra, rb = max(r - (w - 1) // 2, 0), min(r + w // 2, PH - 1)
                plot[ra:rb + 1, xa:xb + 1] = c.colour
        img[by0 + 1:by1, bx0 + 1:bx1] = plot[::-1]
    return img
