"""The shared cases of the curve-sheet tests: the smallest shapes at which the rule of csrc/curve_core.h can go wrong.

values (12 frames, cut to T in {1, 2, 3, 12}); panels drawn over [0, 1] unless they autoscale:
  row 0  a smooth curve, NaN at frame 9        row 5  on ymin, on ymax, on row edges, just outside both, +inf, -inf
  row 1  all NaN                               row 6  row 0 again (two curves that coincide: paint order)
  row 2  NaN at the even frames (dots only)    row 7  one finite value (autoscale's degenerate range)
  row 3  constant                              row 8  a wide range with NaNs (autoscale)
  row 4  bottom to top and back, every frame
windows: item 0 the whole clip, no markers; item 1 one frame, a marker on it; item 2 (T = 12) the interior [3, 9): frame 2 of
row 0 is finite and frame 9 NaN, for row 2 the other way round; markers on the window's first and last frame.
"""
import numpy as np

from nppc_audio.curve_png import Curve, CurveSheet, Panel

TS, SXS, HEIGHTS = (1, 2, 3, 12), (1, 2, 3, 8), (7, 64)
EVERY_GLYPH = "0123456789.- "
NAN = float("nan")


def values12():
    v = np.full((9, 12), np.nan, np.float32)
    t = np.arange(12)
    v[0] = 0.5 + 0.45 * np.sin(t * 0.9)
    v[0, 9] = np.nan
    v[2, 1::2] = 0.1 + 0.07 * t[1::2]
    v[3] = 0.5
    v[4] = (t % 2).astype(np.float32)
    v[5] = [0.0, 1.0, 0.25, 0.5, -1e-7, 1.0000001, np.inf, -np.inf, 3.0 / 7.0, 0.99999994, 1.0 / 64.0, 63.0 / 64.0]
    v[6] = v[0]
    v[7, 0] = 217.25
    v[8] = 100.0 + 30.0 * np.cos(t * 1.7) * t
    v[8, 4:6] = np.nan
    return v


def windows(T):
    one = min(1, T - 1)
    w = [(0, T, -1, -1), (one, one + 1, one, -1)]
    if T == 12:
        w.append((3, 9, 3, 8))
    return w


def sheet(item, sx, PH, g):
    unit = dict(ymin=0.0, ymax=1.0)
    return CurveSheet(item, [
        Panel([Curve(0, 10, 1), Curve(4, 100, 2), Curve(5, 200, 3), Curve(6, 249, 5), Curve(0, 30, 1)], yticks=(0.0, 0.5, 1.0),
              xtick_every=2, x_unit=0.25, markers=True, legend=[(10, "-1.5"), (100, EVERY_GLYPH), (249, "")], **unit),
        Panel([Curve(1, 5, 3), Curve(2, 50, 2), Curve(3, 90, 1)], **unit),                        # no ticks, no legend
        Panel([Curve(7, 20, 3)], yticks=(217.0, 217.25), markers=True),                           # autoscale, one finite value
        Panel([Curve(8, 60, 4), Curve(2, 70, 1), Curve(1, 80, 5)], yticks=(-100.0, 0.0, 100.0), xtick_every=5, x_unit=1.0),
    ], sx, PH, g)


def cases():
    """name -> (values [9, T], sheets, windows)"""
    out = {}
    for T in TS:
        v = np.ascontiguousarray(values12()[:, :T])
        for sx in SXS:
            for PH in HEIGHTS:
                for g in (1, 2):
                    if g == 2 and (sx, PH) not in ((1, 7), (8, 64), (3, 64)):
                        continue
                    w = windows(T)
                    out[f"T{T}_sx{sx}_h{PH}_g{g}"] = (v, [sheet(i, sx, PH, g) for i in range(len(w))], w)
    # one panel, nothing around it: the image is the box and the plot
    v = np.ascontiguousarray(values12()[:, :3])
    out["bare"] = (v, [CurveSheet(0, [Panel([Curve(4, 7, 1)], 0.0, 1.0)], 1, 7, 1)], [(0, 3, -1, -1)])
    return out
