"""CPU: the serial curve-sheet renderer (nppc_curve_render_host over csrc/curve_core.h) gives pixel for pixel what the
restatement tests/curve_ref.py gives on the cases of tests/curve_cases.py; Pillow reads the files back; the layout entry
point agrees with the restatement's layout; the refusals are ValueErrors; the validators' sheet builder names the
reference's files and puts the right contours into the right panels."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import curve_cases
import curve_ref as R
from nppc_audio import _hip as H
from nppc_audio import curve_png as CP
from nppc_audio import png
from nppc_audio.curve_png import Curve, CurveSheet, Panel

CASES = curve_cases.cases()


@pytest.fixture(scope="module")
def drawn():
    """name -> the host renderer's index images, drawn once and shared (read-only)"""
    return {n: [t.numpy() for t in CP.render_indices(torch.from_numpy(v), sheets, torch.tensor(w, dtype=torch.int32), backend="host")]
            for n, (v, sheets, w) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_host_renderer_equals_the_restatement(drawn, name):
    v, sheets, w = CASES[name]
    for s, got in zip(sheets, drawn[name]):
        want = R.render(v, s, w[s.item])
        assert got.shape == want.shape, (name, s.item)
        assert np.array_equal(got, want), (name, s.item, np.argwhere(got != want)[:5].tolist())


def test_the_cases_cover_what_they_are_there_for(drawn):
    shapes = {g.shape for imgs in drawn.values() for g in imgs}
    assert any(w % 4 for _, w in shapes) and any((h * w) % 4 for h, w in shapes)          # the four-pixel store's tail
    assert drawn["bare"][0].shape == (4 + 7 + 2 + 4, 3 + 2)
    seen = set(np.unique(np.concatenate([g.ravel() for g in drawn["T12_sx8_h64_g2"]])).tolist())
    assert {10, 30, 100, 200, 249, 5 + 45, 90, 20, 60, 70, CP.INK, CP.GRID, CP.MARKER, CP.BACKGROUND} <= seen
    assert 80 not in seen and 5 not in seen                                               # the all-NaN curve draws nothing
    # the bare panel, by hand: rows 0 and 6 alternate, joined by vertical runs (sx = 1: the run stands in the left column)
    plot = drawn["bare"][0][5:12, 1:4]
    assert plot[:, 0].tolist() == [255, 7, 7, 7, 7, 7, 7] and plot[:, 1].tolist() == [7, 7, 7, 7, 7, 7, 255]
    assert plot[:, 2].tolist() == [255] * 6 + [7]
    # paint order: the later of two coinciding curves (row 0 drawn last in colour 30, width 1) lies over the wider 249
    g = drawn["T12_sx8_h64_g1"][0]
    assert (g == 30).sum() > 0 and (g == 10).sum() == 49                                   # 10: nothing but its legend swatch
    # autoscale with one finite value: a range of one around it, the dot in the middle row
    v, sheets, w = CASES["T12_sx1_h7_g1"]
    ymin, scale = R.panel_range(v, sheets[0].panels[2], 0, 12, 7)
    assert (float(ymin), float(scale)) == (216.75, 7.0) and R.row_of(v[7, 0], ymin, scale, 7) == 3


def test_png_files_decode_to_the_palette_colours(drawn):
    name = "T12_sx3_h64_g2"
    v, sheets, w = CASES[name]
    files = CP.render_png(torch.from_numpy(v), sheets, torch.tensor(w, dtype=torch.int32), backend="host")
    pal = CP.plot_palette()
    assert len(files) == len(sheets)
    for f, idx in zip(files, drawn[name]):
        im = Image.open(io.BytesIO(f))
        assert im.size == (idx.shape[1], idx.shape[0])
        assert np.array_equal(np.asarray(im.convert("RGB")), pal[idx])
    assert files == png.encode_indexed([torch.from_numpy(g) for g in drawn[name]], pal, backend="host")


def test_palette_and_alpha_colours():
    pal, vir = CP.plot_palette(), png.palette("viridis")
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[0].tolist() == vir[0].tolist() and pal[249].tolist() == vir[253].tolist() and pal[100].tolist() == vir[102].tolist()
    assert pal[250].tolist() == [0, 0, 0] and pal[254].tolist() == [255, 0, 0]
    assert pal[252].tolist() == pal[253].tolist() == pal[255].tolist() == [255, 255, 255] and pal[251].tolist() == [204, 204, 204]
    assert CP.alpha_colours(13) == [int(np.rint(v)) for v in np.linspace(0, 249, 13)] and CP.alpha_colours(1) == [0]
    assert CP.alpha_colours(13)[0] == 0 and CP.alpha_colours(13)[-1] == 249
    assert [CP.label(v) for v in (0, -0.0, 100.0, 0.5, 1.024, -3, 2.5)] == ["0", "0", "100", "0.5", "1.02", "-3", "2.5"]


def test_layout_entry_point_equals_the_restatement():
    for name in ("T12_sx8_h64_g2", "T3_sx2_h7_g1", "bare", "T1_sx1_h7_g1"):
        v, sheets, w = CASES[name]
        tabs = CP._tables(sheets, *v.shape)
        for i, s in enumerate(sheets):
            for frames in {1, v.shape[1]}:
                L = R.layout(s, frames, v.shape[1])
                assert CP.shape(tabs, v.shape[0], v.shape[1], i, frames)[:5] == (L["W"], L["H"], L["ML"], L["MR"], L["PW"]), (name, i)
    # by hand: g = 2, the longest y label "217.25" (6 glyphs), legend text of 13: ML = 72 + 4, MR = 22 + 156
    s = CASES["T12_sx8_h64_g2"][1][0]
    L = R.layout(s, 12, 12)
    assert (L["ML"], L["MR"], L["PW"], L["W"]) == (76, 178, 96, 76 + 96 + 2 + 178)
    assert L["heights"] == [8 + 64 + 2 + 18, 8 + 64 + 2 + 8, 8 + 64 + 2 + 8, 8 + 64 + 2 + 18]


def test_refusals_are_value_errors_before_anything_is_drawn():
    v = torch.zeros(2, 5000)
    one = lambda **kw: CurveSheet(0, [Panel([Curve(0, 1)], 0.0, 1.0)], **kw)
    with pytest.raises(ValueError, match="16384"):                                        # 4 x 5002 rows
        CP.render_indices(v, [CurveSheet(0, [Panel([Curve(0, 1)] * 4, 0.0, 1.0)], 1, 8)], backend="host")
    assert R.refused(CurveSheet(0, [Panel([Curve(0, 1)] * 4, 0.0, 1.0)], 1, 8), 5000, 5000) == "lds"
    CP.render_indices(v, [CurveSheet(0, [Panel([Curve(0, 1)] * 4, 0.0, 1.0)], 1, 8)], max_frames=4094,
                      windows=torch.tensor([[0, 4094, -1, -1]], dtype=torch.int32), backend="host")      # 4 x 4096: the cap itself
    with pytest.raises(ValueError, match="wider or higher"):                              # 5000 x 4 + 2 columns
        CP.render_indices(v, [one(sx=4, plot_height=8)], backend="host")
    assert R.refused(one(sx=4, plot_height=8), 5000, 5000) == "size"
    with pytest.raises(ValueError, match="wider or higher"):                              # 10002 x 8192 pixels
        CP.render_png(v, [one(sx=2, plot_height=8182)], backend="host")
    with pytest.raises(ValueError, match="max_frames"):                                   # a window wider than the workspace
        CP.render_indices(v, [one(sx=1, plot_height=8)], max_frames=10, backend="host")
    for bad in (lambda: Curve(0, 1, 6), lambda: Curve(0, 256), lambda: Panel([], 1.0, 1.0), lambda: Panel([], 0.0, NAN_),
                lambda: Panel([], legend=[(1, "a")]), lambda: Panel([], legend=[(1, "0" * 17)]), lambda: CurveSheet(0, []),
                lambda: one(sx=0), lambda: one(sx=65), lambda: one(glyph_scale=9), lambda: Panel([], xtick_every=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        CP.render_indices(torch.zeros(2, 4), [CurveSheet(0, [Panel([Curve(2, 1)], 0.0, 1.0)])], backend="host")   # row 2 of 2
    with pytest.raises(ValueError):
        CP.render_indices(torch.zeros(2, 4), [CurveSheet(1, [Panel([Curve(0, 1)], 0.0, 1.0)])],
                          windows=torch.tensor([[0, 4, -1, -1]], dtype=torch.int32), backend="host")              # item 1 of 1
    with pytest.raises(ValueError):
        CP.render_indices(torch.zeros(2, 4, dtype=torch.float64), [one()], backend="host")
    with pytest.raises(ValueError):
        CP.render_indices(torch.zeros(2, 4), [one()], backend="cpu")


NAN_ = float("nan")


def test_symbols_are_declared_bound_and_refuse_bad_arguments():
    names = ["nppc_curve_shape", "nppc_curve_render", "nppc_curve_render_png", "nppc_curve_render_host"]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nppc_hip.h")).read()
    for n in names:
        assert n in H.SIGS and hasattr(H.lib(), n) and f"int {n}(" in header
    bad = pytest.raises(RuntimeError, match="bad argument")
    with bad:
        H.call("nppc_curve_shape", None, 1, None, 1, None, 0, None, 0, 1, 1, 0, 1, None, None, None)
    with bad:
        H.call("nppc_curve_render_host", None, 1, 1, None, 1, None, 1, None, 0, None, 0, None, 1, None, None, None, 1)
    with bad:                                                                             # null pointers: before any launch
        H.call("nppc_curve_render", None, 1, 1, None, 1, None, 1, None, 0, None, 0, None, 1, 1, None, None, None, 1, None)
    with bad:                                                                             # 65 panels
        H.call("nppc_curve_render", 8, 1, 1, 8, 1, 8, 1, 8, 0, None, 0, 8, 1, 65, 8, 8, 8, 1, None)
    with bad:
        H.call("nppc_curve_render_png", 8, 1, 1, 8, 1, 8, 1, 8, 0, None, 0, 8, 1, 1, 8, 8, 8, 1, 8, 8, 0, 8, 8, 8, 8, 8, 8, None)
    # a table the layout cannot accept is not drawn: W = H = 0, nothing written
    v, sheets, w = CASES["bare"]
    sheet, panel, curve, stamp = CP._tables(sheets, *v.shape)
    for col, val in ((2, 9), (1, -1)):                                                    # width 9; colour -1
        broken = curve.copy()
        broken[0, col] = val
        meta, pix, rng, win = np.array([[0, 0, 0, 1000]], np.int64), np.full(1000, 77, np.uint8), np.zeros(2, np.float32), np.array(w, np.int32)
        H.call("nppc_curve_render_host", v.ctypes.data, 9, 3, sheet.ctypes.data, 1, panel.ctypes.data, 1, broken.ctypes.data, 1, None, 0,
               win.ctypes.data, 1, rng.ctypes.data, meta.ctypes.data, pix.ctypes.data, 1000)
        assert meta[0].tolist() == [0, 0, 0, 1000] and (pix == 77).all()


def test_pitch_sheets_name_the_references_files_and_fill_the_panels():
    B, K, A, T = 2, 3, 5, 20
    alphas = [-1.0, -0.5, 0.0, 0.5, 1.0]
    f0 = torch.arange(B * K * A * T, dtype=torch.float32).reshape(B, K, A, T)
    pitch = {"f0_clean": -torch.ones(B, T), "f0": f0}
    values = CP.stack_contours(pitch)
    assert values.shape == (B * (1 + K * A), T)
    names, sheets = CP.pitch_sheets(B, K, alphas, T, 0.032)
    per_item = [f"pc_{k}_pitch.png" for k in (1, 2, 3)] + ["pitch_comparison.png"]
    assert names == [(b, n) for b in range(B) for n in per_item] and len(sheets) == len(names)
    colours = CP.alpha_colours(A)
    for (b, name), s in zip(names, sheets):
        assert s.item == b and (s.sx, s.plot_height) == (8, 240)
        panels = list(s.panels)
        if name == "pitch_comparison.png":
            assert len(panels) == 1 + K and [c.row for c in panels[0].curves] == [b * 16]
            panels, ks = panels[1:], range(K)
        else:
            assert len(panels) == 1
            ks = [int(name.split("_")[1]) - 1]
        for p, k in zip(panels, ks):
            ref, var = p.curves[0], p.curves[1:]
            assert (ref.colour, ref.width) == (CP.INK, 2) and bool((values[ref.row] == -1).all())
            assert [c.colour for c in var] == colours and all(c.width == 1 for c in var)
            for a, c in enumerate(var):
                assert torch.equal(values[c.row], f0[b, k, a])
            assert list(p.legend) == [(colours[0], "-1"), (colours[2], "0"), (colours[4], "1")]           # every second alpha
            assert (p.ymin, p.ymax, list(p.yticks), p.xtick_every, p.markers) == (80.0, 400.0, [100.0, 200.0, 300.0, 400.0], 16, True)
    names, sheets = CP.pitch_sheets(1, 2, alphas, T, 0.032, individual=False, markers=False)
    assert names == [(0, "pitch_comparison.png")] and not sheets[0].panels[0].markers
