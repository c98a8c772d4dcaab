"""CPU: the serial PNG encoder (nppc_png_encode_host over csrc/png_core.h) gives byte for byte what the restatement
tests/png_ref.py gives; Pillow and zlib, which this project did not write, read the files back; the restatement's context
window and markers are checked against hand-worked gaps.  The device encoder's tile is 4096 bytes of filtered stream
(png_cases.TILE): `big`, `const2_big` and `twos_big` are six tiles each."""
import ctypes
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases
import png_ref as R
from nppc_audio import _hip as H
from nppc_audio import png

CASES = png_cases.cases()
PAL = png.palette("viridis")


@pytest.fixture(scope="module")
def encoded():
    """name -> the host encoder's bytes, encoded once and shared (read-only)"""
    names = list(CASES)
    blobs = png.encode_indexed([torch.from_numpy(CASES[n]) for n in names], PAL, backend="host")
    return dict(zip(names, blobs))


def test_the_cases_cover_what_they_are_there_for():
    assert {CASES[n].shape[::-1] for n in ("1x1", "1x5", "2x1", "3x1")} == {(1, 1), (1, 5), (2, 1), (3, 1)}
    assert CASES["big"].shape == (70, 300) and len(R.filtered(CASES["big"])) > 5 * png_cases.TILE == 5 * png.TILE
    kinds = lambda n: [t for t in R.tokens(R.filtered(CASES[n]))]
    # 1 + 259 bytes of 17 behind the filter byte: literal, match 258, then 0, 1, 2 literals, a match of 3, a second 258
    assert kinds("row259")[1:] == [("lit", 17), ("match", 258)]
    assert kinds("row260")[1:] == [("lit", 17), ("match", 258), ("lit", 17)]
    assert kinds("row261")[1:] == [("lit", 17), ("match", 258), ("lit", 17), ("lit", 17)]
    assert kinds("row517")[1:] == [("lit", 17), ("match", 258), ("match", 258)]
    assert kinds("row262")[1:] == [("lit", 17), ("match", 258), ("match", 3)]
    assert kinds("3x1") == [("lit", 2), ("lit", 5), ("lit", 5), ("lit", 5)]
    assert all(k == "lit" for k, _ in kinds("noise")) or sum(k == "match" for k, _ in kinds("noise")) < 3
    assert kinds("const2")[:2] == [("lit", 2), ("match", 41)]                  # row 0's run takes both filter bytes around it
    assert kinds("twos_big") == [("lit", 2)] + [("match", 258)] * (21069 // 258) + [("match", 21069 % 258)]
    assert {v for k, v in kinds("literals") if k == "lit"} == set(range(256))


@pytest.mark.parametrize("name", list(CASES))
def test_host_encoder_equals_the_restatement_and_decodes(encoded, name):
    idx, blob = CASES[name], encoded[name]
    h, w = idx.shape
    want = R.encode(idx, PAL)
    assert blob == want, f"first difference at byte {next((i for i, (a, b) in enumerate(zip(blob, want)) if a != b), min(len(blob), len(want)))}"
    assert len(blob) <= R.bound(w, h) == png.bound(w, h)
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "P" and im.size == (w, h)
    assert np.array_equal(np.asarray(im), idx)
    assert bytes(im.getpalette()[:768]) == PAL.tobytes()
    assert zlib.decompress(R.idat(blob)) == R.filtered(idx)


def test_noise_is_the_bounds_worst_case(encoded):
    h, w = CASES["noise"].shape
    assert R.bound(w, h) - len(encoded["noise"]) < (h * (w + 1)) // 8 + 8      # nearly every byte a 9- or 8-bit literal


def test_palettes():
    for name in ("viridis", "gray"):
        p = png.palette(name, marker=(1, 2, 3), background=(4, 5, 6))
        assert p.shape == (256, 3) and p.dtype == np.uint8 and p[254].tolist() == [1, 2, 3] and p[255].tolist() == [4, 5, 6]
    assert png.palette("viridis")[0].tolist() == [68, 1, 84] and png.palette("viridis")[253].tolist() == [253, 231, 37]
    assert png.palette("gray")[0].tolist() == [0, 0, 0] and png.palette("gray")[253].tolist() == [255, 255, 255]
    with pytest.raises(ValueError):
        png.palette("jet")


def test_symbols_are_declared_bound_and_refuse_bad_arguments(tmp_path):
    names = ["nppc_png_bound", "nppc_png_encode_host", "nppc_png_encode", "nppc_spec_windows", "nppc_spec_render",
             "nppc_spec_render_png"]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nppc_hip.h")).read()
    for n in names:
        assert n in H.SIGS and hasattr(H.lib(), n) and f"int {n}(" in header
    n = ctypes.c_long()
    H.call("nppc_png_bound", 64, 33, ctypes.byref(n))
    assert n.value == R.bound(64, 33) == 8 + 25 + 780 + 12 + (2 + (3 + 9 * 33 * 65 + 14) // 8 + 4) + 12
    bad = pytest.raises(RuntimeError, match="bad argument")
    for w, h in ((0, 1), (1, 0), (16385, 1), (1, 16385), (16384, 8192)):
        with bad:
            H.call("nppc_png_bound", w, h, ctypes.byref(n))
    with bad:
        H.call("nppc_png_bound", 4, 4, None)
    idx, out = np.zeros((4, 4), np.uint8), np.zeros(2048, np.uint8)
    with bad:                                                                   # cap below the bound
        H.call("nppc_png_encode_host", idx.ctypes.data, 4, 4, PAL.ctypes.data, out.ctypes.data, R.bound(4, 4) - 1, ctypes.byref(n))
    with bad:
        H.call("nppc_png_encode_host", None, 4, 4, PAL.ctypes.data, out.ctypes.data, 2048, ctypes.byref(n))
    with bad:                                                                   # null pointers, empty batches: before any launch
        H.call("nppc_png_encode", None, 1, None, 1, None, None, 1, None, None, None, None, None, 1, None)
    with bad:
        H.call("nppc_png_encode", 8, 1, 8, 0, 8, 8, 1, 8, 8, 8, 8, 8, 8, None)
    with bad:
        H.call("nppc_spec_windows", None, 1, 1, None, None)
    with bad:
        H.call("nppc_spec_windows", 8, 0, 1, 8, None)
    with bad:
        H.call("nppc_spec_render", None, 1, 1, 1, 1, 1, None, 1, None, 1, None, None, None, None, 1, 1, None)
    with bad:
        H.call("nppc_spec_render", 8, 1, 1, 3, 1, 1, 8, 1, 8, 1, 8, 8, 8, 8, 1, 1, None)              # CH = 3
    with bad:
        H.call("nppc_spec_render", 8, 1, 1, 1, 1, 1, 8, 1, 8, 1, 8, 8, 8, 8, 1, (1 << 26) + 1, None)   # oversize
    with bad:
        H.call("nppc_spec_render_png", 8, 1, 1, 1, 1, 1, 8, 1, 8, 1, 8, 8, 8, 8, 1, 1, 8, 8, 0, 8, 8, 8, 8, 8, 8, None)
    for images in ([torch.zeros(0, 3, dtype=torch.uint8)], [torch.zeros(3, 3)], torch.zeros(3, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            png.encode_indexed(images, PAL, backend="host")
    with pytest.raises(ValueError):
        png.encode_indexed([torch.zeros(3, 3, dtype=torch.uint8)], PAL[:255], backend="host")
    png.write_files([tmp_path / "a" / "x.png"], [b"abc"])
    assert (tmp_path / "a" / "x.png").read_bytes() == b"abc"
    with pytest.raises(ValueError):
        png.write_files([tmp_path / "y.png"], [])


def test_context_window_and_markers_of_the_restatement():
    def mask(n, s, e):
        m = np.ones(n)
        m[s:e] = 0
        return m
    # a 4-frame gap [10, 14) in the middle of 40 frames: 4 frames of context on each side
    assert R.window(mask(40, 10, 14)) == (6, 18, 10, 14)
    # at the start: the left context is clamped; at the end: the right one, and the closing marker lies outside the window
    assert R.window(mask(40, 0, 5)) == (0, 10, 0, 5)
    assert R.window(mask(40, 1, 6)) == (0, 11, 1, 6)
    assert R.window(mask(40, 37, 40)) == (34, 40, 37, 40)
    assert R.window(mask(40, 30, 36)) == (24, 40, 30, 36)
    assert R.window(np.ones(40)) == (0, 40, -1, -1)
    assert R.window(mask(40, 0, 40)) == (0, 40, 0, 40)

    # markers on a 2 x 2 sheet: F = 9 rows of sy = 1, the marker frames' first pixel column, rows 0-3 and 8 of every cell
    from nppc_audio.spectrogram_png import Cell, Sheet
    planes = np.zeros((1, 1, 1, 9, 40), np.float32)
    cell = Cell(p=0, vmin=-1.0, vmax=1.0, markers=True)
    sheet = Sheet(0, [[cell, None], [Cell(p=0, vmin=-1.0, vmax=1.0), cell]], sx=2, sy=1, gutter=3)
    img = R.render(planes, sheet, R.window(mask(40, 10, 14)))
    assert img.shape == (2 * 9 + 3, 2 * 24 + 3)
    dashed = [0, 1, 2, 3, 8]
    assert (img[dashed, 8] == 254).all() and (img[dashed, 16] == 254).all() and (img[[4, 5, 6, 7], 8] == 127).all()
    assert (img[:9, 9] == 127).all() and (img[:9, 24:] == 255).all() and (img[9:12] == 255).all()
    assert (img[12:, :24] == 127).all() and (img[[12 + r for r in dashed], 27 + 8] == 254).all()
