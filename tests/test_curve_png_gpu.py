"""GPU: the curve-sheet kernels (csrc/curve_png.hip, nppc_audio/curve_png.py) against the restatement tests/curve_ref.py on
the cases of tests/curve_cases.py: the device index images equal the restatement exactly, the device PNG bytes equal the
host encoder's, a sheet alone equals the same sheet in a batch, two runs are identical.  Every test runs under a time limit
of its own."""
import faulthandler
import io

import numpy as np
import pytest
import torch
from PIL import Image

import curve_cases
import curve_ref as R
from nppc_audio import curve_png as CP
from nppc_audio import png

pytestmark = pytest.mark.gpu
LIMIT = 120
CASES = curve_cases.cases()


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def wanted():
    """name -> the restatement's images, computed once and shared (read-only)"""
    return {n: [R.render(v, s, w[s.item]) for s in sheets] for n, (v, sheets, w) in CASES.items()}


def on_device(name):
    v, sheets, w = CASES[name]
    return torch.from_numpy(v).cuda(), sheets, torch.tensor(w, dtype=torch.int32).cuda()


@pytest.mark.parametrize("T", curve_cases.TS)
def test_device_index_images_equal_the_restatement_exactly(wanted, T):
    names = [n for n in CASES if n.startswith(f"T{T}_")] + (["bare"] if T == 3 else [])
    assert names
    for name in names:
        v, sheets, win = on_device(name)
        got = CP.render_indices(v, sheets, win)
        for s, g, want in zip(sheets, got, wanted[name]):
            g = g.cpu().numpy()
            assert g.shape == want.shape, (name, s.item)
            assert np.array_equal(g, want), (name, s.item, np.argwhere(g != want)[:5].tolist())


def test_a_ragged_batch_of_every_case_at_once(wanted):
    """sheets of different items, windows, scales and sizes in one call: windows of 1, 6 and 12 frames under max_frames 12"""
    names = [n for n in CASES if n.startswith("T12_")]
    v = torch.from_numpy(CASES[names[0]][0]).cuda()
    win = torch.tensor(CASES[names[0]][2], dtype=torch.int32).cuda()
    sheets = [s for n in names for s in CASES[n][1]]
    want = [w for n in names for w in wanted[n]]
    got = CP.render_indices(v, sheets, win, max_frames=12)
    assert len(got) == len(want) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_png_bytes_equal_the_host_encoders_alone_as_in_a_batch_and_run_after_run(wanted):
    name = "T12_sx3_h64_g2"
    v, sheets, win = on_device(name)
    pal = CP.plot_palette()
    files = CP.render_png(v, sheets, win, backend="hip")
    assert files == png.encode_indexed([torch.from_numpy(w) for w in wanted[name]], pal, backend="host")
    assert files == CP.render_png(v.cpu(), sheets, win.cpu(), backend="host")               # the serial renderer and encoder
    assert CP.render_png(v, sheets, win, backend="hip") == files                            # run after run
    for s, f in zip(sheets, files):
        assert CP.render_png(v, [s], win, backend="hip") == [f]                             # alone as in the batch
    for f, w in zip(files, wanted[name]):
        im = Image.open(io.BytesIO(f))
        assert im.mode == "P" and np.array_equal(np.asarray(im), w) and bytes(im.getpalette()[:768]) == pal.tobytes()
    # windows narrower than max_frames fit; a wider one is refused
    assert CP.render_png(v, sheets[1:2], win, max_frames=1, backend="hip") == files[1:2]
    with pytest.raises(ValueError):
        CP.render_png(v, sheets[2:3], win, max_frames=4, backend="hip")


def test_refusals_come_before_any_launch():
    v = torch.zeros(2, 5000, device="cuda")
    with pytest.raises(ValueError, match="16384"):
        CP.render_png(v, [CP.CurveSheet(0, [CP.Panel([CP.Curve(0, 1)] * 4, 0.0, 1.0)], 1, 8)])
    with pytest.raises(ValueError, match="wider or higher"):
        CP.render_png(v, [CP.CurveSheet(0, [CP.Panel([CP.Curve(0, 1)], 0.0, 1.0)], 4, 8)])
