"""GPU: the spectrogram renderer (csrc/spec_png.hip, nppc_audio/spectrogram_png.py) against the restatement tests/png_ref.py.

Real planes: the index images equal the fp32 restatement exactly (every operation is a separately rounded fp32 operation on
both sides).  dB planes: every pixel's [idx, idx + 1] contains the fp64 position (dB - vmin) 254 / (vmax - vmin), clamped to
[0, 254], to within EPS = 2e-3 levels: an fp32 chain of about eight roundings on values up to 160 dB moves a pixel by about
3e-4 levels at 0.24 dB per level, the rest is margin for the device's log10f.  Every test runs under a time limit of its own.
"""
import faulthandler
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R
from nppc_audio import png
from nppc_audio.spectrogram_png import Cell, Sheet, render_indices, render_png, windows_from_mask

pytestmark = pytest.mark.gpu
LIMIT = 120
EPS = 2e-3
F, T, B, K = 9, 12, 3, 2
ALPHAS = (-1.5, 0.0, 2.0)
WIN = [(3, 4, -1, -1), (2, 7, 3, 5), (0, 12, 4, 9)]                          # widths 1, 5 and 12
CLEAN, PRED, PC = 0, 1, 2                                                     # planes: clean, pred, pc_1 .. pc_K


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def real_planes():
    rng = np.random.default_rng(2)
    x = (2.0 * rng.standard_normal((B, 2 + K, 1, F, T))).astype(np.float32)   # well outside [-3, 3] here and there
    x[:, CLEAN, 0, 0, :] = 3.0                                                 # exactly vmax
    x[:, CLEAN, 0, 1, :] = -3.0                                                # exactly vmin
    x[:, CLEAN, 0, 2, :] = np.float32(-3.0) + np.float32(6.0 / 254.0) * np.arange(T, dtype=np.float32)   # on the level edges
    x[:, PRED, 0, 3, ::2] = np.nan
    x[:, PRED, 0, 4, :] = [9.0, -9.0, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-30, 3.0000002, 2.9999998, -3.0000002]
    x[:, PC, 0, 5, 1::3] = np.nan
    return x


def inpainting_sheet(b, sx, sy, gutter=2):
    rng_, err = dict(vmin=-3.0, vmax=3.0), dict(vmin=0.0, vmax=3.0)
    top = [Cell(p=CLEAN, markers=True, **rng_), Cell(p=PRED, markers=True, **rng_),
           Cell(p=CLEAN, q=PRED, alpha=-1.0, g="abs", markers=True, **err), None]
    rows = [top]
    for k in range(K):
        rows.append([Cell(q=PC + k, **rng_)] + [Cell(p=PRED, q=PC + k, alpha=a, markers=True, **rng_) for a in ALPHAS])
    return Sheet(b, rows, sx=sx, sy=sy, gutter=gutter)


def test_real_planes_equal_the_fp32_restatement_exactly():
    x = real_planes()
    sheets = [inpainting_sheet(b, sx, sy) for b in range(B) for sx in (1, 2, 3) for sy in (1, 2, 3)]
    win = torch.tensor(WIN, dtype=torch.int32).cuda()
    got = render_indices(torch.from_numpy(x).cuda(), sheets, win)
    seen = set()
    for s, g in zip(sheets, got):
        want = R.render(x, s, WIN[s.item])
        g = g.cpu().numpy()
        assert g.shape == want.shape, (s.item, s.sx, s.sy)
        assert np.array_equal(g, want), (s.item, s.sx, s.sy, np.argwhere(g != want)[:5].tolist())
        seen |= set(np.unique(g).tolist())
    assert {0, 253, 254, 255} <= seen and len(seen) > 100                      # both clamps, markers, background and the ramp
    # the values the test is there for: below vmin, above vmax, exactly vmax, NaN
    one = render_indices(torch.from_numpy(x).cuda(), [Sheet(2, [[Cell(p=CLEAN, vmin=-3.0, vmax=3.0), Cell(p=PRED, vmin=-3.0, vmax=3.0)]])],
                         win)[0].cpu().numpy()
    assert (one[F - 1, :T] == 253).all() and (one[F - 2, :T] == 0).all()       # bin 0 is the bottom row
    assert (one[F - 1 - 3, T:][::2] == 0).all()                                # NaN
    assert one[F - 1 - 4, T:].tolist()[:6] == [253, 0, 253, 0, 253, 0]


def db_planes():
    rng = np.random.default_rng(3)
    mag = 10.0 ** rng.uniform(-6.0, 1.0, (B, 3, F, T))
    ph = rng.uniform(0, 2 * np.pi, mag.shape)
    z = np.stack([mag * np.cos(ph), mag * np.sin(ph)], axis=2).astype(np.float32)          # [B, 3, 2, F, T]
    z[:, :, :, ::4, ::3] = 0.0                                                              # exact zeros: 1e-8 matters
    z[:, 2] = 0.25                                                                          # a constant plane
    return z


@pytest.mark.parametrize("rng_", [(-60.0, 0.0), (float("nan"), float("nan"))], ids=["minus60_0", "autoscale"])
def test_db_planes_lie_within_eps_levels_of_the_fp64_position(rng_):
    z = db_planes()
    cells = [Cell(p=0, g="db", vmin=rng_[0], vmax=rng_[1]), Cell(p=0, q=1, alpha=-1.0, g="db", vmin=rng_[0], vmax=rng_[1]),
             Cell(q=1, alpha=2.5, g="db", vmin=rng_[0], vmax=rng_[1])]
    sheets = [Sheet(b, [cells]) for b in range(B)]
    win = torch.tensor(WIN, dtype=torch.int32).cuda()
    got = render_indices(torch.from_numpy(z).cuda(), sheets, win)
    worst, pixels = 0.0, 0
    for s, g in zip(sheets, got):
        t0, t1 = WIN[s.item][:2]
        g = g.cpu().numpy().astype(np.float64)
        for c, cell in enumerate(cells):
            pos, _, _ = R.positions(z, s.item, cell, t0, t1)
            pos = np.clip(pos[::-1], 0.0, 254.0)                                            # bin 0 at the bottom
            idx = g[:, c * (t1 - t0):(c + 1) * (t1 - t0)]
            assert idx.max() <= 253
            worst = max(worst, float(np.maximum(idx - pos, pos - (idx + 1)).max()))
            pixels += idx.size
    print(f"dB {rng_}: largest excess over [idx, idx + 1] {worst:.3e} levels on {pixels} pixels")
    assert worst <= EPS, worst


def test_a_constant_autoscaled_panel_is_all_zeros():
    z = db_planes()
    for cell in (Cell(p=2, g="db"), Cell(p=2, g="abs"), Cell(p=2)):
        got = render_indices(torch.from_numpy(z).cuda(), [Sheet(1, [[cell]], sx=2, sy=2)])[0]
        assert got.shape == (2 * F, 2 * T) and int(got.max()) == 0


def test_sheet_geometry_gutters_blanks_markers_and_bin_0_at_the_bottom():
    x = np.zeros((1, 2, 1, F, 40), np.float32)
    x[0, 0, 0] = np.arange(F, dtype=np.float32)[:, None]                       # plane 0: the bin's number
    x[0, 1, 0] = np.arange(40, dtype=np.float32)[None, :]                      # plane 1: the frame's number
    mask = torch.ones(1, 40)
    mask[0, 10:14] = 0
    win = windows_from_mask(mask.cuda())
    assert win.cpu().tolist() == [[6, 18, 10, 14]] == [list(R.window(mask[0].numpy()))]
    sx, sy, gut = 2, 3, 5
    cw, ch = 12 * sx, F * sy
    bins, frames = Cell(p=0, vmin=0.0, vmax=float(F), markers=True), Cell(p=1, vmin=0.0, vmax=254.0)
    sheet = Sheet(0, [[bins, None, frames], [None, bins, None]], sx=sx, sy=sy, gutter=gut)
    g = render_indices(torch.from_numpy(x).cuda(), [sheet], win)[0].cpu().numpy()
    assert g.shape == (2 * ch + gut, 3 * cw + 2 * gut)
    assert np.array_equal(g, R.render(x, sheet, (6, 18, 10, 14)))
    assert (g[ch:ch + gut] == 255).all() and (g[:, cw:cw + gut] == 255).all() and (g[:, 2 * cw + gut:2 * cw + 2 * gut] == 255).all()
    assert (g[:ch, cw + gut:2 * cw + gut] == 255).all() and (g[ch + gut:, :cw] == 255).all()             # blank cells
    level = lambda f: int(np.floor(np.float32(f) * np.float32(254.0 / F)))
    assert g[ch - 1, 1] == level(0) == 0 and g[0, 1] == level(F - 1) and g[ch - sy, 1] == 0 and g[ch - sy - 1, 1] == level(1)
    cols = [(10 - 6) * sx, (14 - 6) * sx]
    dashed = (np.arange(ch) // 4) % 2 == 0
    for c in cols:
        assert (g[:ch][dashed, c] == 254).all() and (g[:ch][~dashed, c] != 254).all() and (g[:ch, c + 1] != 254).all()
        assert (g[ch + gut:][dashed, cw + gut + c] == 254).all()
    assert (g[:ch, 2 * cw + 2 * gut:] != 254).all()                            # a cell that asks for no markers
    assert g[3, 2 * cw + 2 * gut:].tolist() == [t for t in range(6, 18) for _ in range(sx)]              # frames left to right
    # an item without a gap: the whole clip, no marker
    whole = windows_from_mask(torch.ones(1, 40).cuda())
    assert whole.cpu().tolist() == [[0, 40, -1, -1]]
    g = render_indices(torch.from_numpy(x).cuda(), [Sheet(0, [[bins]])], whole)[0]
    assert g.shape == (F, 40) and int((g == 254).sum()) == 0


def test_png_path_decodes_to_the_indices_and_a_batch_equals_its_items_alone():
    x = torch.from_numpy(real_planes()).cuda()
    sheets = [inpainting_sheet(b, sx, sy, gutter=b) for b, sx, sy in ((0, 1, 1), (1, 2, 3), (2, 3, 2), (1, 1, 2))]
    win = torch.tensor(WIN, dtype=torch.int32).cuda()
    files = render_png(x, sheets, win)
    idx = render_indices(x, sheets, win)
    pal = png.palette("viridis")
    for f, i in zip(files, idx):
        im = Image.open(io.BytesIO(f))
        assert im.mode == "P" and im.size == (i.shape[1], i.shape[0])
        assert np.array_equal(np.asarray(im), i.cpu().numpy())
        assert bytes(im.getpalette()[:768]) == pal.tobytes()
    assert png.encode_indexed(idx, pal, backend="host") == files                # the fused path writes the host encoder's bytes
    assert render_png(x, sheets, win) == files                                  # run after run
    for s, f in zip(sheets, files):
        assert render_png(x, [s], win) == [f]                                   # alone as in the batch
    # windows narrower than max_frames fit; a wider one is refused
    assert render_png(x, sheets[:1], win, max_frames=1) == files[:1]
    with pytest.raises(ValueError):
        render_png(x, sheets[1:2], win, max_frames=4)
