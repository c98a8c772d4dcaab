"""CPU: the host half of whole-recording restoration: plan_windows against the restatement
(tests/restore_ref.py) and its error cases, the restatement's own properties on constructed signals, the configuration, the
declarations, and the no-gap path of RecordingRestorer.restore."""
import os
import re

import numpy as np
import pytest
import torch

import restore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN, XF, NFFT, HOP = 8192, 64, 255, 128
KW = dict(window_samples=WIN, crossfade_samples=XF, n_fft=NFFT, hop_length=HOP)


def plan_windows(length, gaps, **kw):
    from nppc_audio.inpainting.restore import plan_windows as pw
    return pw(length, gaps, **{**KW, **kw})


def span_cap():
    from nppc_audio.inpainting.phase import gl_gap_shape
    return gl_gap_shape(1, 1, NFFT // 2 + 1, 1 + WIN // HOP, NFFT, HOP, length=WIN, n_iter=0)["span_cap"]


def check_against_restatement(length, gaps):
    got = plan_windows(length, gaps)
    want = R.plan(length, gaps, WIN, XF, NFFT, HOP, span_cap())
    assert len(got) == len(want)
    for g, (ws, own, fm) in zip(got, want):
        assert g["start"] == ws and tuple(g["gap"]) == own
        sm = np.ones(WIN)
        for a, b in g["masked"]:
            sm[a:b] = 0
        assert np.array_equal(R.frame_mask(sm, NFFT, HOP), fm)
        gone = np.flatnonzero(fm == 0)
        assert g["frames"] == (gone[0], gone[-1])
    return got


def test_plan_merges_gaps_closer_than_two_crossfades():
    got = check_against_restatement(24000, [(12000, 12500), (12500 + 2 * XF - 1, 13000), (5000, 5600)])
    assert [p["gap"] for p in got] == [(5000, 5600), (12000, 13000)]
    got = check_against_restatement(40000, [(12000, 12500), (30000, 30400), (12500 + 2 * XF, 13000)])
    assert [p["gap"] for p in got] == [(12000, 12500), (12500 + 2 * XF, 13000), (30000, 30400)]
    assert plan_windows(24000, [(12000, 12600), (12100, 12300)])[0]["gap"] == (12000, 12600)       # nested
    assert plan_windows(24000, []) == [] and plan_windows(10, []) == []


def test_plan_centres_and_clamps_at_both_ends():
    got = check_against_restatement(24000, [(500, 1524), (11500, 12524), (22000, 23024)])
    assert [p["start"] for p in got] == [0, 12012 - WIN // 2, 24000 - WIN]
    assert [p["masked"] for p in got] == [[(500, 1524)], [(11500 - 7916, 12524 - 7916)], [(22000 - 15808, 23024 - 15808)]]
    one = check_against_restatement(WIN, [(4000, 5000)])                              # length == window_samples
    assert one[0]["start"] == 0


def test_plan_masks_a_foreign_gap_in_the_window_but_owns_each_gap_once():
    # 1400 samples apart: both fit one span of 30 masked frames, each is centred in its own window, masked in the other's
    gaps = [(10000, 10400), (11800, 12200)]
    got = check_against_restatement(30000, gaps)
    assert [p["gap"] for p in got] == gaps
    for p, other in zip(got, gaps[::-1]):
        ws = p["start"]
        assert (other[0] - ws, other[1] - ws) in p["masked"] and len(p["masked"]) == 2


@pytest.mark.parametrize("gap,word", [((5, 5), r"\(5, 5\)"), ((7, 3), r"\(7, 3\)"), ((-4, 9), r"\(-4, 9\)"),
                                      ((23000, 24001), r"\(23000, 24001\)")])
def test_plan_rejects_bad_pairs_by_name(gap, word):
    with pytest.raises(ValueError, match=word):
        plan_windows(24000, [(1000, 1500), gap])
    with pytest.raises(ValueError, match="gap"):
        R.plan(24000, [gap], WIN, XF, NFFT, HOP, 32)


def test_plan_error_cases():
    with pytest.raises(ValueError, match="fewer than one window"):
        plan_windows(WIN - 1, [(100, 200)])
    with pytest.raises(ValueError, match="not a .start, end. pair"):
        plan_windows(24000, [5])
    # a gap at the very start: no known frame on its left (and one that leaves a single known frame)
    for gap in ((0, 600), (130, 700), (23500, 24000)):
        with pytest.raises(ValueError, match="fewer than 2 known frames"):
            plan_windows(24000, [gap])
        with pytest.raises(ValueError, match="known frames"):
            R.plan(24000, [gap], WIN, XF, NFFT, HOP, span_cap())
    ok = plan_windows(24000, [(256 + 127, 900)])                                     # frames 0 and 1 stay known
    assert ok[0]["frames"][0] == 2
    # too long for Griffin-Lim's span: checked here, with gl_gap_shape's cap, never by the kernel
    cap = span_cap()
    long_gap = (10000, 10000 + (cap - 2) * HOP)
    with pytest.raises(ValueError, match=f"span cap of {cap}"):
        plan_windows(24000, [long_gap])
    with pytest.raises(ValueError, match="span cap"):
        R.plan(24000, [long_gap], WIN, XF, NFFT, HOP, cap)
    fits = (10000, 10000 + (cap - 4) * HOP)
    assert plan_windows(24000, [fits])[0]["frames"][1] - plan_windows(24000, [fits])[0]["frames"][0] + 1 + 2 <= cap
    with pytest.raises(ValueError, match="span cap"):                                  # two gaps far apart inside one window
        plan_windows(24000, [(10000, 10400), (13600, 14000)])
    with pytest.raises(ValueError, match="span cap"):
        R.plan(24000, [(10000, 10400), (13600, 14000)], WIN, XF, NFFT, HOP, cap)
    with pytest.raises(ValueError, match="crossfade"):
        plan_windows(24000, [(11500, 12524)], crossfade_samples=4000)
    with pytest.raises(ValueError, match="does not fit a window"):
        plan_windows(24000, [(3000, 3000 + WIN + 2)])


# ---- the restatement on constructed signals -------------------------------------------------------------------------
def test_restated_crossfade_is_continuous_and_hits_the_window_output_on_the_gap():
    L, s, e, ws, g = 4000, 1500, 2100, 1000, 2.5
    rec = np.full(L, 0.25, np.float32)
    wout = np.full((1, 2, 2000), -1.0 * g, np.float32)
    wout[0, 1] = 3.0 * g
    out = R.splice(rec, [(s, e)], [ws], wout, g, XF)
    assert out.shape == (2, L)
    for v, y in ((0, -1.0), (1, 3.0)):
        assert np.array_equal(out[v, s:e], np.full(e - s, y))                          # exactly the window output / gain
        assert np.array_equal(out[v, :s - XF], rec[:s - XF]) and np.array_equal(out[v, e + XF:], rec[e + XF:])
        ramp = out[v, s - XF - 1:s + 1]
        step = np.abs(np.diff(ramp)).max()
        assert step <= abs(y - 0.25) * np.pi / (2 * (XF + 1)) * 1.0001               # no step larger than the cosine's slope
        assert np.all(np.diff(ramp) * np.sign(y - 0.25) > 0)                           # monotone from recording to output
        assert np.allclose(out[v, s - XF:s][::-1], out[v, e:e + XF], rtol=0, atol=1e-15)   # the two ramps mirror each other
    assert 0 < R.crossfade_weight(0, XF) < 2e-3 and 1 - 2e-3 < R.crossfade_weight(XF - 1, XF) < 1
    # clipped at sample 0 and at L; a gap next to the window's edge keeps the recording outside the window
    out = R.splice(rec, [(10, 300), (3900, 3990)], [0, 2000], np.full((2, 1, 2000), 1.0, np.float32), 1.0, XF)
    assert np.array_equal(out[0, 10:300], np.ones(290)) and out[0, 0] == 0.25 + R.crossfade_weight(XF - 10, XF) * 0.75
    assert np.array_equal(out[0, 3900:3990], np.ones(90)) and out.shape == (1, L)
    assert np.array_equal(R.spliced_region(L, [(10, 300), (3900, 3990)], XF), out[0] != 0.25)


@pytest.mark.parametrize("name", list(R.ZERO_RUN_CASES))
def test_restated_zero_runs(name):
    x, min_len = R.ZERO_RUN_CASES[name]
    got = R.zero_runs(x, min_len)
    want = {"touches_both_ends": [(0, 200), (2800, 3000)], "one_short_of_min_len": [(1000, 1160)],
            "split_by_one_sample": [(500, 700), (701, 900)],
            "straddles_chunks": [(R.CHUNK - 1, R.CHUNK + 1), (2 * R.CHUNK - 300, 2 * R.CHUNK + 1)],
            "whole_chunk_and_edges": [(R.CHUNK - 1, 2 * R.CHUNK + 1), (3 * R.CHUNK - 1, 3 * R.CHUNK + 1)],
            "all_zero": [(0, 2 * R.CHUNK + 1)], "no_zero": [], "negative_zero": [(100, 300)]}
    if name in want:
        assert got == want[name]
    else:
        assert got == [(a, a + 3) for a in range(1, R.CHUNK - 4, 7)]
    # against a vectorised formulation
    z = np.concatenate([[0], (x == 0).astype(np.int8), [0]])
    d = np.diff(z)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    assert got == [(int(a), int(b)) for a, b in zip(starts, ends) if b - a >= min_len]


def test_restated_gain_and_windows():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(24000) * 0.05).astype(np.float32)
    gaps = [(500, 1524), (11500, 12524)]
    g = R.gain(x, gaps)
    filled = x.copy()
    filled[500:1524] = 9.0                                                            # what the gaps hold does not matter
    assert R.gain(filled, gaps) == g
    known = np.ones(24000, bool)
    known[500:1524] = known[11500:12524] = False
    rms = np.sqrt(np.mean((x[known].astype(np.float64) * g) ** 2))
    rms_in = np.sqrt(np.mean(x[known].astype(np.float64) ** 2))
    # the known samples sit at -25 dBFS, less what the 1e-8 next to the RMS takes
    assert abs(20 * np.log10(rms) + 25.0 + 20 * np.log10(1 + 1e-8 / rms_in)) < 1e-9
    w, m = R.windows(filled, gaps, [0, 7916], WIN, g)
    assert np.array_equal(m[0] == 0, ~known[:WIN]) and np.array_equal(w[0][~known[:WIN]], np.zeros(1024))
    assert np.array_equal(w[1], x[7916:7916 + WIN].astype(np.float64) * g * known[7916:7916 + WIN])


# ---- the package's host side ---------------------------------------------------------------------------------------------
def model_configuration(path="restorer.pt", K=2):
    return dict(pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2),
                pretrained_restoration_model_path=path,
                audio_pc_wrapper_configuration=dict(n_dirs=K, model_configuration=dict(in_channels=2, out_channels=K)),
                device="cuda")


def test_config_round_trip_and_defaults():
    from nppc_audio.inpainting.restore import RecordingRestorerConfig
    c = RecordingRestorerConfig(checkpoint_path="nppc.pt", model_configuration=model_configuration())
    assert (c.window_samples, c.n_fft, c.hop_length, c.target_dB_FS) == (32704, 255, 128, -25.0)
    assert (c.gl_iters, c.momentum, c.crossfade_samples, c.min_gap_samples, c.device) == (32, 0.0, 64, 160, "cuda")
    c2 = RecordingRestorerConfig(**c.model_dump())
    assert c2 == c and RecordingRestorerConfig.model_validate_json(c.model_dump_json()) == c
    c3 = RecordingRestorerConfig(checkpoint_path="x", model_configuration=model_configuration(), window_samples=8192, gl_iters=4)
    assert c3.window_samples == 8192 and c3.model_dump()["gl_iters"] == 4
    with pytest.raises(Exception):
        RecordingRestorerConfig(model_configuration=model_configuration())


def test_restore_without_gaps_returns_the_input_and_needs_no_gpu():
    from nppc_audio.inpainting.restore import RecordingRestorer, RecordingRestorerConfig
    r = RecordingRestorer.__new__(RecordingRestorer)                                    # no checkpoint, no model, no device
    r.config = RecordingRestorerConfig(checkpoint_path="x", model_configuration=model_configuration())
    r.device = "cpu"
    x = torch.randn(1000)                                                               # shorter than a window: still fine
    keep = x.clone()
    out = r.restore(x, [])
    assert torch.equal(out["restored"], keep) and out["windows"] == [] and out["status"] is None
    with pytest.raises(ValueError, match=r"\(10, 2000\)"):
        r.restore(x, [(10, 2000)])
    with pytest.raises(ValueError, match="variations"):
        r.restore(x, [], variations="all")
    with pytest.raises(ValueError, match="one channel"):
        r.restore(torch.zeros(2, 1000), [])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):                                  # no fall-back: a gap needs the device
            r.restore(torch.randn(40000), [(20000, 21000)])
        with pytest.raises(RuntimeError, match="HIP"):
            r.detect_gaps(torch.zeros(1000))


def test_new_symbols_are_declared_bound_and_exported():
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import restore as RS
    txt = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    fns = {m.group(1): [a for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
           for m in re.finditer(r"\bint\s+(nppc_\w+)\s*\((.*?)\)\s*;", bare, flags=re.S)}
    for name in ("nppc_rec_gain", "nppc_rec_windows", "nppc_rec_splice", "nppc_zero_runs"):
        assert name in fns and len(fns[name]) == len(H.SIGS[name]), name
        assert hasattr(H.lib(), name), f"{name} not exported by libnppc_hip.so"
    assert int(re.search(r"#define\s+NPPC_REC_GAIN_WORK\s+(\d+)", txt).group(1)) == RS.REC_GAIN_WORK
    assert int(re.search(r"#define\s+NPPC_ZERO_RUN_CHUNK\s+(\d+)", txt).group(1)) == RS.ZERO_RUN_CHUNK == R.CHUNK
    with pytest.raises(RuntimeError, match="bad argument"):                             # refused before any launch
        H.call("nppc_rec_gain", None, 100, None, 0, -25.0, None, None, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_rec_windows", None, 100, None, 1, None, 1, 64, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_rec_splice", None, 100, None, None, 1, None, 0, 0, 64, 1, 8, None, None, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_zero_runs", None, 100, 1, None, 0, None, 0, None, None)
