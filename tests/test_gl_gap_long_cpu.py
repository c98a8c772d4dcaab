"""CPU: the host half of Griffin-Lim's tiled long-span path (csrc/gl_gap_long.hip): the declarations,
the argument rules of nppc_gl_gap_long_shape against those of nppc_gl_gap_shape, the defaults of the new options, and
plan_windows with long_gaps=True."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nppc_gl_gap_long_shape", "nppc_gl_gap_long", "nppc_gl_gap_pc_long")


def header_functions():
    txt = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): [a for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(nppc_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_new_symbols_are_declared_bound_and_exported():
    from nppc_audio import _hip as H
    fns = header_functions()
    for name in NEW:
        assert name in fns and len(fns[name]) == len(H.SIGS[name]), name
        assert hasattr(H.lib(), name), f"{name} not exported by libnppc_hip.so"
    # the tiled entry points take what the resident ones take, plus long_max_span and mode in front of the stream
    assert len(H.SIGS["nppc_gl_gap_long"]) == len(H.SIGS["nppc_gl_gap"]) + 2
    assert len(H.SIGS["nppc_gl_gap_pc_long"]) == len(H.SIGS["nppc_gl_gap_pc"]) + 2
    with pytest.raises(RuntimeError, match="bad argument"):                     # null pointers are refused before any launch
        H.call("nppc_gl_gap_long", None, None, None, None, 0, None, None, None, None, None, 0, 1, 1, 40, 255, 128, 4993, 1, 0.0,
               0, 0, 1, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_gl_gap_pc_long", None, None, None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 1, 40,
               255, 128, 4993, 1, 0.0, 0, 0, 2, None)


GOOD = [dict(B=16, V=66, F=128, T=256), dict(B=1, V=1, F=128, T=40, n_iter=0), dict(B=3, V=3, F=128, T=64, momentum=0.99),
        dict(B=1, V=1, F=257, T=48, n_fft=512, hop_length=256, momentum=0.99), dict(B=1, V=1, F=256, T=48, n_fft=510, hop_length=256),
        dict(B=2, V=5, F=33, T=80, n_fft=64, hop_length=16), dict(B=1, V=1, F=128, T=256, max_span=19),
        dict(B=1, V=1, F=2, T=2, n_fft=2, hop_length=2, length=2, n_iter=0)]
BAD = [dict(B=1, V=1, F=129, T=40), dict(B=1, V=1, F=128, T=40, length=128 * 40), dict(B=1, V=1, F=128, T=40, length=128 * 39 - 1),
       dict(B=1, V=1, F=51, T=40, n_fft=100, hop_length=12), dict(B=1, V=1, F=513, T=40, n_fft=1024, hop_length=256),
       dict(B=1, V=1, F=128, T=40, n_iter=-1), dict(B=1, V=1, F=128, T=40, momentum=-0.1),
       dict(B=1, V=1, F=128, T=40, momentum=float("nan")), dict(B=1, V=1, F=128, T=40, max_span=2),
       dict(B=0, V=1, F=128, T=40), dict(B=1, V=70000, F=128, T=40), dict(B=1, V=1, F=128, T=40, hop_length=0),
       dict(B=1, V=1, F=128, T=1, length=100)]


def test_long_shape_accepts_and_refuses_what_the_resident_shape_does():
    from nppc_audio.inpainting.phase import gl_gap_shape
    for kw in GOOD:
        a, b = gl_gap_shape(**kw), gl_gap_shape(long_spans=True, **kw)
        for k in ("length", "r", "span_cap", "lds_bytes"):
            assert a[k] == b[k], (kw, k)
        assert b["long_span_cap"] >= kw["T"] and b["work_bytes"] > a["work_bytes"], kw      # spans up to T, both paths' workspace
        assert gl_gap_shape(long_spans="always", **kw) == b
    for kw in BAD:
        with pytest.raises(ValueError) as e0:
            gl_gap_shape(**kw)
        for mode in (True, "always"):
            with pytest.raises(ValueError) as e1:
                gl_gap_shape(long_spans=mode, **kw)
            assert str(e1.value) == str(e0.value), kw


def test_long_max_span_sizes_the_workspace_and_has_rules_of_its_own():
    from nppc_audio.inpainting.phase import gl_gap_shape
    full = gl_gap_shape(4, 8, 128, 256, long_spans=True)
    small = gl_gap_shape(4, 8, 128, 256, long_spans=True, long_max_span=35)
    assert full["long_span_cap"] == 256 + 2 * full["r"] and small["long_span_cap"] == 35
    assert small["work_bytes"] < full["work_bytes"]
    assert gl_gap_shape(4, 8, 128, 256, long_spans=True, momentum=0.99)["work_bytes"] > full["work_bytes"]      # P
    with pytest.raises(ValueError, match="max_span"):
        gl_gap_shape(1, 1, 128, 40, long_spans=True, long_max_span=2)            # no room for a gap frame between neighbours
    with pytest.raises(ValueError, match="long_max_span"):
        gl_gap_shape(1, 1, 128, 40, long_spans=True, long_max_span=-3)
    with pytest.raises(ValueError, match="long_spans"):
        gl_gap_shape(1, 1, 128, 40, long_spans="sometimes")
    with pytest.raises(ValueError, match="long_spans"):
        gl_gap_shape(1, 1, 128, 40, long_spans=2)


def test_the_new_options_default_to_the_old_behaviour():
    from nppc_audio.inpainting import phase as PH
    from nppc_audio.inpainting import restore as RS
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    for fn in (PH.griffin_lim_gap, PH.pc_audio_variations_blind, PH.gl_gap_shape, V.NPPCModelValidator.validate_batch):
        assert inspect.signature(fn).parameters["long_spans"].default is False, fn
    assert inspect.signature(RS.plan_windows).parameters["long_gaps"].default is False
    assert RS.RecordingRestorerConfig.model_fields["long_gaps"].default is False
    import torch
    with pytest.raises(ValueError, match="long_spans"):                          # checked before anything touches the GPU
        PH.griffin_lim_gap(torch.zeros(2, 128, 40), torch.zeros(2, 2, 128, 40), torch.ones(2, 40), long_spans="yes")


def test_plan_windows_with_long_gaps():
    from nppc_audio.inpainting.phase import gl_gap_shape
    from nppc_audio.inpainting.restore import plan_windows
    n_fft, hop, W = 255, 128, 32704
    cap = gl_gap_shape(1, 1, n_fft // 2 + 1, 1 + W // hop, n_fft, hop, length=W, n_iter=0)["span_cap"]
    one = [(20000, 20000 + 4096)]
    two = [(10000, 10400), (10000 + 100 * hop, 10400 + 100 * hop)]               # 100 frames apart, one window holds both
    for gaps in (one, two):
        with pytest.raises(ValueError, match=f"span cap of {cap}"):              # the default keeps refusing, in the same words
            plan_windows(48000, gaps)
        plan = plan_windows(48000, gaps, long_gaps=True)
        assert [p["gap"] for p in plan] == gaps
        for p in plan:
            assert p["frames"][1] - p["frames"][0] + 1 + 2 > cap
    assert all(len(p["masked"]) == 2 for p in plan)
    # what long_gaps does not change: a plan within the cap, and every other refusal
    short = [(500, 1524), (11500, 12524), (22000, 23024)]
    kw = dict(window_samples=8192, crossfade_samples=64)
    assert plan_windows(24000, short, long_gaps=True, **kw) == plan_windows(24000, short, **kw)
    for gap in ((0, 600), (130, 700), (23500, 24000)):
        with pytest.raises(ValueError, match="fewer than 2 known frames"):
            plan_windows(24000, [gap], long_gaps=True, **kw)
    with pytest.raises(ValueError, match="fewer than 2 known frames"):           # a long gap that reaches the window's edge
        plan_windows(8192, [(300, 300 + 7800)], long_gaps=True, **kw)
    with pytest.raises(ValueError, match="does not fit a window"):
        plan_windows(24000, [(3000, 3000 + 8192 + 2)], long_gaps=True, **kw)
    with pytest.raises(ValueError, match="crossfade"):
        plan_windows(24000, [(11500, 12524)], long_gaps=True, window_samples=8192, crossfade_samples=4000)
    with pytest.raises(ValueError, match="fewer than one window"):
        plan_windows(8191, [(100, 200)], long_gaps=True, **kw)
    with pytest.raises(ValueError, match=r"\(7, 3\)"):
        plan_windows(24000, [(7, 3)], long_gaps=True, **kw)
