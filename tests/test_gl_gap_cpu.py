"""CPU: the fp64 restatement of gap-constrained Griffin-Lim (tests/gl_gap_ref.py) is the yardstick of the GPU tests, so its
own properties are checked here at the same shapes; plus the argument rules of nppc_gl_gap_shape and the declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gl_gap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_fixed_point(case):
    n_fft, hop, T, ranges = case
    L = R.natural_length(n_fft, hop, T)
    x = torch.from_numpy(R.signal(L, 5))
    S = R.stft(x, n_fft, hop)
    mask = R.frame_mask(T, ranges)
    got, d, tn = R.griffin_lim_gap(S.abs(), S * mask[None, :], mask, torch.angle(S), 8, 0.0, n_fft, hop, L)
    assert R.rel_l2(got, x) < 1e-12
    assert float(d.max()) / tn < 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_distance_never_grows_and_known_samples_stay(case):
    z = R.make_case(case, B=3, V=3, seed=R.MONOTONE_SEED)
    W, D, N = R.run_case(z, 16, 0.0, torch.float64)
    assert bool((N > 0).all()) and bool(torch.isfinite(W).all())
    assert bool((D[..., 1:] <= D[..., :-1] * (1 + 1e-9)).all()), D
    assert bool((D[..., -1] < D[..., 0]).all())
    Kn = torch.complex(z["known"][:, 0].double(), z["known"][:, 1].double())
    for b in range(3):
        known = R.istft(Kn[b], z["n_fft"], z["hop"], z["L"])
        out = ~R.reach(z["mask"][b], z["n_fft"], z["hop"], z["L"])
        assert out.any()
        assert float((W[b, 0] - known)[torch.from_numpy(out)].abs().max()) <= 1e-14


def test_restatement_without_a_gap_and_without_iterations():
    z = R.make_case(R.CASES[3], B=1, V=1)
    Kn = torch.complex(z["known"][0, 0].double(), z["known"][0, 1].double())
    full = torch.ones(z["T"])
    x, d, tn = R.griffin_lim_gap(z["target_mag"][0, 0], Kn, full, z["init_phase"][0, 0], 4)
    assert tn == 0.0 and float(d.abs().max()) == 0.0 and torch.equal(x, R.istft(Kn, 255, 128, z["L"]))
    x0, d0, _ = R.griffin_lim_gap(z["target_mag"][0, 0], Kn, z["mask"][0], z["init_phase"][0, 0], 0)
    assert d0.numel() == 0 and x0.shape == (z["L"],)


def test_phase_advance_of_a_stationary_sinusoid_is_its_true_phase():
    n_fft, hop, T = 64, 16, 48
    L = R.natural_length(n_fft, hop, T)
    k = 5                                                                       # a sinusoid on bin 5 exactly
    x = torch.cos(2 * math.pi * k * torch.arange(L, dtype=torch.float64) / n_fft + 0.3)
    S = R.stft(x, n_fft, hop)
    for ranges in ([(20, 30)], [(0, 6)]):
        mask = R.frame_mask(T, ranges)
        phi = R.phase_advance_init(S * mask[None, :], mask, n_fft, hop)
        a, e = max(ranges[0][0], 2), ranges[0][1]                               # frames 0 and 1 see the reflected head
        err = torch.angle(torch.polar(torch.ones(e - a + 1, dtype=torch.float64), phi[k, a:e + 1] - torch.angle(S[k, a:e + 1])))
        assert float(err.abs().max()) < 1e-9
        assert float(phi[:, mask != 0].abs().max()) == 0.0


def test_shape_rules_raise_value_errors():
    from nppc_audio.inpainting.phase import GL_MAX_SPAN_FRAMES, gl_gap_shape
    sh = gl_gap_shape(16, 66, 128, 256)
    assert sh["length"] == 128 * 255 + 1 and sh["r"] == 1 and sh["span_cap"] == GL_MAX_SPAN_FRAMES
    assert sh["lds_bytes"] <= 160 * 1024 and sh["work_bytes"] > 0
    # the reference's 128 ms gap (2048 samples at 16 kHz) with its neighbours fits at both settings, momentum or not
    for n_fft, hop in ((255, 128), (510, 256)):
        gap_frames = 2048 // hop + 2
        for mu in (0.0, 0.99):
            s = gl_gap_shape(1, 1, n_fft // 2 + 1, 64, n_fft, hop, momentum=mu)
            assert s["span_cap"] >= gap_frames + 2 * s["r"], (n_fft, hop, mu, s)
    assert gl_gap_shape(1, 1, 128, 256, max_span=19)["lds_bytes"] < sh["lds_bytes"]
    with pytest.raises(ValueError, match="frequency bins"):
        gl_gap_shape(1, 1, 129, 40)
    with pytest.raises(ValueError, match="frames"):
        gl_gap_shape(1, 1, 128, 40, length=128 * 40)                            # 41 frames
    with pytest.raises(ValueError, match="frames"):
        gl_gap_shape(1, 1, 128, 40, length=128 * 39 - 1)                        # 39 frames
    with pytest.raises(ValueError, match="ceil"):
        gl_gap_shape(1, 1, 51, 40, n_fft=100, hop_length=12)                    # 9 overlapping frames
    with pytest.raises(ValueError, match="512"):
        gl_gap_shape(1, 1, 513, 40, n_fft=1024, hop_length=256)
    with pytest.raises(ValueError, match="negative"):
        gl_gap_shape(1, 1, 128, 40, n_iter=-1)
    with pytest.raises(ValueError, match="negative"):
        gl_gap_shape(1, 1, 128, 40, momentum=-0.1)
    with pytest.raises(ValueError, match="negative"):
        gl_gap_shape(1, 1, 128, 40, momentum=float("nan"))
    with pytest.raises(ValueError, match="max_span"):
        gl_gap_shape(1, 1, 128, 40, max_span=2)                                 # no room for a gap frame between neighbours
    assert gl_gap_shape(1, 1, 128, 40, n_iter=0)["length"] == 128 * 39 + 1


def test_python_entry_points_check_before_touching_the_gpu():
    from nppc_audio.inpainting import phase as PH
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    B, K, F, T = 2, 3, 128, 40
    with pytest.raises(ValueError, match="no alphas"):
        PH.pc_audio_variations_blind(torch.zeros(B, 1, F, T), torch.zeros(B, K, F, T), torch.zeros(B, 2, F, T), torch.ones(B, T),
                                     [], 0.0, 1.0)
    with pytest.raises(ValueError, match="frequency bins"):
        PH.griffin_lim_gap(torch.zeros(B, F + 1, T), torch.zeros(B, 2, F + 1, T), torch.ones(B, T))
    with pytest.raises(ValueError, match="frames"):
        PH.griffin_lim_gap(torch.zeros(B, F, T), torch.zeros(B, 2, F, T), torch.ones(B, T), length=100)
    with pytest.raises(ValueError, match="do not fit"):
        PH.griffin_lim_gap(torch.zeros(B, F, T), torch.zeros(B, 2, F, T), torch.ones(B, T + 1))
    val = V.NPPCModelValidator.__new__(V.NPPCModelValidator)                    # the checks come before anything touches the model
    with pytest.raises(ValueError, match="alphas"):
        val.validate_batch(None, None, None, phase="griffin_lim")
    with pytest.raises(ValueError, match="phase"):
        val.validate_batch(None, None, None, phase="random")


def header_functions():
    txt = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt, {m.group(1): [a for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
                 for m in re.finditer(r"\bint\s+(nppc_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_new_symbols_are_declared_bound_and_exported():
    from nppc_audio import _hip as H
    from nppc_audio.inpainting.phase import GL_MAX_SPAN_FRAMES
    txt, fns = header_functions()
    for name in ("nppc_gl_gap_shape", "nppc_gl_phase_init", "nppc_gl_gap", "nppc_gl_gap_pc"):
        assert name in fns and len(fns[name]) == len(H.SIGS[name]), name
        assert hasattr(H.lib(), name), f"{name} not exported by libnppc_hip.so"
    assert int(re.search(r"#define\s+NPPC_GL_MAX_SPAN_FRAMES\s+(\d+)", txt).group(1)) == GL_MAX_SPAN_FRAMES
    with pytest.raises(RuntimeError, match="bad argument"):                     # null pointers are refused before any launch
        H.call("nppc_gl_gap", None, None, None, None, 0, None, None, None, None, None, 0, 1, 1, 40, 255, 128, 4993, 1, 0.0, 0, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_gl_phase_init", None, None, None, 1, 40, 255, 128, None)
