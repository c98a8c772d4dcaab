"""CPU: the fp64 restatement of the BSS-eval SDR contract (tests/bss_eval_ref.py) is the yardstick of the GPU tests, so it
is pinned here: its direct sums are the numbers of the FFT route mir_eval takes, the choice of solver does not move the SDR
on the inputs the GPU tests use, and the causal filter absorbs a delay.  Plus the public surface that needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bss_eval_ref as R

# (lengths, P) of the GPU test's fixed cases; the chunk-boundary cases are appended below from the exported constants
CASES = [((700, 513, 37, 1), 8), ((4000, 64, 63, 65), 64), ((16000, 300, 512, 511), 512)]
SPREAD_DB = 1e-12


def chunk_cases():
    from nppc_audio import metrics as M
    P = 64
    out = []
    for C in sorted({M.BSS_CORR_CHUNK, M.BSS_CORR_TILE, M.BSS_PROJ_CHUNK}):
        out.append(((C - 1, C, C + 1, C + P - 1), P))
    return out


def all_cases():
    return CASES + chunk_cases()


def exact_in_span(n, P):
    """n = 1: the estimate is a multiple of the reference, den is rounding noise and the SDR is +inf or > 250 dB"""
    return n == 1


def test_direct_sums_equal_the_fft_route():
    for lengths, P in CASES:
        for s, e in R.make_batch(lengths, seed0=P):
            r, d = R.correlations(s, e, P)
            rf, df = R.correlations_fft(s, e, P)
            scale = np.sqrt(r[0] * np.sum(e.astype(np.float64) ** 2))
            # an FFT of size N carries errors of a few eps log2(N) times the signals' norms
            assert np.abs(r - rf).max() <= 1e-13 * r[0], (lengths, P)
            assert np.abs(d - df).max() <= 1e-13 * scale, (lengths, P)


def test_delay_convention_is_causal():
    """d[t] pairs the estimate with the reference delayed by t: an estimate that IS the reference delayed by 3 has all its
    correlation at lag 3 (relative to r[0]), none of it at the mirrored lag"""
    s, _ = R.make_pair(5, 2000)
    s[-3:] = 0.0                                           # so that the delayed copy still holds all of it
    e = np.concatenate((np.zeros(3, np.float32), s[:-3]))
    r, d = R.correlations(s, e, 8)
    assert np.argmax(d) == 3 and abs(d[3] / r[0] - 1) < 1e-12
    assert abs(d[0] - r[3]) <= 1e-12 * r[0]


def test_solvers_agree_on_the_test_inputs():
    worst = 0.0
    for lengths, P in all_cases():
        for (s, e), n in zip(R.make_batch(lengths, seed0=P), lengths):
            if exact_in_span(n, P):
                continue
            sp = R.solver_spread(s, e, P)
            worst = max(worst, sp)
            assert sp < SPREAD_DB, (lengths, P, n, sp)
            # the recursion the device runs is a fourth solver with the same answer
            assert abs(R.sdr(s, e, P, "levinson") - R.sdr(s, e, P, "lu")) < SPREAD_DB, (lengths, P, n)
    print(f"worst solver spread {worst:.2e} dB")


def test_delay_and_gain_are_forgiven_by_sdr_not_by_si_sdr():
    s, _ = R.make_pair(11, 4000)
    s[-3:] = 0.0                                           # so that the delayed copy still holds all of it
    e = np.concatenate((np.zeros(3, np.float32), 0.5 * s[:-3]))
    assert R.sdr(s, e, 64) > 200.0
    assert R.si_sdr(s, e) < 10.0


def test_all_zero_reference_is_nan_and_a_copy_is_huge():
    s, e = R.make_pair(2, 500)
    assert np.isnan(R.sdr(np.zeros_like(s), e, 8))
    assert R.sdr(s, s, 8) > 250.0


def test_scale_bss_eval_restatement_identities():
    s, e = R.make_pair(4, 3000)
    m = R.scale_bss_eval(s, e)
    s64, e64 = s.astype(np.float64), e.astype(np.float64)
    a = np.dot(s64, e64) / np.dot(s64, s64)
    proj = a * s64
    assert abs(m["si_sdr"] - 10 * np.log10(np.sum(proj ** 2) / np.sum((e64 - proj) ** 2))) < 1e-12
    assert abs(m["sd_sdr"] - (m["snr"] + 20 * np.log10(abs(a)))) < 1e-12
    assert m["si_sdr"] >= m["sd_sdr"] - 1e-12              # the scale-dependent SDR never beats the scale-invariant one


def test_public_surface():
    from nppc_audio import metrics as M
    assert "SDR" in M.REGISTERED_METRICS
    assert callable(M.sdr) and callable(M.sdr_stages) and callable(M.scale_bss_eval)
    assert {"sdr", "sdr_stages", "scale_bss_eval"} <= set(M.__all__)
    assert M.BSS_MAX_FILTER == 512


def test_chunk_constants_match_the_library():
    from nppc_audio import _hip as H
    from nppc_audio import metrics as M
    cc, ct, pc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n1, n2 = ctypes.c_long(), ctypes.c_long()
    L, P = 20000, 64
    H.call("nppc_bss_shape", L, P, ctypes.byref(cc), ctypes.byref(ct), ctypes.byref(pc), ctypes.byref(n1), ctypes.byref(n2))
    assert (cc.value, ct.value, pc.value) == (M.BSS_CORR_CHUNK, M.BSS_CORR_TILE, M.BSS_PROJ_CHUNK)
    assert n1.value == -(-L // M.BSS_CORR_CHUNK) * 2 * P
    assert n2.value == -(-(L + P - 1) // M.BSS_PROJ_CHUNK) * 2
    with pytest.raises(RuntimeError, match="unsupported"):
        H.call("nppc_bss_shape", L, 513, ctypes.byref(cc), ctypes.byref(ct), ctypes.byref(pc), ctypes.byref(n1), ctypes.byref(n2))
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_bss_corr", None, None, None, 1, 100, 8, None, 0, None)


def test_bad_filter_length_is_a_value_error_before_anything_else():
    from nppc_audio import metrics as M
    x = torch.zeros(2, 100)
    for bad in (0, 513, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="filter_length"):
            M.sdr(x, x, filter_length=bad)
        with pytest.raises(ValueError, match="filter_length"):
            M.sdr_stages(x, x, filter_length=bad)


def test_cpu_tensors_raise_the_usual_error():
    from nppc_audio import metrics as M
    x = torch.zeros(2, 100)
    for fn in (M.sdr, M.scale_bss_eval, M.REGISTERED_METRICS["SDR"]):
        with pytest.raises(RuntimeError, match="HIP"):
            fn(x, x)


def test_validator_rejects_unknown_extra_metrics():
    from nppc_audio.model_validator import EXTRA_METRICS, ModelValidator
    assert EXTRA_METRICS == ("SDR",)
    assert ModelValidator._check_extra(()) == ()
    assert ModelValidator._check_extra(["SDR"]) == ("SDR",)
    with pytest.raises(ValueError, match="WB_PESQ"):
        ModelValidator._check_extra(("WB_PESQ",))
