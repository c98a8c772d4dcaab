"""CPU: the fp64 oracle of the speech-enhancement metrics (tests/se_metrics_ref.py) against the reference's recorded SI-SDRs
(tests/golden/se_metrics.npz), the STOI contract's fixed parts (resampler taps, band matrix) and STOI's defining
properties; the host side of nppc_audio.metrics (tap design, registered names, argument checks)."""
import json
import os

import numpy as np
import pytest
from scipy.signal import resample_poly

import se_metrics_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_pairs():
    z = np.load(os.path.join(GOLD, "se_metrics.npz"))
    meta = json.load(open(os.path.join(GOLD, "se_metrics.json")))
    lens = [int(n) for n in z["lengths"]]
    off = np.concatenate([[0], np.cumsum(lens)])
    ref = z["ref_pcm"].astype(np.float32) / np.float32(meta["pcm_scale"])
    est = z["est_pcm"].astype(np.float32) / np.float32(meta["pcm_scale"])
    pairs = []
    for i, n in enumerate(lens):
        r = ref[off[i]:off[i + 1]]
        e = est[off[i]:off[i + 1]] if off[i + 1] <= est.size else r.copy()    # the last pair's estimate is the reference
        pairs.append((r, e))
    return pairs, z


def speech(n, seed):
    from nppc_audio.data import synth_clip
    _, c = synth_clip(seed, n)
    return c.astype(np.float64)


def test_oracle_si_sdr_equals_reference_goldens():
    pairs, z = golden_pairs()
    for (r, e), want, want_zm in zip(pairs, z["si_sdr"], z["si_sdr_zero_mean"]):
        got, got_zm = R.si_sdr(r, e), R.si_sdr_zero_mean(r, e)
        if np.isinf(want):
            assert np.isinf(got) and got > 0
        else:
            assert abs(got - want) < 1e-9, (got, want)
        assert abs(got_zm - want_zm) < 1e-9, (got_zm, want_zm)
    assert np.isinf(z["si_sdr"]).sum() == 1                       # the pair whose estimate equals the reference


def test_resampler_taps_and_stage():
    from nppc_audio.metrics import resample_window
    h = resample_window()
    assert h.shape == (581,)
    assert abs(h.sum() - 1.0) < 1e-12
    assert np.array_equal(h, h[::-1])
    np.testing.assert_array_equal(h, R.resample_taps())
    x = speech(12345, 3)
    y = R.resample(x)
    assert y.shape == (-(-12345 * 5 // 8),)
    np.testing.assert_array_equal(y, resample_poly(x, 5, 8, window=h))
    # the polyphase form the kernel evaluates: y[j] = 5 sum_i x[i] h[290 + 8 j - 5 i] over the taps in range
    j = np.array([0, 1, 7, 500, y.size - 1])
    for jj in j:
        i = np.arange(x.size)
        k = 290 + 8 * jj - 5 * i
        ok = (k >= 0) & (k < 581)
        assert abs(5 * np.sum(x[i[ok]] * h[k[ok]]) - y[jj]) < 1e-12


def test_band_matrix_bins():
    assert R.band_edges() == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55),
                              (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
    m = R.obm()
    assert m.shape == (15, 257) and m[:, :7].sum() == 0 and m[:, 219:].sum() == 0 and m.sum() == 219 - 7


def test_stoi_of_identical_signals_is_one():
    x = speech(32000, 5)
    assert abs(R.stoi(x, x) - 1.0) < 1e-9


def test_stoi_is_invariant_to_estimate_scale():
    x = speech(32000, 6)
    y = x + 0.2 * np.std(x) * np.random.default_rng(0).standard_normal(x.size)
    assert abs(R.stoi(x, 0.3 * y) - R.stoi(x, y)) < 1e-9


def test_stoi_short_item_gives_1e_5():
    x = speech(4800, 7)                              # 0.3 s: 22 frames before silence removal
    assert R.stoi(x, x) == 1e-5
    x = speech(32000, 7)
    z = np.zeros(32000)
    z[10000:14000] = x[10000:14000]                  # 0.25 s of signal in 2 s of silence
    st = R.stoi_stages(z, z)
    assert st["x_tob"].shape[1] < 30 and st["stoi"] == 1e-5


def test_stoi_decreases_with_noise():
    x = speech(48000, 8)
    n = np.random.default_rng(1).standard_normal(x.size)
    n *= np.sqrt(np.mean(x ** 2) / np.mean(n ** 2))
    s = [R.stoi(x, x + n * 10 ** (-snr / 20)) for snr in (20, 10, 0, -10)]
    assert all(a > b for a, b in zip(s, s[1:])), s
    assert s[0] > 0.9 and s[-1] < 0.7


def test_registered_metrics_and_argument_checks():
    from nppc_audio import metrics as M
    assert {"STOI", "SI_SDR", "WB_PESQ", "NB_PESQ", "MOSNET"} <= set(M.REGISTERED_METRICS)
    for name in ("WB_PESQ", "NB_PESQ", "MOSNET"):
        with pytest.raises(NotImplementedError, match=name):
            M.REGISTERED_METRICS[name](None, None, sr=16000)
    with pytest.raises(ValueError, match="16000"):
        M.stoi(None, None, sr=8000)
