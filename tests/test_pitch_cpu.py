"""CPU: the fp64 pYIN restatement (tests/pyin_ref.py) against ground truth, its sensitivity to an fp32 d', and the host
logic of nppc_audio/pitch.py and nppc_pyin_shape.  librosa is not available: nothing here compares with librosa.pyin.

Measured on the restatement (fmin 80, fmax 400, sr 16000, frame 2048; interior frames = frames whose 2048-sample window
lies inside the signal; the reference frequency of a frame is the instantaneous f0 at its centre sample):

| signal (2 s, 6 partials, 1/h)   | interior frames | voiced share | largest |cents| error |
|---------------------------------|-----------------|--------------|------------------------|
| tone 100 Hz                     | 59              | 1.00         | 3.69                   |
| tone 155.56 Hz                  | 59              | 1.00         | 1.28                   |
| tone 220 Hz                     | 59              | 1.00         | 1.32                   |
| tone 330 Hz                     | 59              | 1.00         | 3.27                   |
| linear glide 120 -> 240 Hz      | 59              | 1.00         | 29.35                  |

(the glide's error is the lag of the analysis window: d(tau) reads samples 0 .. W + tau of the frame, whose middle lies some
460 samples before the frame's centre, 1.7 Hz of glide).  1 s of zeros: 32 frames, none voiced, voiced_prob 0.  White noise
(seed 0, sigma 0.1, 1 s): 32 frames, none voiced, largest voiced_prob 0.01 (= no_trough_prob).

Limits: the measured error plus one pitch bin (10 cents); a voiced share no lower than the measured one minus 2 points.

Precision sensitivity (d' rounded to fp32 before the observation stage, against all-fp64): 0 of the frames of every signal
used by tests/test_pitch_gpu.py differ in voiced_flag or pitch bin (the five signals above, zeros, noise, speech_like seeds
1, 2, 3); the bound is 0.5 %.
"""
import ctypes

import numpy as np
import pytest
import torch

import pyin_ref as R

FMIN, FMAX = 80.0, 400.0
# (name, measured largest |cents| error, measured voiced share)
MEASURED = {"tone100": (3.69, 1.0), "tone155.56": (1.28, 1.0), "tone220": (1.32, 1.0), "tone330": (3.27, 1.0),
            "glide": (29.35, 1.0)}
ONE_BIN_CENTS = 10.0
SPEECH_SEEDS = (1, 2, 3)


def ground_truth_signals():
    """name -> (waveform fp32, reference f0 per sample or scalar)"""
    out = {}
    for f in (100.0, 155.56, 220.0, 330.0):
        out["tone%g" % f] = (R.harmonic_tone(f), f)
    y, f = R.glide()
    out["glide"] = (y, f)
    return out


def all_signals():
    """every waveform the GPU tests track, name -> fp32 array"""
    out = {k: v[0] for k, v in ground_truth_signals().items()}
    out["zeros"] = np.zeros(16000, np.float32)
    out["noise"] = R.white_noise(0)
    for s in SPEECH_SEEDS:
        out[f"speech{s}"] = R.speech_like(s)[0]
    return out


def ground_truth_figures(name, y, ref, f0, voiced):
    """(largest |cents| error over the voiced interior frames, voiced share of the interior frames)"""
    s = R.Setting(FMIN, FMAX)
    it = R.interior_frames(len(y), s)
    v = np.asarray(voiced)[it].astype(bool)
    r = np.full(len(it), ref) if np.isscalar(ref) else np.asarray(ref)[it * s.hop_length]
    c = np.abs(R.cents(np.asarray(f0)[it][v], r[v]))
    return (float(c.max()) if len(c) else float("nan")), float(v.mean())


def check_ground_truth(name, y, ref, f0, voiced):
    err, share = ground_truth_figures(name, y, ref, f0, voiced)
    m_err, m_share = MEASURED[name]
    print(f"{name}: largest |cents| error {err:.2f} (measured on the restatement {m_err}), voiced share {share:.3f}")
    assert err <= m_err + ONE_BIN_CENTS, (name, err)
    assert share >= m_share - 0.02, (name, share)
    return err, share


_cache = {}


def ref_run(name, y):
    if name not in _cache:
        _cache[name] = R.pyin(y, FMIN, FMAX)
    return _cache[name]


# ---- 1. ground truth -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MEASURED))
def test_restatement_tracks_tones_and_a_glide(name):
    y, ref = ground_truth_signals()[name]
    o = ref_run(name, y)
    err, share = check_ground_truth(name, y, ref, o["f0"], o["voiced_flag"])
    if name != "glide":                                       # a steady tone: the restatement itself must be this good
        assert err <= 2 * ONE_BIN_CENTS and share >= 0.95
    assert abs(err - MEASURED[name][0]) < 0.01 and share == MEASURED[name][1]     # the header's figures are current


def test_restatement_on_zeros_and_noise():
    o = ref_run("zeros", np.zeros(16000, np.float32))
    assert o["f0"].shape == (32,) and not o["voiced_flag"].any() and np.isnan(o["f0"]).all()
    assert np.all(o["voiced_prob"] == 0.0)
    n = ref_run("noise", R.white_noise(0))
    print("noise: voiced frames", int(n["voiced_flag"].sum()), "largest voiced_prob", float(n["voiced_prob"].max()))
    assert not n["voiced_flag"].any() and float(n["voiced_prob"].max()) <= 0.01 + 1e-7


def test_restatement_shapes_and_tables():
    s = R.Setting(FMIN, FMAX)
    assert (s.min_period, s.max_period, s.P, s.n_pitch_bins, s.width, s.nbps) == (40, 200, 161, 279, 281, 10)
    w = s.beta_weights()
    assert w.shape == (100,) and abs(w.sum() - 1.0) < 1e-12 and np.all(w >= 0)
    ltri, lrow, lstay, lsw, linit = s.hmm_tables()
    assert ltri.shape == (281,) and lrow.shape == (279,) and np.all(np.isfinite(ltri))
    assert abs(np.exp(lstay) + np.exp(lsw) - 1.0) < 1e-15 and abs(np.exp(linit) * 558 - 1.0) < 1e-12
    o = ref_run("tone220", R.harmonic_tone(220.0))
    assert np.allclose(o["obs"].sum(axis=1), 1.0, atol=1e-9)           # a distribution over the 558 states per frame


# ---- 2. precision sensitivity --------------------------------------------------------------------------------------------
def test_an_fp32_dprime_changes_at_most_half_a_percent_of_the_frames():
    total = differ = 0
    for name, y in all_signals().items():
        a = ref_run(name, y)
        b = R.pyin(y, FMIN, FMAX, dprime_dtype=np.float32)
        d = (a["voiced_flag"] != b["voiced_flag"]) | ((a["voiced_flag"] == 1) & (a["bin"] != b["bin"]))
        print(f"{name}: {int(d.sum())} of {d.size} frames differ with an fp32 d'")
        assert d.mean() <= 0.005, name
        total, differ = total + d.size, differ + int(d.sum())
    assert differ <= 0.005 * total


# ---- 3. host logic -------------------------------------------------------------------------------------------------------
def test_pitch_variation_summary():
    from nppc_audio.pitch import pitch_variation_summary
    B, K, A, T = 2, 3, 4, 9
    f0c = torch.full((B, T), 200.0)
    vc = torch.ones(B, T, dtype=torch.uint8)
    vc[:, 0] = 0
    f0c[:, 0] = float("nan")
    f0v = f0c[:, None, None, :].repeat(1, K, A, 1) * 2.0 ** (50.0 / 1200.0)      # + 50 cents everywhere
    vv = vc[:, None, None, :].repeat(1, K, A, 1)
    f0v[0, 1, 2, 3:] = float("nan")                                              # (0, 1, 2): voiced in frames 1, 2 only
    vv[0, 1, 2, 3:] = 0
    f0v[1, 0, 0] = float("nan")                                                  # (1, 0, 0): never voiced
    vv[1, 0, 0] = 0
    f0v[1, 2, 3, 1] = 200.0 * 2.0 ** (-700.0 / 1200.0)                           # one outlier frame: the median ignores it
    s = pitch_variation_summary(f0c, vc, f0v, vv)
    assert set(s) == {"shift_cents", "voicing_agreement", "n_joint_voiced"}
    assert all(v.shape == (B, K, A) for v in s.values())
    assert torch.isnan(s["shift_cents"][1, 0, 0]) and int(s["n_joint_voiced"][1, 0, 0]) == 0
    rest = torch.ones(B, K, A, dtype=torch.bool)
    rest[1, 0, 0] = False
    assert float((s["shift_cents"][rest] - 50.0).abs().max()) < 1e-3
    assert int(s["n_joint_voiced"][0, 1, 2]) == 2 and int(s["n_joint_voiced"][0, 0, 0]) == T - 1
    assert abs(float(s["voicing_agreement"][0, 1, 2]) - 3.0 / 9.0) < 1e-6        # frames 0, 1, 2 agree
    assert abs(float(s["voicing_agreement"][1, 0, 0]) - 1.0 / 9.0) < 1e-6
    assert float(s["voicing_agreement"][0, 0, 0]) == 1.0
    with pytest.raises(ValueError):
        pitch_variation_summary(f0c, vc, f0v[..., :5], vv[..., :5])


def test_shape_query_at_the_reference_setting_and_equals_the_restatement():
    from nppc_audio.pitch import pyin_shape
    sh = pyin_shape(66, 63873, 80, 400, sr=16000)
    assert (sh["T"], sh["P"], sh["n_pitch_bins"], sh["width"]) == (1 + 63873 // 512, 161, 279, 281)
    assert (sh["min_period"], sh["max_period"]) == (40, 200)
    assert sh["workspace_bytes"] == 66 * 125 * 558 * 2
    for kw in (dict(fmin=100, fmax=500, frame_length=600, hop_length=100), dict(fmin=60, fmax=1000, sr=22050),
               dict(fmin=80, fmax=400, sr=8000, frame_length=1024, resolution=0.25)):
        s = R.Setting(**kw)
        fmin, fmax = kw.pop("fmin"), kw.pop("fmax")
        sh = pyin_shape(1, 5000, fmin, fmax, **kw)
        assert (sh["T"], sh["P"], sh["min_period"], sh["n_pitch_bins"], sh["width"], sh["bins_per_semitone"]) == \
            (s.n_frames(5000), s.P, s.min_period, s.n_pitch_bins, s.width, s.nbps), kw


BAD_SETTINGS = [
    dict(frame_length=4096),                                   # frame_length > 2048
    dict(fmin=80, fmax=80),                                    # no lag range
    dict(fmin=400, fmax=80),
    dict(fmin=80, fmax=400, sr=50),                            # min_period == max_period == 1
    dict(fmin=4000, fmax=7000, frame_length=8, win_length=6, hop_length=2),   # max_period clipped below min_period
    dict(win_length=2048),                                     # no room for any lag
    dict(win_length=0),
    dict(hop_length=0),
    dict(fmin=0.0),
    dict(fmin=float("nan")),
    dict(sr=0),
    dict(resolution=0.0),
    dict(fmin=20, fmax=7000, resolution=0.05),                 # more than 768 pitch bins
    dict(L=0),
    dict(N=0),
]


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_unsupported_settings_are_bad_arguments(bad):
    from nppc_audio import _hip as H
    from nppc_audio.pitch import pyin, pyin_shape
    kw = dict(N=2, L=4000, fmin=80.0, fmax=400.0, sr=16000, frame_length=2048, win_length=None, hop_length=None)
    kw.update(bad)
    with pytest.raises(ValueError, match="pyin"):
        pyin_shape(kw["N"], kw["L"], kw["fmin"], kw["fmax"], kw["sr"], kw["frame_length"], kw["win_length"], kw["hop_length"],
                   kw.get("resolution", 0.1))
    if kw["N"] >= 1 and kw["L"] >= 1:
        with pytest.raises(ValueError, match="pyin"):            # before any launch: no GPU is needed to be refused
            pyin(torch.zeros(kw["N"], kw["L"]), kw["fmin"], kw["fmax"], sr=kw["sr"], frame_length=kw["frame_length"],
                 win_length=kw["win_length"], hop_length=kw["hop_length"], resolution=kw.get("resolution", 0.1))


def test_entry_points_refuse_bad_arguments_before_launching():
    from nppc_audio import _hip as H
    lib = H.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def rc(name, *args):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = H.SIGS[name], ctypes.c_int
        return fn(*args)
    null = ctypes.c_void_p(0)
    # cmnd: y, lengths, dprime, N, L, frame, win, hop, min_period, max_period, stream
    assert rc("nppc_pyin_cmnd", null, null, p, 1, 100, 2048, 1024, 512, 40, 200, null) == 1
    assert rc("nppc_pyin_cmnd", p, null, p, 1, 100, 4096, 2048, 512, 40, 200, null) == 1        # frame_length > 2048
    assert rc("nppc_pyin_cmnd", p, null, p, 1, 100, 2048, 1024, 512, 40, 1024, null) == 1       # max_period >= frame - win
    assert rc("nppc_pyin_cmnd", p, null, p, 1, 100, 2048, 1024, 512, 40, 40, null) == 1         # min_period == max_period
    assert rc("nppc_pyin_cmnd", p, null, p, 1, 100, 2048, 1024, 512, 0, 200, null) == 1         # min_period < 1
    assert rc("nppc_pyin_cmnd", p, null, p, 1, 0, 2048, 1024, 512, 40, 200, null) == 1          # no samples
    # observe: dprime, lengths, beta_w, obs, vp, N, T, L, hop, P, min_period, n_thr, bins, nbps, sr, fmin, boltzmann, no_trough
    ok = [p, null, p, p, p, 1, 4, 2000, 512, 161, 40, 100, 279, 10, 16000.0, 80.0, 2.0, 0.01, null]
    for idx, val in ((9, 1), (9, 2000), (11, 0), (11, 5000), (12, 769), (13, 0), (16, 0.0), (17, -1.0), (2, null)):
        a = list(ok)
        a[idx] = val
        assert rc("nppc_pyin_observe", *a) == 1, (idx, val)
    # viterbi: obs, lengths, tab, backptr, f0, flag, N, T, L, hop, bins, nbps, width, fmin, stream
    ok = [p, null, p, p, p, p, 1, 4, 2000, 512, 279, 10, 281, 80.0, null]
    for idx, val in ((10, 769), (10, 0), (12, 280), (12, 0), (13, 0.0), (3, null), (7, 0)):
        a = list(ok)
        a[idx] = val
        assert rc("nppc_pyin_viterbi", *a) == 1, (idx, val)


def test_python_argument_checks():
    from nppc_audio.pitch import pyin
    y = torch.zeros(2, 4000)
    for kw in (dict(n_thresholds=0), dict(n_thresholds=2000), dict(beta_parameters=(2, 0)), dict(boltzmann_parameter=0),
               dict(switch_prob=0.0), dict(switch_prob=1.0), dict(no_trough_prob=-0.1)):
        with pytest.raises(ValueError, match="pyin"):
            pyin(y, 80, 400, **kw)
    with pytest.raises(ValueError, match="pyin"):
        pyin(torch.zeros(2, 0), 80, 400)


def test_pyin_fails_loudly_without_a_gpu():
    from nppc_audio.pitch import pyin
    with pytest.raises(RuntimeError, match="HIP"):               # a host tensor is refused, never tracked on the host
        pyin(torch.zeros(4000), 80, 400)


def test_validate_batch_with_pitch_needs_alphas():
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    val = V.NPPCModelValidator.__new__(V.NPPCModelValidator)     # the check comes before anything touches the model
    with pytest.raises(ValueError, match="alphas"):
        val.validate_batch(None, None, None, pitch=True)


def test_new_symbols_are_declared_and_bound():
    import os
    from nppc_audio import _hip as H
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "nppc_hip.h")).read()
    for name in ("nppc_pyin_shape", "nppc_pyin_cmnd", "nppc_pyin_observe", "nppc_pyin_viterbi"):
        assert f"int {name}(" in hdr and name in H.SIGS and hasattr(H.lib(), name)
