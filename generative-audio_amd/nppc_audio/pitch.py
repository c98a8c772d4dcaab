"""Batched pYIN f0 tracking on the device (csrc/pitch.hip; specification tests/pyin_ref.py).

The reference's plot_pitch_comparison (nppc_audio/inpainting/validator/validator_nppc_model.py:19-270) runs
librosa.pyin(fmin=80, fmax=400, sr=16000) over the clean waveform and each of the K * A variations of an item, one call at
a time on the host.  Here the waveforms stay on the device and all of them go through three launches.
"""
import ctypes
import math

import numpy as np
import torch

from . import _hip as H

__all__ = ["pyin", "pyin_shape", "pyin_stages", "pitch_variation_summary", "REFERENCE_SETTING"]

# the reference's call (validator_nppc_model.py:60-66)
REFERENCE_SETTING = dict(fmin=80.0, fmax=400.0, sr=16000)

_tables = {}


def pyin_shape(N, L, fmin, fmax, sr=16000, frame_length=2048, win_length=None, hop_length=None, resolution=0.1,
               max_transition_rate=35.92):
    """nppc_pyin_shape: runs without a GPU.  -> dict(T, P, min_period, max_period, n_pitch_bins, width, workspace_bytes,
    win_length, hop_length, bins_per_semitone); ValueError for a setting the kernels do not take."""
    win_length = frame_length // 2 if win_length is None else int(win_length)
    hop_length = frame_length // 4 if hop_length is None else int(hop_length)
    T, P, mp, nb, w = (ctypes.c_int() for _ in range(5))
    ws = ctypes.c_long()
    fn = H.lib().nppc_pyin_shape
    fn.argtypes, fn.restype = H.SIGS["nppc_pyin_shape"], ctypes.c_int
    ok = all(math.isfinite(float(v)) for v in (sr, fmin, fmax, resolution, max_transition_rate))
    rc = 1 if not ok else fn(int(N), int(L), float(sr), float(fmin), float(fmax), int(frame_length), win_length, hop_length,
                             float(resolution), float(max_transition_rate), ctypes.byref(T), ctypes.byref(P), ctypes.byref(mp),
                             ctypes.byref(nb), ctypes.byref(w), ctypes.byref(ws))
    if rc != 0:
        raise ValueError(
            f"pyin: unsupported setting (N={N}, L={L}, sr={sr}, fmin={fmin}, fmax={fmax}, frame_length={frame_length}, "
            f"win_length={win_length}, hop_length={hop_length}, resolution={resolution}): needs frame_length <= 2048, "
            "1 <= min_period < max_period < frame_length - win_length and at most 768 pitch bins")
    return dict(T=T.value, P=P.value, min_period=mp.value, max_period=mp.value + P.value - 1, n_pitch_bins=nb.value,
                width=w.value, workspace_bytes=ws.value, win_length=win_length, hop_length=hop_length,
                bins_per_semitone=int(math.ceil(1.0 / resolution)))


def beta_weights(n_thresholds, beta_parameters):
    """threshold weights: differences of the Beta CDF over s_i = i / n_thresholds (SciPy, on the host)"""
    import scipy.stats
    s = np.arange(n_thresholds + 1, dtype=np.float64) / n_thresholds
    return np.diff(scipy.stats.beta.cdf(s, beta_parameters[0], beta_parameters[1]))


def hmm_table(n_pitch_bins, width, switch_prob):
    """log tri [width] | log rowsum [n_pitch_bins] | log stay, log switch, log init (fp64, on the host)"""
    half = width // 2
    d = np.arange(width, dtype=np.float64)
    tri = 1.0 - np.abs(d - half) / (half + 1.0)
    rows = np.empty(n_pitch_bins, dtype=np.float64)
    for i in range(n_pitch_bins):
        lo, hi = max(0, i - half), min(n_pitch_bins - 1, i + half)
        rows[i] = np.sum(tri[lo - i + half:hi - i + half + 1])
    tail = np.array([np.log(1.0 - switch_prob), np.log(switch_prob), np.log(1.0 / (2 * n_pitch_bins))])
    return np.concatenate([np.log(tri), np.log(rows), tail])


def _device_tables(dev, n_thresholds, beta_parameters, n_pitch_bins, width, switch_prob):
    key = (str(dev), n_thresholds, tuple(beta_parameters), n_pitch_bins, width, switch_prob)
    if key not in _tables:
        _tables[key] = (torch.from_numpy(beta_weights(n_thresholds, beta_parameters)).to(dev),
                        torch.from_numpy(hmm_table(n_pitch_bins, width, switch_prob)).to(dev))
    return _tables[key]


def _check(n_thresholds, beta_parameters, boltzmann_parameter, switch_prob, no_trough_prob):
    if not (1 <= int(n_thresholds) <= 1024):
        raise ValueError(f"pyin: n_thresholds = {n_thresholds} is outside 1..1024")
    if len(beta_parameters) != 2 or not all(float(b) > 0 for b in beta_parameters):
        raise ValueError(f"pyin: beta_parameters = {beta_parameters} must be two positive numbers")
    if not float(boltzmann_parameter) > 0:
        raise ValueError(f"pyin: boltzmann_parameter = {boltzmann_parameter} must be positive")
    if not 0.0 < float(switch_prob) < 1.0:
        raise ValueError(f"pyin: switch_prob = {switch_prob} must lie inside (0, 1)")
    if not 0.0 <= float(no_trough_prob) <= 1.0:
        raise ValueError(f"pyin: no_trough_prob = {no_trough_prob} must lie in [0, 1]")


def pyin_stages(y, fmin, fmax, sr=16000, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
                beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01,
                no_trough_prob=0.01, lengths=None, dprime=None, obs=None):
    """The three launches on y [N, L] with every intermediate returned: dict(dprime [N,T,P], obs [N,T,2 bins], voiced_prob,
    f0, voiced_flag, shape).  `dprime` / `obs` given: that stage's input is taken from the caller instead (tests feed a stage
    the arrays they also hand to the fp64 restatement)."""
    if y.dim() != 2:
        raise ValueError(f"pyin_stages takes [N, L], got {tuple(y.shape)}")
    N, L = y.shape
    _check(n_thresholds, beta_parameters, boltzmann_parameter, switch_prob, no_trough_prob)
    sh = pyin_shape(N, L, fmin, fmax, sr, frame_length, win_length, hop_length, resolution, max_transition_rate)
    H.require_gpu()
    if not y.is_cuda:
        raise RuntimeError("pyin needs its waveforms on a HIP device: the hot path is HIP-only")
    y = y.contiguous().float()
    dev = y.device
    T, P, nb = sh["T"], sh["P"], sh["n_pitch_bins"]
    hop, nbps = sh["hop_length"], sh["bins_per_semitone"]
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if lengths.numel() != N:
            raise ValueError(f"pyin: {lengths.numel()} lengths for {N} waveforms")
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous().reshape(N)
    bw, tab = _device_tables(dev, int(n_thresholds), tuple(float(b) for b in beta_parameters), nb, sh["width"],
                             float(switch_prob))
    s = H.stream()
    if dprime is None:
        dprime = torch.empty(N, T, P, dtype=torch.float32, device=dev)
        H.call("nppc_pyin_cmnd", y, lengths, dprime, N, L, int(frame_length), sh["win_length"], hop, sh["min_period"],
               sh["max_period"], s)
    else:
        dprime = dprime.to(dev).float().contiguous()
        assert dprime.shape == (N, T, P)
    vp = torch.empty(N, T, dtype=torch.float32, device=dev)
    if obs is None:
        obs = torch.empty(N, T, 2 * nb, dtype=torch.float32, device=dev)
        H.call("nppc_pyin_observe", dprime, lengths, bw, obs, vp, N, T, L, hop, P, sh["min_period"], int(n_thresholds), nb, nbps,
               float(sr), float(fmin), float(boltzmann_parameter), float(no_trough_prob), s)
    else:
        obs = obs.to(dev).float().contiguous()
        assert obs.shape == (N, T, 2 * nb)
        vp = obs[:, :, :nb].double().sum(-1).clamp(0, 1).float()
    back = torch.empty(sh["workspace_bytes"] // 2, dtype=torch.int16, device=dev)
    f0 = torch.empty(N, T, dtype=torch.float32, device=dev)
    flag = torch.empty(N, T, dtype=torch.uint8, device=dev)
    H.call("nppc_pyin_viterbi", obs, lengths, tab, back, f0, flag, N, T, L, hop, nb, nbps, sh["width"], float(fmin), s)
    return dict(dprime=dprime, obs=obs, voiced_prob=vp, f0=f0, voiced_flag=flag, shape=sh)


def pyin(y, fmin, fmax, sr=16000, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
         beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01,
         no_trough_prob=0.01, lengths=None):
    """pYIN f0 contours of y [..., L] (center=True, zero padding) -> (f0 [..., T] fp32 with NaN where unvoiced,
    voiced_flag [..., T] uint8, voiced_prob [..., T] fp32), T = 1 + L // hop_length.

    lengths (one int per waveform, any shape with that many elements; host or device): waveform i is its first lengths[i]
    samples; its first 1 + lengths[i] // hop_length frames are those of that clip run alone, bit for bit, the rest are
    NaN / 0 / 0.  No host synchronisation.  ValueError for an unsupported setting, before any launch; RuntimeError without
    a HIP device."""
    lead = tuple(y.shape[:-1])
    L = y.shape[-1]
    N = 1
    for d in lead:
        N *= d
    if y.dim() < 1 or N < 1 or L < 1:
        raise ValueError(f"pyin takes [..., L] with at least one sample and one waveform, got {tuple(y.shape)}")
    st = pyin_stages(y.reshape(N, L), fmin, fmax, sr, frame_length, win_length, hop_length, n_thresholds, beta_parameters,
                     boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob, lengths)
    T = st["shape"]["T"]
    return st["f0"].view(*lead, T), st["voiced_flag"].view(*lead, T), st["voiced_prob"].view(*lead, T)


def pitch_variation_summary(f0_clean, voiced_clean, f0_var, voiced_var):
    """What each (direction, alpha) does to the contour.  f0_clean, voiced_clean [B, T]; f0_var, voiced_var [B, K, A, T] ->
    dict of [B, K, A] tensors: 'shift_cents' = median over the frames voiced in both of 1200 log2(f0_var / f0_clean) (NaN
    where there is none; the lower of the two middle values for an even count, as torch.nanmedian), 'voicing_agreement' =
    share of frames with equal flags, 'n_joint_voiced'.  Plain torch ops; runs on CPU tensors too."""
    if f0_var.dim() != 4 or f0_clean.dim() != 2 or f0_var.shape[0] != f0_clean.shape[0] or f0_var.shape[-1] != f0_clean.shape[-1]:
        raise ValueError(f"contours {tuple(f0_clean.shape)} and {tuple(f0_var.shape)} do not fit [B, T] and [B, K, A, T]")
    vc = voiced_clean.bool()[:, None, None, :]
    vv = voiced_var.bool()
    joint = vc & vv
    cents = 1200.0 * torch.log2(f0_var.double() / f0_clean.double()[:, None, None, :])
    cents = torch.where(joint, cents, torch.full_like(cents, float("nan")))
    n_joint = joint.sum(-1)
    # nanmedian of an all-NaN row is NaN already; the where keeps that explicit
    shift = torch.where(n_joint > 0, torch.nanmedian(cents, dim=-1).values, torch.full_like(cents[..., 0], float("nan")))
    return {"shift_cents": shift.float(), "voicing_agreement": (vc == vv).float().mean(-1), "n_joint_voiced": n_joint}


def contours_of_variations(clean_wave, variations, fmin=80.0, fmax=400.0, sr=16000, **kw):
    """clean_wave [B, L] and variations [B, K, A, L] in ONE pyin call -> {'f0_clean' [B,T], 'voiced_flag_clean',
    'voiced_prob_clean', 'f0' [B,K,A,T], 'voiced_flag', 'voiced_prob', 'summary'}"""
    B, K, A, L = variations.shape
    both = torch.cat((clean_wave.reshape(B, 1, L), variations.reshape(B, K * A, L)), dim=1)
    f0, vf, vp = pyin(both, fmin, fmax, sr=sr, **kw)
    T = f0.shape[-1]
    out = {"f0_clean": f0[:, 0], "voiced_flag_clean": vf[:, 0], "voiced_prob_clean": vp[:, 0],
           "f0": f0[:, 1:].reshape(B, K, A, T), "voiced_flag": vf[:, 1:].reshape(B, K, A, T),
           "voiced_prob": vp[:, 1:].reshape(B, K, A, T)}
    out["summary"] = pitch_variation_summary(out["f0_clean"], out["voiced_flag_clean"], out["f0"], out["voiced_flag"])
    return out
