"""Speech-enhancement metrics on the device: STOI, SI-SDR and BSS-eval SDR of ragged batches (audio_zen/metrics.py:8-89,
use_pre_trained_model/model_validator/model_validator.py:56-65).

Every function takes [B, L] or [L] device tensors (clean / reference first, estimate second) and an optional per-item
`lengths` ([B] ints: the samples of row b past lengths[b] are padding and never read), and returns a [B] float64 device
tensor.  An item's value depends on its own samples only and is bit-identical in any batch and on every run.

- `si_sdr`: audio_zen's SI_SDR (no mean removal, no eps; +inf when the estimate is an exact multiple of the reference).
- `si_sdr_zero_mean`: ModelValidator.calculate_metrics' SI-SDR (both signals mean-removed, eps 1e-6).
- `stoi`: classic STOI (extended=False) at 16 kHz, the algorithm pystoi 0.3 implements, stated step by step in DESIGN.md
  ("Speech-enhancement metrics").  pystoi is not available to this project: agreement with pystoi itself is unverified;
  the kernels are tested stage by stage against a float64 numpy restatement of that contract.

- `sdr`: audio_zen's SDR, i.e. mir_eval.separation.bss_eval_sources for one source (the estimate projected on the span of
  `filter_length` = 512 delayed copies of the reference), as DESIGN.md section 7d "BSS-eval SDR" states it.  mir_eval is
  not available to this project: agreement with mir_eval itself is unverified; the kernels are tested stage by stage
  against a float64 numpy restatement of that contract (tests/bss_eval_ref.py).
- `scale_bss_eval`: audio_zen's _scale_bss_eval without SIR / SAR (si_sdr, sd_sdr, snr, srr).

PESQ (WB / NB) and MOSNET are registered names that raise NotImplementedError, so a metric list taken from train.toml fails
loudly instead of silently dropping a metric.
"""
import math

import numpy as np
import torch

from . import _hip as H

__all__ = ["si_sdr", "si_sdr_zero_mean", "si_sdr_both", "stoi", "stoi_stages", "resample_window", "REGISTERED_METRICS",
           "nppc_direction_scores", "sdr", "sdr_stages", "scale_bss_eval", "BSS_MAX_FILTER", "BSS_CORR_CHUNK",
           "BSS_CORR_TILE", "BSS_PROJ_CHUNK"]

SR = 16000
UP, DOWN = 5, 8                 # 16 kHz -> 10 kHz
N_FRAME, HOP, NUMBAND = 256, 128, 15

# csrc/bss_eval.hip (nppc_bss_shape reports the same numbers; tests/test_bss_eval_cpu.py keeps the two in step)
BSS_MAX_FILTER = 512            # longest projection filter
BSS_CORR_CHUNK = 8192           # samples per workgroup of the correlation kernel (one row of partial sums each)
BSS_CORR_TILE = 1024            # samples that workgroup stages in LDS at a time
BSS_PROJ_CHUNK = 1024           # output samples per workgroup of the projection kernel

_TAPS = {}


def resample_window(p=UP, q=DOWN):
    """pystoi's _resample_window_oct(p, q) normalised to unit sum (the window resample_oct hands to resample_poly):
    Kaiser-windowed sinc, cutoff 1 / (2 max(p, q)), 60 dB rejection; 581 taps for 5 / 8"""
    g = math.gcd(p, q)
    p, q = p // g, q // g
    rejection_db = 60.0
    stopband_cutoff_f = 1.0 / (2 * max(p, q))
    roll_off_width = stopband_cutoff_f / 10
    L = int(np.ceil((rejection_db - 8) / (28.714 * roll_off_width)))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stopband_cutoff_f * np.sinc(2 * stopband_cutoff_f * t)
    h = np.kaiser(2 * L + 1, 0.1102 * (rejection_db - 8.7)) * ideal
    return h / np.sum(h)


def _taps(device):
    key = str(device)
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(resample_window()).to(device)
    return _TAPS[key]


def _batch(ref, est, lengths):
    """(ref, est) as [B, L] fp32 contiguous device rows and lengths as a [B] int32 device tensor"""
    H.require_gpu()
    if not (isinstance(ref, torch.Tensor) and isinstance(est, torch.Tensor) and ref.is_cuda and est.is_cuda):
        raise RuntimeError("nppc_audio.metrics takes HIP device tensors")
    if ref.shape != est.shape or ref.dim() not in (1, 2):
        raise ValueError(f"reference {tuple(ref.shape)} and estimate {tuple(est.shape)} must be the same [B, L] or [L]")
    if ref.dim() == 1:
        ref, est = ref[None], est[None]
    ref, est = ref.contiguous().float(), est.contiguous().float()
    B, L = ref.shape
    if B == 0 or L == 0:
        raise ValueError("empty batch")
    if lengths is None:
        lens = torch.full((B,), L, dtype=torch.int32, device=ref.device)
    else:
        if not isinstance(lengths, torch.Tensor) or not lengths.is_cuda:
            host = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
            if host.numel() != B or int(host.min()) < 1 or int(host.max()) > L:
                raise ValueError(f"lengths must be {B} values in [1, {L}]")
        lens = torch.as_tensor(lengths).to(device=ref.device, dtype=torch.int32).reshape(-1).contiguous()
        if lens.numel() != B:
            raise ValueError(f"lengths must hold {B} values")
    return ref, est, lens


def si_sdr_both(ref, est, lengths=None, return_sums=False):
    """[B, 2] float64: column 0 = audio_zen SI_SDR, column 1 = ModelValidator's mean-removed SI-SDR (one launch)"""
    ref, est, lens = _batch(ref, est, lengths)
    B, L = ref.shape
    out = torch.empty(B, 2, dtype=torch.float64, device=ref.device)
    sums = torch.empty(B, 9, dtype=torch.float64, device=ref.device) if return_sums else None
    H.call("nppc_sisdr_sums", ref, est, lens, B, L, sums, out, H.stream())
    return (out, sums) if return_sums else out


def si_sdr(ref, est, lengths=None):
    """audio_zen/metrics.py:61-85 per item: 10 log10(|a s|^2 / |e - a s|^2), a = <s, e> / |s|^2 -> [B] float64"""
    return si_sdr_both(ref, est, lengths)[:, 0]


def si_sdr_zero_mean(ref, est, lengths=None):
    """model_validator.py:60-65 per item: mean-removed, a = <e, s> / (|s|^2 + 1e-6),
    20 log10(|a s| / (|a s - e| + 1e-6)) -> [B] float64"""
    return si_sdr_both(ref, est, lengths)[:, 1]


def stoi_stages(clean, est, sr=SR, lengths=None):
    """the STOI launch sequence with every intermediate kept: resampled signals xr / yr [B, Lr] and their lengths lr,
    frame energies / slot (kept position or -1) / kidx / K of the silence mask, band magnitudes x_tob / y_tob
    [B, 15, nfr] (the first K - 1 frames of each item are defined) and stoi [B]"""
    if sr != SR:
        raise ValueError(f"stoi: sr = {sr} is not supported; the resampler is designed for 16000 Hz input (5 / 8 to 10 kHz)")
    x, y, lens = _batch(clean, est, lengths)
    B, L = x.shape
    dev = x.device
    Lr = -(-L * UP // DOWN)
    nfr = max(1, -(-(Lr - N_FRAME) // HOP))
    h = _taps(dev)
    xr = torch.empty(B, Lr, dtype=torch.float64, device=dev)
    yr = torch.empty_like(xr)
    H.call("nppc_resample_poly", x, lens, B, L, h, h.numel(), UP, DOWN, xr, Lr, H.stream())
    H.call("nppc_resample_poly", y, lens, B, L, h, h.numel(), UP, DOWN, yr, Lr, H.stream())
    lr = torch.div(lens * UP + (DOWN - 1), DOWN, rounding_mode="floor").to(torch.int32)
    energy = torch.empty(B, nfr, dtype=torch.float64, device=dev)
    slot = torch.empty(B, nfr, dtype=torch.int32, device=dev)
    kidx = torch.empty_like(slot)
    K = torch.empty(B, dtype=torch.int32, device=dev)
    H.call("nppc_stoi_frames", xr, lr, B, Lr, nfr, energy, slot, kidx, K, H.stream())
    x_tob = torch.empty(B, NUMBAND, nfr, dtype=torch.float64, device=dev)
    y_tob = torch.empty_like(x_tob)
    H.call("nppc_stoi_bands", xr, yr, Lr, kidx, K, B, nfr, x_tob, y_tob, H.stream())
    out = torch.empty(B, dtype=torch.float64, device=dev)
    H.call("nppc_stoi_corr", x_tob, y_tob, K, B, nfr, out, H.stream())
    return dict(xr=xr, yr=yr, lr=lr, energy=energy, slot=slot, kidx=kidx, K=K, x_tob=x_tob, y_tob=y_tob, stoi=out)


def stoi(clean, est, sr=SR, lengths=None):
    """classic STOI (pystoi.stoi(clean, est, 16000, extended=False) as DESIGN.md states it) per item -> [B] float64;
    1e-5 for an item with fewer than 30 STFT frames after silence removal"""
    return stoi_stages(clean, est, sr, lengths)["stoi"]


def _filter_length(filter_length):
    if isinstance(filter_length, bool) or not isinstance(filter_length, (int, np.integer)) \
            or not 1 <= filter_length <= BSS_MAX_FILTER:
        raise ValueError(f"filter_length = {filter_length!r} must be an integer in [1, {BSS_MAX_FILTER}]")
    return int(filter_length)


def sdr_stages(ref, est, lengths=None, filter_length=512):
    """the BSS-eval SDR launch sequence with every intermediate kept.  Per item (s = ref, e = est, n samples, P =
    filter_length, M = n + P - 1): r [B, P] = sum_m s[m] s[m - t] and d [B, P] = sum_m e[m] s[m - t], c [B, P] the solution
    of toeplitz(r) c = d (Levinson-Durbin), num / den [B] = sum over all M samples of proj^2 / (e - proj)^2 with
    proj[m] = sum_t c[t] s[m - t], sdr [B] = 10 log10(num / den) (+inf when den == 0), status [B] int32 (non-zero: the
    solve broke down and num, den, sdr are NaN).  All float64."""
    P = _filter_length(filter_length)
    ref, est, lens = _batch(ref, est, lengths)
    B, L = ref.shape
    dev = ref.device
    n_corr = -(-L // BSS_CORR_CHUNK) * 2 * P
    n_proj = -(-(L + P - 1) // BSS_PROJ_CHUNK) * 2
    part = torch.empty(B * n_corr, dtype=torch.float64, device=dev)
    r = torch.empty(B, P, dtype=torch.float64, device=dev)
    d, c = torch.empty_like(r), torch.empty_like(r)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    H.call("nppc_bss_corr", ref, est, lens, B, L, P, part, part.numel(), H.stream())
    H.call("nppc_bss_solve", part, lens, B, L, P, r, d, c, status, H.stream())
    part2 = torch.empty(B * n_proj, dtype=torch.float64, device=dev)
    num = torch.empty(B, dtype=torch.float64, device=dev)
    den, out = torch.empty_like(num), torch.empty_like(num)
    H.call("nppc_bss_project", ref, est, lens, B, L, P, c, status, part2, part2.numel(), num, den, out, H.stream())
    return dict(r=r, d=d, c=c, status=status, num=num, den=den, sdr=out)


def sdr(ref, est, lengths=None, filter_length=512):
    """audio_zen/metrics.py:56-58 per item: mir_eval.separation.bss_eval_sources(ref[None], est[None])[0] as DESIGN.md
    section 7d states it (the classical SDR: a linear distortion of the reference shorter than filter_length samples, a
    delay included, is forgiven) -> [B] float64.  +inf when the estimate lies in the span exactly.  NaN for an item whose
    reference is all zeros (mir_eval raises ValueError there; a batched launch cannot) or whose Toeplitz solve breaks down
    (a non-positive pivot or prediction error); the other items are unaffected.  Unverified against mir_eval itself."""
    return sdr_stages(ref, est, lengths, filter_length)["sdr"]


def scale_bss_eval(ref, est, lengths=None, return_sums=False):
    """audio_zen/metrics.py:8-53 with compute_sir_sar=False per item, alpha = <s, e> / |s|^2 -> dict of [B] float64:
    si_sdr = 10 log10(|alpha s|^2 / |e - alpha s|^2), sd_sdr = snr + 10 log10(alpha^2), snr = 10 log10(|s|^2 / |e - s|^2),
    srr = -10 log10((1 - 1 / alpha)^2).  Every energy is summed directly in fp64 (no expansion, so no cancellation);
    return_sums adds "sums" [B, 4] = |s|^2, <s, e>, |e - s|^2, |e - alpha s|^2."""
    ref, est, lens = _batch(ref, est, lengths)
    B, L = ref.shape
    out = torch.empty(B, 4, dtype=torch.float64, device=ref.device)
    sums = torch.empty(B, 4, dtype=torch.float64, device=ref.device) if return_sums else None
    H.call("nppc_bss_scale", ref, est, lens, B, L, sums, out, H.stream())
    res = {"si_sdr": out[:, 0], "sd_sdr": out[:, 1], "snr": out[:, 2], "srr": out[:, 3]}
    if return_sums:
        res["sums"] = sums
    return res


def _not_built(name, reason):
    def metric(ref, est, sr=SR, lengths=None):
        raise NotImplementedError(f"{name}: {reason}")
    metric.__name__ = name
    return metric


def _stoi_metric(ref, est, sr=SR, lengths=None):
    return stoi(ref, est, sr=sr, lengths=lengths)


def _si_sdr_metric(ref, est, sr=SR, lengths=None):
    return si_sdr(ref, est, lengths=lengths)


def _sdr_metric(ref, est, sr=SR, lengths=None):
    return sdr(ref, est, lengths=lengths)


# audio_zen/metrics.py:143-149: only registered metrics can be used; each is metric(ref, est, sr=..) -> [B] float64 here
REGISTERED_METRICS = {
    "SI_SDR": _si_sdr_metric,
    "STOI": _stoi_metric,
    "SDR": _sdr_metric,
    "WB_PESQ": _not_built("WB_PESQ", "PESQ (ITU-T P.862) is not implemented in this build"),
    "NB_PESQ": _not_built("NB_PESQ", "PESQ (ITU-T P.862) is not implemented in this build"),
    "MOSNET": _not_built("MOSNET", "MOSNet needs a pretrained network this build does not have"),
}


def nppc_direction_scores(err_norm, err_proj_mag, w_norms):
    """How good are NPPC directions on held-out clips?  Pure host fp64 algebra on the loss's own per-item outputs (runs
    without a GPU): err_norm [B] = |e|, the norm of the restorer's error e = gt - pred in the compressed-cIRM domain;
    err_proj_mag [B, K] = |<w_k, e>| / (|w_k| |e|), the loss's normalised projection of e on direction k; w_norms [B, K]
    = |w_k| / |e|, the loss's normalised predicted spread.  The directions of an item are orthogonal (Gram-Schmidt), so
    squared projections add up.

      captured[b, k]  = sum_{j <= k} err_proj_mag[b, j]^2     share of the item's SQUARED error inside the span of its
                                                              first k + 1 directions (the loss's normalisation: already
                                                              divided by err_norm^2; times err_norm[b]^2 = absolute)
      residual[b, k]  = 1 - captured[b, k]                    residual[b, K - 1] is the loss's reconst_err[b]
      calibration[b, k] = err_proj_mag[b, k] / w_norms[b, k]  observed / predicted spread along direction k

    and over the whole set:
      captured_mean / residual_mean [K]: means over the items (residual_mean[K - 1] = the mean reconst_err);
      captured_pooled / residual_pooled [K]: sum_b captured[b, k] err_norm[b]^2 / sum_b err_norm[b]^2, the share of the
        set's total squared error (long and badly restored clips weigh more);
      calibration [K] = sqrt(mean_b err_proj_mag[b, k]^2) / sqrt(mean_b w_norms[b, k]^2): 1.0 means the predicted spread
        matches the observed one, below 1 the direction is over-confident about its own size.
    Returns a dict of float64 numpy arrays."""
    en = np.asarray(err_norm, dtype=np.float64).reshape(-1)
    pm = np.asarray(err_proj_mag, dtype=np.float64)
    wn = np.asarray(w_norms, dtype=np.float64)
    if pm.ndim != 2 or pm.shape != wn.shape or pm.shape[0] != en.shape[0]:
        raise ValueError(f"expected err_norm [B], err_proj_mag [B, K], w_norms [B, K]; got {en.shape}, {pm.shape}, {wn.shape}")
    if pm.shape[0] == 0:
        raise ValueError("nppc_direction_scores needs at least one item")
    captured = np.cumsum(pm * pm, axis=1)
    e2 = en * en
    tot = e2.sum()
    pooled = (captured * e2[:, None]).sum(axis=0) / tot if tot > 0 else np.full(pm.shape[1], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        cal_item = pm / wn
        cal = np.sqrt((pm * pm).mean(axis=0)) / np.sqrt((wn * wn).mean(axis=0))
    return {"captured": captured, "residual": 1.0 - captured, "calibration_item": cal_item,
            "captured_mean": captured.mean(axis=0), "residual_mean": 1.0 - captured.mean(axis=0),
            "captured_pooled": pooled, "residual_pooled": 1.0 - pooled, "calibration": cal}
