"""fp64 numpy restatement of the DNS dynamic mixer's per-sample arithmetic (fullsubnet_plus/dataset/dataset_train.py:146-182,
audio_zen/acoustics/feature.py:98-113): np.convolve in fp64 for the room impulse response, snr_mix line by line.  The two
random draws inside snr_mix (RIR channel, output level) are arguments here."""
import numpy as np

EPS = 1e-6


def rir_convolve(clean, rir):
    """fftconvolve(clean, rir)[:len(clean)] as a direct convolution in fp64; rir None or empty = dry"""
    clean = np.asarray(clean, dtype=np.float64)
    if rir is None or len(rir) == 0:
        return clean.copy()
    return np.convolve(clean, np.asarray(rir, dtype=np.float64))[:len(clean)]


def tailor_dB_FS(y, target_dB_FS, eps=EPS):
    rms = np.sqrt(np.mean(y ** 2))
    scalar = 10 ** (target_dB_FS / 20) / (rms + eps)
    return y * scalar, rms, scalar


def snr_mix(clean_y, noise_y, snr, target_dB_FS, noisy_target_dB_FS, rir=None, eps=EPS, info=None):
    """(noisy, clean) in fp64; info (a dict) receives max|noisy| before the clip rule and whether it fired"""
    clean_y = rir_convolve(clean_y, rir)
    noise_y = np.asarray(noise_y, dtype=np.float64)
    clean_y = clean_y / (np.max(np.abs(clean_y)) + eps)
    clean_y, _, _ = tailor_dB_FS(clean_y, target_dB_FS)
    clean_rms = (clean_y ** 2).mean() ** 0.5
    noise_y = noise_y / (np.max(np.abs(noise_y)) + eps)
    noise_y, _, _ = tailor_dB_FS(noise_y, target_dB_FS)
    noise_rms = (noise_y ** 2).mean() ** 0.5
    snr_scalar = clean_rms / (10 ** (snr / 20)) / (noise_rms + eps)
    noise_y = noise_y * snr_scalar
    noisy_y = clean_y + noise_y
    noisy_y, _, noisy_scalar = tailor_dB_FS(noisy_y, noisy_target_dB_FS)
    clean_y = clean_y * noisy_scalar
    peak = float(np.max(np.abs(noisy_y)))
    clipped = bool(np.any(np.abs(noisy_y) > 0.999))
    if info is not None:
        info["peak_before_guard"], info["clipped"] = peak, clipped
    if clipped:
        noisy_y_scalar = np.max(np.abs(noisy_y)) / (0.99 - eps)
        noisy_y = noisy_y / noisy_y_scalar
        clean_y = clean_y / noisy_y_scalar
    return noisy_y, clean_y


def rel_peak(got, want):
    """max |got - want| over the peak of want (1 when want is all zero)"""
    want = np.asarray(want, dtype=np.float64)
    peak = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))) / (peak if peak > 0 else 1.0)


def limit(e_ref):
    """the fixture rule: three times the reference's own fp32 error, floored at one fp32 ulp of the peak"""
    return max(3.0 * e_ref, 2.0 ** -23)
