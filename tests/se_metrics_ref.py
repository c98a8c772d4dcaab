"""fp64 numpy oracle of the speech-enhancement metrics (nppc_audio/metrics.py).

SI-SDR: audio_zen/metrics.py:61-85 (`si_sdr`) and use_pre_trained_model/model_validator/model_validator.py:60-65
(`si_sdr_zero_mean`), restated in float64.

STOI: classic STOI (Taal et al. 2011, extended=False) as pystoi 0.3 computes it, written out step by step from the
project's contract ("Speech-enhancement metrics").  pystoi itself is not available to this project, so
agreement with pystoi is unverified; this module IS the definition the HIP kernels are tested against.  Every stage is a
separate function so the GPU tests can compare stage by stage.
"""
import math

import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME = 256
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40
EPS = np.finfo(np.float64).eps
HOP = N_FRAME // 2


# ---- SI-SDR --------------------------------------------------------------------------------------------------------------
def si_sdr(ref, est):
    """audio_zen.metrics.SI_SDR in float64: no mean removal, no eps (+inf when est is an exact multiple of ref)"""
    ref, est = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    alpha = np.sum(ref * est) / np.sum(ref ** 2)
    proj = alpha * ref
    noise = est - proj
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(np.sum(proj ** 2) / np.sum(noise ** 2)))


def si_sdr_zero_mean(ref, est):
    """ModelValidator.calculate_metrics' SI-SDR in float64 (mean-removed, eps 1e-6 in both places)"""
    ref, est = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    e = est - np.mean(est)
    s = ref - np.mean(ref)
    alpha = np.dot(e, s) / (np.linalg.norm(s) ** 2 + 1e-6)
    return float(20 * np.log10(np.linalg.norm(alpha * s) / (np.linalg.norm(alpha * s - e) + 1e-6)))


# ---- STOI ----------------------------------------------------------------------------------------------------------------
def resample_window(p=5, q=8):
    """pystoi's _resample_window_oct(p, q) (an Octave port): Kaiser-windowed sinc, 60 dB rejection"""
    g = math.gcd(p, q)
    p, q = p // g, q // g
    log10_rejection = -3.0
    stopband_cutoff_f = 1.0 / (2 * max(p, q))
    roll_off_width = stopband_cutoff_f / 10
    rejection_db = -20 * log10_rejection
    L = np.ceil((rejection_db - 8) / (28.714 * roll_off_width))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stopband_cutoff_f * np.sinc(2 * stopband_cutoff_f * t)
    beta = 0.1102 * (rejection_db - 8.7)       # rejection_db = 60 > 50
    return np.kaiser(int(2 * L + 1), beta) * ideal


def resample_taps():
    """the normalised window resample_poly gets: h / sum(h)"""
    h = resample_window(5, 8)
    return h / np.sum(h)


def resample(x):
    """step 1: 16 kHz -> 10 kHz, resample_poly(x, 5, 8, window=h / sum(h))"""
    return resample_poly(np.asarray(x, np.float64), 5, 8, window=resample_taps())


def hann256():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_energies(x):
    """20 log10(||w x[i:i+256]|| + EPS) for i in range(0, len(x) - 256, 128)"""
    w = hann256()
    fr = np.array([w * x[i:i + N_FRAME] for i in range(0, len(x) - N_FRAME, HOP)]).reshape(-1, N_FRAME)
    return 20 * np.log10(np.linalg.norm(fr, axis=1) + EPS)


def keep_mask(x):
    """step 2 mask: (max energy - 40 - energy) < 0, and the signed distance to the threshold in dB"""
    e = frame_energies(x)
    if e.size == 0:
        return np.zeros(0, bool), np.zeros(0)
    margin = np.max(e) - DYN_RANGE - e
    return margin < 0, margin


def remove_silent_frames(x, y):
    """step 2: overlap-add of the kept windowed frames of x and of y (the frames x selects)"""
    w = hann256()
    idx = range(0, len(x) - N_FRAME, HOP)
    xf = np.array([w * x[i:i + N_FRAME] for i in idx]).reshape(-1, N_FRAME)
    yf = np.array([w * y[i:i + N_FRAME] for i in idx]).reshape(-1, N_FRAME)
    mask, _ = keep_mask(x)
    xf, yf = xf[mask], yf[mask]
    n_sil = (len(xf) - 1) * HOP + N_FRAME
    xs, ys = np.zeros(max(n_sil, 0)), np.zeros(max(n_sil, 0))
    for i in range(xf.shape[0]):
        xs[i * HOP:i * HOP + N_FRAME] += xf[i]
        ys[i * HOP:i * HOP + N_FRAME] += yf[i]
    return xs, ys


def stft_power(s):
    """step 3: |rfft(w s[i:i+256], 512)|^2 for i in range(0, len(s) - 256, 128) -> [frames, 257]"""
    w = hann256()
    fr = [np.fft.rfft(w * s[i:i + N_FRAME], n=NFFT) for i in range(0, len(s) - N_FRAME, HOP)]
    return np.square(np.abs(np.array(fr).reshape(-1, NFFT // 2 + 1)))


def band_edges(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """pystoi's thirdoct(): (lo, hi) bin range of every third-octave band, hi exclusive"""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    cf = np.power(2.0 ** (1.0 / 3), k) * min_freq
    freq_low = min_freq * np.power(2.0, (2 * k - 1) / 6)
    freq_high = min_freq * np.power(2.0, (2 * k + 1) / 6)
    out = []
    for i in range(len(cf)):
        lo = int(np.argmin(np.square(f - freq_low[i])))
        hi = int(np.argmin(np.square(f - freq_high[i])))
        out.append((lo, hi))
    return out


def obm():
    m = np.zeros((NUMBAND, NFFT // 2 + 1))
    for k, (lo, hi) in enumerate(band_edges()):
        m[k, lo:hi] = 1
    return m


def third_octave(power):
    """step 4: tob = sqrt(OBM @ |X|^2): [frames, 257] -> [15, frames]"""
    return np.sqrt(obm() @ power.T)


def correlate(x_tob, y_tob):
    """step 5: mean correlation of the clipped, normalised 30-frame segments (1e-5 for fewer than 30 frames)"""
    T = x_tob.shape[1]
    if T < N:
        return 1e-5
    xs = np.array([x_tob[:, m - N:m] for m in range(N, T + 1)])
    ys = np.array([y_tob[:, m - N:m] for m in range(N, T + 1)])
    norm_const = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yn = ys * norm_const
    clip_value = 10 ** (-BETA / 20)
    yp = np.minimum(yn, xs * (1 + clip_value))
    yp = yp - np.mean(yp, axis=2, keepdims=True)
    xs = xs - np.mean(xs, axis=2, keepdims=True)
    yp /= (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xs /= (np.linalg.norm(xs, axis=2, keepdims=True) + EPS)
    J, M = xs.shape[0], xs.shape[1]
    return float(np.sum(yp * xs) / (J * M))


def stoi_stages(clean, est):
    """every intermediate of one item: resampled signals, keep mask (+ margin), K, band magnitudes, STOI"""
    xr, yr = resample(clean), resample(est)
    mask, margin = keep_mask(xr)
    xs, ys = remove_silent_frames(xr, yr)
    x_tob, y_tob = third_octave(stft_power(xs)), third_octave(stft_power(ys))
    return dict(xr=xr, yr=yr, mask=mask, margin=margin, K=int(mask.sum()), x_tob=x_tob, y_tob=y_tob,
                stoi=correlate(x_tob, y_tob))


def stoi(clean, est):
    return stoi_stages(clean, est)["stoi"]


# ---- test inputs ---------------------------------------------------------------------------------------------------------
RAGGED_SECONDS = [0.3, 1.0, 2.5, 4.0, 10.0, 0.7, 1.7, 6.0]


def ragged_batch(seconds=RAGGED_SECONDS, seed=7):
    """(clean, est, lengths) float32 numpy [B, Lmax] x2 + [B]: speech-like clips with silent stretches, peak 1, and
    noisy / garbled / scaled estimates; the padding is zero (tests overwrite it with garbage)"""
    from scipy.signal import lfilter
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [int(round(s * 16000)) for s in seconds]
    B, Lm = len(lens), max(lens)
    clean = np.zeros((B, Lm), np.float32)
    est = np.zeros((B, Lm), np.float32)
    for b, n in enumerate(lens):
        t = np.arange(n) / 16000.0
        col = lfilter([0.05], [1.0, -0.95], rng.standard_normal(n))
        env = 0.5 * (1.0 - np.cos(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi)))
        c = col * (0.05 + env)
        for _ in range(max(1, n // 24000)):            # silent stretches of 0.1 - 0.4 s
            m = min(int(rng.integers(1600, 6400)), n // 4)
            a = int(rng.integers(0, n - m))
            c[a:a + m] = 0.0
        c /= np.max(np.abs(c))
        kind = b % 4
        if kind == 0:                                  # white noise at 0 - 10 dB SNR
            nz = rng.standard_normal(n)
            e = c + nz * np.sqrt(np.mean(c ** 2) / 10 ** (rng.uniform(0, 1)) / np.mean(nz ** 2))
        elif kind == 1:                                # garbled: low-passed, delayed, scaled
            e = 0.4 * lfilter([0.25, 0.5, 0.25], [1.0], np.roll(c, 37)) + 0.01 * rng.standard_normal(n)
        elif kind == 2:                                # babble-like: a second clip mixed in
            e = c + 0.5 * np.roll(c, n // 3)[::-1]
        else:                                          # mild noise, scaled estimate
            e = 0.3 * (c + 0.05 * rng.standard_normal(n))
        clean[b, :n], est[b, :n] = c, e
    return clean, est, np.array(lens, np.int64)
