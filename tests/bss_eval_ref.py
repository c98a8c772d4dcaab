"""float64 numpy restatement of the BSS-eval SDR contract (DESIGN.md section 7d "BSS-eval SDR") and of audio_zen's
_scale_bss_eval: the yardstick of tests/test_bss_eval_cpu.py and tests/test_bss_eval_gpu.py.

SDR of one (reference s, estimate e) pair of n samples, filter length P, both zero-padded to M = n + P - 1 (what
mir_eval.separation.bss_eval_sources computes for one source; mir_eval is not available here, so agreement with mir_eval
itself is unverified):
    r[t] = sum_m s[m] s[m - t], d[t] = sum_m e[m] s[m - t], t < P     (direct sums)
    toeplitz(r) c = d                                                   (np.linalg.solve, lstsq on LinAlgError)
    proj = convolve(s, c)  (M samples), num = sum proj^2, den = sum (e_padded - proj)^2
    SDR = 10 log10(num / den), +inf when den == 0
"""
import numpy as np
import scipy.linalg
import scipy.signal


def correlations(s, e, P):
    """r, d [P] by direct sums: r[t] = sum_m s[m] s[m - t], d[t] = sum_m e[m] s[m - t] (the reference delayed by t)"""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    n = s.size
    r, d = np.zeros(P), np.zeros(P)
    for t in range(min(P, n)):
        r[t] = np.dot(s[t:], s[:n - t])
        d[t] = np.dot(e[t:], s[:n - t])
    return r, d


def correlations_fft(s, e, P):
    """the same numbers by the route mir_eval takes: FFTs of size 2^ceil(log2(M)), r = irfft(|S|^2)[:P] and
    d[t] = ifft(S conj(E)) at the indices [0], [-1], .., [-(P - 1)]"""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    M = s.size + P - 1
    n_fft = int(2 ** np.ceil(np.log2(M)))
    S, E = np.fft.rfft(s, n_fft), np.fft.rfft(e, n_fft)
    r = np.fft.irfft(np.abs(S) ** 2, n_fft)[:P]
    x = np.fft.irfft(S * np.conj(E), n_fft)
    d = np.hstack((x[0], x[-1:-P:-1]))
    return r, d


def solve(r, d, how="lu"):
    """toeplitz(r) c = d by LU (mir_eval's route: np.linalg.solve, lstsq on LinAlgError), lstsq, scipy's Levinson
    (solve_toeplitz) or the plain Levinson-Durbin recursion the device kernel runs"""
    if how == "lu":
        G = scipy.linalg.toeplitz(r)
        try:
            return np.linalg.solve(G, d)
        except np.linalg.LinAlgError:
            return np.linalg.lstsq(G, d, rcond=None)[0]
    if how == "lstsq":
        return np.linalg.lstsq(scipy.linalg.toeplitz(r), d, rcond=None)[0]
    if how == "toeplitz":
        return scipy.linalg.solve_toeplitz(r, d)
    if how == "levinson":
        return levinson(r, d)
    raise ValueError(how)


def levinson(r, d):
    """Levinson-Durbin for toeplitz(r) x = d in float64; None on a breakdown (a prediction error that is not positive)"""
    P = r.size
    if not r[0] > 0:
        return None
    a = np.zeros(P)
    a[0] = 1.0
    x = np.zeros(P)
    x[0] = d[0] / r[0]
    E = r[0]
    for k in range(1, P):
        kappa = -np.dot(a[:k], r[k:0:-1]) / E
        a[:k + 1] = a[:k + 1] + kappa * a[k::-1]
        E = E * (1.0 - kappa * kappa)
        if not (E > 0 and np.isfinite(E)):
            return None
        mu = (d[k] - np.dot(x[:k], r[k:0:-1])) / E
        x[:k + 1] += mu * a[k::-1]
    return x


def residual(r, d, c):
    """|toeplitz(r) c - d| / |d|"""
    return float(np.linalg.norm(scipy.linalg.toeplitz(r) @ c - d) / np.linalg.norm(d))


def project(s, e, c):
    """num = sum proj^2 and den = sum (e_padded - proj)^2 over all M = n + P - 1 samples"""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    proj = np.convolve(s, c)                              # n + P - 1 samples
    ep = np.zeros(proj.size)
    ep[:e.size] = e
    return float(np.sum(proj ** 2)), float(np.sum((ep - proj) ** 2))


def sdr_stages(s, e, P=512, how="lu"):
    r, d = correlations(s, e, P)
    if not np.any(np.asarray(s) != 0):
        nan = float("nan")
        return dict(r=r, d=d, c=np.full(P, nan), num=nan, den=nan, sdr=nan)
    c = solve(r, d, how)
    num, den = project(s, e, c)
    with np.errstate(divide="ignore"):
        val = float("inf") if den == 0 else float(10 * np.log10(num / den))
    return dict(r=r, d=d, c=c, num=num, den=den, sdr=val)


def sdr(s, e, P=512, how="lu"):
    return sdr_stages(s, e, P, how)["sdr"]


SOLVERS = ("lu", "lstsq", "toeplitz")


def solver_spread(s, e, P):
    """max - min of the SDR (dB) over LU, lstsq and scipy's Levinson: how well-posed the yardstick is on this input"""
    r, d = correlations(s, e, P)
    vals = []
    for how in SOLVERS:
        num, den = project(s, e, solve(r, d, how))
        vals.append(10 * np.log10(num / den))
    return float(max(vals) - min(vals))


def scale_bss_eval(s, e):
    """audio_zen/metrics.py:8-53 with compute_sir_sar=False, restated: dict si_sdr, sd_sdr, snr, srr (dB)"""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    energy = np.sum(s ** 2)
    alpha = np.dot(s, e) / energy
    snr = 10 * np.log10(energy / np.sum((e - s) ** 2))
    scaled = alpha * s
    si_sdr = 10 * np.log10(np.sum(scaled ** 2) / np.sum((e - scaled) ** 2))
    srr = -10 * np.log10((1 - 1 / alpha) ** 2)
    sd_sdr = snr + 10 * np.log10(alpha ** 2)
    return dict(si_sdr=float(si_sdr), sd_sdr=float(sd_sdr), snr=float(snr), srr=float(srr))


def si_sdr(s, e):
    return scale_bss_eval(s, e)["si_sdr"]


# ---- inputs ------------------------------------------------------------------------------------------------------------
FILTER_TAPS = 20


def make_pair(seed, n):
    """(reference, estimate) fp32 [n]: the reference is low-passed (one pole at 0.9) white noise, amplitude-modulated at
    3 Hz (16 kHz); the estimate is the reference through a decaying 20-tap filter plus white noise 26 dB below it"""
    rng = np.random.default_rng(seed)
    x = scipy.signal.lfilter([1.0], [1.0, -0.9], rng.standard_normal(n + 64))[64:]
    x *= (1.0 + 0.6 * np.sin(2 * np.pi * 3.0 * np.arange(n) / 16000.0 + seed)) * 0.1
    h = rng.standard_normal(FILTER_TAPS) * np.exp(-0.25 * np.arange(FILTER_TAPS))
    h[0] = 1.0
    y = np.convolve(x, h)[:n] + 0.05 * np.std(x) * rng.standard_normal(n) if n > 1 else 0.8 * x + 0.01
    return x.astype(np.float32), np.asarray(y).astype(np.float32)


def make_batch(lengths, seed0=0):
    return [make_pair(seed0 + 17 * i, n) for i, n in enumerate(lengths)]
