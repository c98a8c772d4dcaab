"""fp64 numpy restatement of nppc_audio.resample (torchaudio's default Resample: a Hann-windowed sinc bank applied as a
strided convolution), the brute-force support / gap mapping over the bank's nonzero taps, and the native-rate splice of
RecordingRestorer.restore(..., sample_rate=...).  Shares no code with the package."""
import math

import numpy as np

RATIOS = [(441, 160), (160, 441), (3, 1), (1, 3), (2, 1), (1, 2), (441, 320), (441, 640), (3, 2), (2, 3), (7, 5)]
U = 2.0 ** -24


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def full_bank(orig_freq, new_freq, lpw=6, rolloff=0.99):
    """-> (kern [new, Klen] fp64, clamped [new, Klen] bool, width)"""
    orig, new = reduced(orig_freq, new_freq)
    base = min(orig, new) * rolloff
    width = int(math.ceil(lpw * orig / base))
    k = np.arange(2 * width + orig, dtype=np.float64)
    p = np.arange(new, dtype=np.float64)[:, None]
    t = (-p / new + (k[None] - width) / orig) * base
    clamped = (t <= -lpw) | (t >= lpw)
    t = np.clip(t, -lpw, lpw)
    window = np.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return sinc * window * (base / orig), clamped, width


def bank32(orig_freq, new_freq, lpw=6, rolloff=0.99):
    """the fp32 bank the implementations multiply by -> (kern [new, Klen] float32, width)"""
    kern, _, width = full_bank(orig_freq, new_freq, lpw, rolloff)
    return kern.astype(np.float32), width


def out_length(n, orig_freq, new_freq):
    orig, new = reduced(orig_freq, new_freq)
    return -(-new * int(n) // orig)


def resample(x, orig_freq, new_freq, lpw=6, rolloff=0.99, live=None):
    """x [n] -> (y [ceil(new n / orig)] fp64, bound [same]) with the fp32 taps upcast; bound[j] = sum_k |h_k x_k|, the
    factor of the rounding bound gamma_n.  live: None, or (k0 [new], count [new]) to assert nothing else contributes"""
    orig, new = reduced(orig_freq, new_freq)
    kern, width = bank32(orig_freq, new_freq, lpw, rolloff)
    kern = kern.astype(np.float64)
    klen = kern.shape[1]
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    target = -(-new * n // orig)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    frames = (n + 2 * width + orig - klen) // orig + 1
    xpad = np.concatenate([np.zeros(width), x, np.zeros(width + orig)])
    win = np.lib.stride_tricks.sliding_window_view(xpad, klen)[::orig][:frames]      # [frames, Klen]
    y = (win @ kern.T).reshape(-1)[:target]
    bound = (np.abs(win) @ np.abs(kern).T).reshape(-1)[:target]
    return y, bound


def gamma(n):
    return n * U / (1.0 - n * U)


def support(j, orig_freq, new_freq, lpw=6, rolloff=0.99, _cache={}):
    """[lo, hi) of the input samples under the NONZERO fp32 taps of output j"""
    orig, new = reduced(orig_freq, new_freq)
    key = (orig, new, lpw, rolloff)
    if key not in _cache:
        kern, width = bank32(orig, new, lpw, rolloff)
        rows = []
        for p in range(new):
            nz = np.nonzero(kern[p])[0]
            rows.append((int(nz[0]), int(nz[-1]) + 1))
        _cache[key] = (rows, width)
    rows, width = _cache[key]
    i, p = divmod(int(j), new)
    return i * orig - width + rows[p][0], i * orig - width + rows[p][1]


def map_gap(s, e, n_in, orig_freq, new_freq, lpw=6, rolloff=0.99):
    """brute force over EVERY output of an input of n_in samples: the hull of those whose support meets [s, e)"""
    hits = [j for j in range(out_length(n_in, orig_freq, new_freq))
            if (lambda r: r[1] > s and r[0] < e)(support(j, orig_freq, new_freq, lpw, rolloff))]
    return (hits[0], hits[-1] + 1) if hits else None


def native_crossfade(crossfade_samples, rate, model_rate):
    return -(-int(crossfade_samples) * int(rate) // int(model_rate))


def merge_gaps(gaps, xf):
    """sorted; two gaps closer than 2 xf become their hull"""
    pairs = sorted((int(s), int(e)) for s, e in gaps)
    merged = [pairs[0]]
    for s, e in pairs[1:]:
        if s - merged[-1][1] < 2 * xf:
            merged[-1] = (merged[-1][0], max(merged[-1][1], e))
        else:
            merged.append((s, e))
    return merged


def splice_native(wave, up, gaps, xf):
    """fp64: wave [N] the input, up [>= N] the upsampled restoration, gaps merged (regions [s - xf, e + xf) disjoint):
    inside a gap `up`; over the xf samples on either side wave + c (up - wave) with c = 0.5 - 0.5 cos(pi (t + 1) / (xf + 1)),
    t = 0 at the outer end of the ramp; every other sample is wave's.  -> (out [N] fp64, touched [N] bool)"""
    wave = np.asarray(wave, dtype=np.float64)
    up = np.asarray(up, dtype=np.float64)
    N = wave.size
    out = wave.copy()
    touched = np.zeros(N, dtype=bool)
    for s, e in gaps:
        for n in range(max(s - xf, 0), min(e + xf, N)):
            touched[n] = True
            if s <= n < e:
                out[n] = up[n]
            else:
                t = n - (s - xf) if n < s else e + xf - 1 - n
                c = 0.5 - 0.5 * math.cos(math.pi * (t + 1) / (xf + 1))
                out[n] = wave[n] + c * (up[n] - wave[n])
    return out, touched
