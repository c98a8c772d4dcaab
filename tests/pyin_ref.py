"""fp64 NumPy / SciPy restatement of pYIN (Mauch & Dixon 2014) with librosa's parameterisation: the specification of
csrc/pitch.hip and nppc_audio/pitch.py.  librosa is not available to this project, so nothing here was compared with
librosa.pyin itself ("Unverified").

Decisions this file fixes (the kernels follow them):
- Framing: zero padding of frame_length // 2 on both sides, T = 1 + L // hop_length frames, frame t starts at t * hop_length
  of the padded signal.
- Lag range: min_period = max(floor(sr / fmax), 1), max_period = min(ceil(sr / fmin), frame_length - win_length - 1).
- Difference function d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 for tau = 0..max_period, formed directly in fp64 (no
  energy-minus-correlation form).  Energies below 1e-6 are noise of the arithmetic, as in librosa's yin: d(tau) < 1e-6 is
  replaced by 0 BEFORE the cumulative mean.  d'(tau) = d(tau) / (mean_{u = 1..tau} d(u) + tiny) with tiny = the smallest
  normal fp64, kept for tau = min_period..max_period.  A frame of digital silence has d = 0, so d' = 0 everywhere, no lag is
  strictly below a neighbour, there is no trough and the frame is unvoiced with voiced_prob = 0.
- Parabolic shift at an interior lag with neighbours (a, b, c): den = a - 2 b + c, shift = clip((a - c) / (2 den), -1, 1),
  0 where den == 0 and at both ends.
- Troughs: an interior lag is a trough if d' is strictly below its left neighbour and not above its right one; the first
  lag if strictly below its right neighbour; the last lag if strictly below its left neighbour (the right neighbour of the
  last lag is the lag itself, edge replication).
- Thresholds s_i = i / n_thresholds in fp64, compared as (fp64) d' < s_i.  Threshold weights w_i = differences of the
  Beta(a, b) CDF at s_{i-1}, s_i.  For threshold i the n troughs below it are ranked in lag order, the trough of rank r gets
  boltzmann.pmf(r, lambda, n) = (1 - e^-lambda) e^(-lambda r) / (1 - e^(-lambda n)) times w_i.  A threshold with no trough
  below it gives no_trough_prob * w_i to the lowest trough of the frame (the lowest lag among equals); a frame with no
  trough at all gets nothing.
- Pitch bins: f0 = sr / (min_period + index + shift), bin = round_half_even(12 nbps log2(f0 / fmin)) clipped to
  [0, n_pitch_bins - 1], always in fp64; probabilities landing in one bin ADD, in lag order.  voiced_prob =
  clip(sum of the bins, 0, 1); each of the n_pitch_bins unvoiced states gets (1 - voiced_prob) / n_pitch_bins.
- HMM: triangular window tri[d] = 1 - |d - half| / (half + 1), d = 0..width-1, half = width // 2,
  width = 2 * round_half_even(max_transition_rate * 12 * hop_length / sr) * nbps + 1, truncated at the edges and renormalised
  per source row; Kronecker product with the voicing switch matrix; uniform initial distribution.
- Viterbi in the log domain in fp64 with exactly this arithmetic (so that a second implementation can be bit-identical):
  log observation lo = log(obs + tiny);  a[v, i] = value[v, i] - log(rowsum_i);
  M_v[j] = max_i (a[v, i] + log tri[j - i + half]) over the window, the lowest i among equals;
  c_v = M_v[j] + log switch(v, v');  the predecessor voicing is v = 1 only if c_1 > c_0;  value'[v', j] = max(c_0, c_1) + lo.
  State index = v * n_pitch_bins + bin with v = 0 voiced.  The lowest final state wins ties.
- Outputs: f0 = fmin * 2^(bin / (12 nbps)) as fp32, NaN where unvoiced; voiced_flag; voiced_prob as fp32.
"""
import math

import numpy as np
import scipy.stats

TINY = float(np.finfo(np.float64).tiny)

DEFAULTS = dict(sr=16000, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
                boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)


class Setting:
    def __init__(self, fmin, fmax, **kw):
        p = dict(DEFAULTS)
        p.update(kw)
        self.fmin, self.fmax, self.sr = float(fmin), float(fmax), float(p["sr"])
        self.frame_length = int(p["frame_length"])
        self.win_length = int(p["win_length"]) if p["win_length"] is not None else self.frame_length // 2
        self.hop_length = int(p["hop_length"]) if p["hop_length"] is not None else self.frame_length // 4
        self.n_thresholds = int(p["n_thresholds"])
        self.beta_parameters = tuple(p["beta_parameters"])
        self.boltzmann_parameter = float(p["boltzmann_parameter"])
        self.resolution = float(p["resolution"])
        self.max_transition_rate = float(p["max_transition_rate"])
        self.switch_prob = float(p["switch_prob"])
        self.no_trough_prob = float(p["no_trough_prob"])
        self.min_period = max(int(math.floor(self.sr / self.fmax)), 1)
        self.max_period = min(int(math.ceil(self.sr / self.fmin)), self.frame_length - self.win_length - 1)
        if self.frame_length > 2048 or not (1 <= self.min_period < self.max_period < self.frame_length - self.win_length):
            raise ValueError("unsupported pYIN setting")
        self.P = self.max_period - self.min_period + 1
        self.nbps = int(math.ceil(1.0 / self.resolution))
        self.n_pitch_bins = int(math.floor(12 * self.nbps * math.log2(self.fmax / self.fmin))) + 1
        self.width = 2 * int(round(self.max_transition_rate * 12 * self.hop_length / self.sr)) * self.nbps + 1

    def n_frames(self, L):
        return 1 + L // self.hop_length

    def beta_weights(self):
        s = np.arange(self.n_thresholds + 1, dtype=np.float64) / self.n_thresholds
        return np.diff(scipy.stats.beta.cdf(s, self.beta_parameters[0], self.beta_parameters[1]))

    def hmm_tables(self):
        """(log tri [width], log rowsum [n_pitch_bins], log stay, log switch, log init) in fp64"""
        half = self.width // 2
        d = np.arange(self.width, dtype=np.float64)
        tri = 1.0 - np.abs(d - half) / (half + 1.0)
        nb = self.n_pitch_bins
        rows = np.empty(nb, dtype=np.float64)
        for i in range(nb):
            lo, hi = max(0, i - half), min(nb - 1, i + half)
            rows[i] = np.sum(tri[lo - i + half:hi - i + half + 1])
        return (np.log(tri), np.log(rows), float(np.log(1.0 - self.switch_prob)), float(np.log(self.switch_prob)),
                float(np.log(1.0 / (2 * nb))))


def frames_of(y, s):
    """[L] -> [T, frame_length] fp64 frames of the zero-padded signal"""
    y = np.asarray(y, dtype=np.float64)
    pad = s.frame_length // 2
    yp = np.concatenate([np.zeros(pad), y, np.zeros(pad)])
    T = s.n_frames(len(y))
    idx = np.arange(T)[:, None] * s.hop_length + np.arange(s.frame_length)[None, :]
    return yp[idx]


def difference(frames, s, dtype=np.float64):
    """d(tau), tau = 0..max_period: [T, max_period + 1]"""
    x = frames.astype(dtype)
    W = s.win_length
    d = np.empty((x.shape[0], s.max_period + 1), dtype=dtype)
    for tau in range(s.max_period + 1):
        e = x[:, :W] - x[:, tau:tau + W]
        d[:, tau] = np.sum(e * e, axis=1, dtype=dtype)
    return d


def cmnd(y, s, dtype=np.float64):
    """waveform [L] -> d' [T, P] (fp64 unless dtype says otherwise)"""
    d = difference(frames_of(y, s), s, dtype)
    d = np.where(d < dtype(1e-6), dtype(0), d)
    tau = np.arange(1, s.max_period + 1, dtype=dtype)
    mean = np.cumsum(d[:, 1:], axis=1, dtype=dtype) / tau
    dp = d[:, 1:] / (mean + dtype(TINY) if dtype == np.float64 else mean + np.finfo(dtype).tiny)
    return dp[:, s.min_period - 1:]


def parabolic_shifts(dp):
    dp = np.asarray(dp, dtype=np.float64)
    sh = np.zeros_like(dp)
    a, b, c = dp[:, :-2], dp[:, 1:-1], dp[:, 2:]
    den = a - 2.0 * b + c
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.clip((a - c) / (2.0 * den), -1.0, 1.0)
    sh[:, 1:-1] = np.where(den == 0.0, 0.0, v)
    return sh


def troughs_of(row):
    n = len(row)
    is_t = np.zeros(n, dtype=bool)
    is_t[1:-1] = (row[1:-1] < row[:-2]) & (row[1:-1] <= row[2:])
    is_t[0] = row[0] < row[1]
    is_t[-1] = row[-1] < row[-2]
    return np.nonzero(is_t)[0]


def observe(dp, s, dtype=np.float64):
    """d' [T, P] (any float type; read as given) -> (obs [T, 2 n_pitch_bins], voiced_prob [T]) in `dtype`.  Branches (troughs,
    thresholds, bins) are always taken in fp64 on the values given; `dtype` is the type of the probability arithmetic."""
    dp64 = np.asarray(dp, dtype=np.float64)
    T, P = dp64.shape
    nb, nth = s.n_pitch_bins, s.n_thresholds
    thr = np.arange(1, nth + 1, dtype=np.float64) / nth
    w = s.beta_weights().astype(dtype)
    shifts = parabolic_shifts(dp64)
    obs = np.zeros((T, 2 * nb), dtype=dtype)
    vp = np.zeros(T, dtype=dtype)
    lam = s.boltzmann_parameter
    for t in range(T):
        row = dp64[t]
        tr = troughs_of(row)
        if len(tr):
            h = row[tr]
            below = np.less.outer(h, thr)                              # [n_troughs, n_thresholds]
            rank = np.cumsum(below, axis=0) - 1
            n = np.count_nonzero(below, axis=0)
            with np.errstate(all="ignore"):
                prior = scipy.stats.boltzmann.pmf(rank, lam, np.maximum(n, 1)[None, :])
            prior = np.where(below, prior, 0.0).astype(dtype)
            probs = np.zeros(len(tr), dtype=dtype)
            for i in range(nth):                                       # thresholds in ascending order
                probs = probs + prior[:, i] * w[i]
            gmin = int(np.argmin(h))
            extra = dtype(0)
            for i in range(nth):
                if n[i] == 0:
                    extra = extra + w[i]
            probs[gmin] = probs[gmin] + dtype(s.no_trough_prob) * extra
            period = s.min_period + tr + shifts[t, tr]
            f0 = s.sr / period
            b = np.clip(np.round(12 * s.nbps * np.log2(f0 / s.fmin)), 0, nb - 1).astype(np.int64)
            for k in range(len(tr)):                                   # lag order
                obs[t, b[k]] = obs[t, b[k]] + probs[k]
        tot = dtype(0)
        tot = np.sum(obs[t, :nb], dtype=dtype)
        vp[t] = min(max(tot, dtype(0)), dtype(1))
        obs[t, nb:] = (dtype(1) - vp[t]) / dtype(nb)
    return obs, vp


def viterbi(obs, s):
    """obs [T, 2 n_pitch_bins] (any float type) -> states [T] int64, the arithmetic of the module docstring"""
    obs = np.asarray(obs, dtype=np.float64)
    T, S = obs.shape
    nb = s.n_pitch_bins
    assert S == 2 * nb
    ltri, lrow, lstay, lsw, linit = s.hmm_tables()
    half = s.width // 2
    i = np.arange(nb)[:, None]
    j = np.arange(nb)[None, :]
    dd = j - i + half
    ok = (dd >= 0) & (dd < s.width)
    LT = np.where(ok, ltri[np.clip(dd, 0, s.width - 1)], -np.inf)     # [i, j]
    lo = np.log(obs + TINY)
    val = linit + lo[0]
    bp = np.zeros((T, S), dtype=np.int64)
    ar = np.arange(nb)
    for t in range(1, T):
        M = np.empty((2, nb))
        arg = np.empty((2, nb), dtype=np.int64)
        for v in range(2):
            a = val[v * nb:(v + 1) * nb] - lrow
            cand = a[:, None] + LT
            arg[v] = np.argmax(cand, axis=0)                           # the first (lowest i) maximum
            M[v] = cand[arg[v], ar]
        new = np.empty(S)
        for vp_ in range(2):
            c0 = M[0] + (lstay if vp_ == 0 else lsw)
            c1 = M[1] + (lsw if vp_ == 0 else lstay)
            take1 = c1 > c0
            best = np.where(take1, c1, c0)
            bp[t, vp_ * nb:(vp_ + 1) * nb] = np.where(take1, nb + arg[1], arg[0])
            new[vp_ * nb:(vp_ + 1) * nb] = best + lo[t, vp_ * nb:(vp_ + 1) * nb]
        val = new
    states = np.empty(T, dtype=np.int64)
    states[T - 1] = int(np.argmax(val))
    for t in range(T - 1, 0, -1):
        states[t - 1] = bp[t, states[t]]
    return states


def decode(states, s):
    """states [T] -> (f0 fp32 with NaN, voiced_flag uint8, bin int64)"""
    nb = s.n_pitch_bins
    b = states % nb
    voiced = states < nb
    f0 = (s.fmin * 2.0 ** (b / (12.0 * s.nbps))).astype(np.float32)
    f0[~voiced] = np.nan
    return f0, voiced.astype(np.uint8), b


def pyin(y, fmin, fmax, dprime_dtype=None, **kw):
    """one waveform -> dict(f0, voiced_flag, voiced_prob, bin, dprime, obs); dprime_dtype=np.float32 rounds d' to fp32 before
    the observation stage (the precision-sensitivity run)"""
    s = Setting(fmin, fmax, **kw)
    dp = cmnd(y, s)
    if dprime_dtype is not None:
        dp = dp.astype(dprime_dtype)
    obs, vp = observe(dp, s)
    st = viterbi(obs, s)
    f0, vf, b = decode(st, s)
    return dict(f0=f0, voiced_flag=vf, voiced_prob=vp.astype(np.float32), bin=b, dprime=dp, obs=obs, setting=s)


# ---- the test signals shared by tests/test_pitch_cpu.py and tests/test_pitch_gpu.py ---------------------------------------

def harmonic_tone(f0, dur=2.0, sr=16000, partials=6):
    t = np.arange(int(dur * sr)) / sr
    y = sum(np.sin(2 * np.pi * h * f0 * t) / h for h in range(1, partials + 1))
    return (0.3 * y).astype(np.float32)


def glide(f_a=120.0, f_b=240.0, dur=2.0, sr=16000, partials=6):
    t = np.arange(int(dur * sr)) / sr
    f = f_a + (f_b - f_a) * t / dur
    ph = 2 * np.pi * np.cumsum(f) / sr
    y = sum(np.sin(h * ph) / h for h in range(1, partials + 1))
    return (0.3 * y).astype(np.float32), f


def white_noise(seed, dur=1.0, sr=16000, level=0.1):
    return (level * np.random.default_rng(seed).standard_normal(int(dur * sr))).astype(np.float32)


def speech_like(seed, dur=1.5, sr=16000, snr_db=20.0, partials=8):
    """harmonic source with a slowly varying f0 in 100..300 Hz, voiced / silent segments, white noise at `snr_db`"""
    rng = np.random.default_rng(seed)
    n = int(dur * sr)
    t = np.arange(n) / sr
    f = 180.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.6 * rng.random()) * t + 2 * np.pi * rng.random()) \
        + 25.0 * np.sin(2 * np.pi * (2.0 + rng.random()) * t + 2 * np.pi * rng.random())
    ph = 2 * np.pi * np.cumsum(f) / sr
    amp = rng.random(partials) + 0.2
    y = sum(amp[h - 1] * np.sin(h * ph) / h for h in range(1, partials + 1))
    gate = (np.sin(2 * np.pi * 1.3 * t + 2 * np.pi * rng.random()) > -0.6).astype(np.float64)
    k = np.hanning(321)
    gate = np.convolve(gate, k / k.sum(), mode="same")
    y = 0.25 * y * gate
    p_sig = np.mean(y ** 2)
    noise = rng.standard_normal(n) * np.sqrt(p_sig / 10 ** (snr_db / 10))
    return (y + noise).astype(np.float32), f


def interior_frames(L, s):
    """indices of frames whose whole frame_length window lies inside the signal"""
    T = s.n_frames(L)
    t = np.arange(T)
    start = t * s.hop_length - s.frame_length // 2
    return t[(start >= 0) & (start + s.frame_length <= L)]


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, dtype=np.float64) / np.asarray(ref, dtype=np.float64))
