"""Restatement of gap-constrained Griffin-Lim with torch.stft / torch.istft on the CPU over the WHOLE
signal, no locality tricks: the yardstick of tests/test_gl_gap_cpu.py and tests/test_gl_gap_gpu.py.  Parametrised by dtype:
float64 is the specification, float32 is the error yardstick ("a kernel may be twice as far from fp64 as this code in fp32").

Agreement with torchaudio's or librosa's Griffin-Lim is unverified: neither is available to this project.  With momentum 0
and no gap restriction the loop below is the textbook algorithm; the momentum form is torchaudio's as published
(tprev kept, angles = rebuilt - momentum / (1 + momentum) * tprev, normalised by abs + 1e-16)."""
import math

import numpy as np
import torch

# (n_fft, hop, T, [gap frame ranges, inclusive]) -- the cases of the issue
CASES = [
    (255, 128, 40, [(12, 28)]),
    (255, 128, 40, [(0, 5)]),
    (255, 128, 40, [(34, 39)]),
    (255, 128, 40, [(7, 7)]),
    (255, 128, 40, [(5, 8), (20, 24)]),
    (512, 256, 24, [(8, 13)]),
    (510, 256, 24, [(8, 13)]),
    (64, 16, 48, [(20, 30)]),
    (64, 16, 48, [(0, 6)]),
    (64, 16, 48, [(41, 47)]),
]


# Inputs of the monotonicity checks.  `d` as the contract defines it is NOT guaranteed to be non-increasing, for any gap
# position.  stft(istft(.)) is the orthogonal projection on the consistent spectrograms in the norm of the full, two-sided
# spectrum, in which bins 1 .. ceil(n_fft / 2) - 1 count twice; d sums the one-sided n_fft / 2 + 1 bins unweighted.  Measured
# with this fp64 code (make_case seeds 0 .. 3, B = 3, V = 3, 16 steps, mu = 0; largest d[n+1] / d[n] - 1, fp32 alike):
#   (64, 16, 48, gap 20..30)  seed 0  +1.09e-3      an interior gap, the largest step of all
#   (64, 16, 48, gap 0..6)    seed 0  +8.9e-5,  seed 2  +1.65e-4
#   every other case and seed: no step above 0; seeds 1 and 3: none in any case.
# With the bins weighted 1, 2, .., 2, (1) the same runs show no step above 0 in any case or seed, clip-edge gaps included,
# so the weighting accounts for everything measured here; whether reflect padding at a clip edge can break the decrease on
# its own is not settled by these runs.  The monotonicity tests use seed 1, on which the restatement itself meets
# (1 + 1e-9) at all ten shapes, and assert that before they look at the device.
MONOTONE_SEED = 1


def case_id(c):
    return f"{c[0]}-{c[1]}-T{c[2]}-" + "+".join(f"{a}..{b}" for a, b in c[3])


def natural_length(n_fft, hop, T):
    return hop * (T - 1) + (n_fft & 1)


def signal(L, seed, sr=16000.0):
    """harmonic glide plus noise, float64 [L], peak below 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    f0 = 110.0 + 40.0 * rng.random() + (60.0 + 30.0 * rng.random()) * t / max(t[-1], 1e-9)
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(L)
    for h in range(1, 9):
        x += rng.random() / h * np.sin(h * ph + 2.0 * np.pi * rng.random())
    x += 0.05 * rng.standard_normal(L)
    return 0.5 * x / np.abs(x).max()


def frame_mask(T, ranges):
    m = torch.ones(T)
    for a, b in ranges:
        m[a:b + 1] = 0
    return m


def stft(x, n_fft, hop):
    w = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    return torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", return_complex=True)


def istft(C, n_fft, hop, L):
    w = torch.hann_window(n_fft, periodic=True, dtype=C.real.dtype)
    return torch.istft(C, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=L)


def neighbours(mask, r):
    """known frames within r frames of a gap frame"""
    gap = (mask == 0).numpy()
    T = len(gap)
    nb = np.zeros(T, bool)
    for t in range(T):
        if not gap[t]:
            nb[t] = gap[max(0, t - r):t + r + 1].any()
    return torch.from_numpy(nb)


def griffin_lim_gap(M, Kn, mask, phi0, n_iter, mu=0.0, n_fft=255, hop=128, L=None, dtype=torch.float64):
    """one waveform: M [F,T] magnitudes, Kn [F,T] complex, mask [T] (1 = known), phi0 [F,T]  ->  (x [L], d [n_iter],
    target_norm), all in `dtype` arithmetic"""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    F, T = M.shape
    L = natural_length(n_fft, hop, T) if L is None else L
    assert 1 + L // hop == T and F == n_fft // 2 + 1
    gap = (mask == 0)[None, :].expand(F, T)
    r = -(-n_fft // hop) - 1
    nb = neighbours(mask, r)[None, :].expand(F, T)
    M = torch.where(gap, M.to(dtype), torch.zeros((), dtype=dtype))
    Kn = torch.where(gap, torch.zeros((), dtype=cd), Kn.to(cd))
    phi0 = torch.where(gap, phi0.to(dtype), torch.zeros((), dtype=dtype))
    tnorm = float(torch.sqrt((M.double() ** 2).sum()))
    if not bool(gap.any()):
        return istft(Kn, n_fft, hop, L), torch.zeros(n_iter, dtype=dtype), 0.0
    C = torch.where(gap, torch.polar(M, phi0), Kn)
    Pp = torch.zeros_like(C)
    d = []
    for _ in range(n_iter):
        x = istft(C, n_fft, hop, L)
        R = stft(x, n_fft, hop)
        dg = ((R.abs() - M) ** 2)[gap].sum()
        dk = ((R - Kn).abs() ** 2)[nb].sum()
        d.append(torch.sqrt(dg + dk))
        A = R - (mu / (1.0 + mu)) * Pp
        A = A / (A.abs() + 1e-16)
        Pp = R
        C = torch.where(gap, M * A, Kn)
    return istft(C, n_fft, hop, L), (torch.stack(d) if d else torch.zeros(0, dtype=dtype)), tnorm


def phase_advance_init(Kn, mask, n_fft, hop):
    """Kn [F,T] complex, mask [T] -> phi0 [F,T] float64 (0 on known frames)"""
    F, T = Kn.shape
    gap = (mask == 0).numpy()
    out = torch.zeros(F, T, dtype=torch.float64)
    f = torch.arange(F, dtype=torch.float64)
    for t in range(T):
        if not gap[t]:
            continue
        t0 = t - 1
        while t0 >= 0 and gap[t0]:
            t0 -= 1
        if t0 < 0:
            t0 = t + 1
            while t0 < T and gap[t0]:
                t0 += 1
        if t0 >= T:
            continue
        out[:, t] = torch.angle(Kn[:, t0].to(torch.complex128)) + 2.0 * math.pi * f * hop * (t - t0) / n_fft
    return out


def reach(mask, n_fft, hop, L):
    """bool [L]: samples that a gap frame's window covers"""
    pad = n_fft // 2
    out = np.zeros(L, bool)
    for t in np.nonzero((mask == 0).numpy())[0]:
        out[max(0, t * hop - pad):max(0, min(L, t * hop + n_fft - pad))] = True
    return out


def make_case(case, B=3, V=3, seed=0, perturb=0.2):
    """inputs of one test case as float32 torch tensors (what the device sees) plus the clean signal:
    item b has the case's gap shifted right by b frames, so every item has a different gap; a gap at a clip edge keeps
    the edge and is b frames longer."""
    n_fft, hop, T, ranges = case
    L = natural_length(n_fft, hop, T)
    F = n_fft // 2 + 1
    rng = np.random.default_rng(1000 + seed)
    clean, spec, masks = [], [], []
    for b in range(B):
        x = torch.from_numpy(signal(L, 17 * seed + b)).float()
        clean.append(x)
        spec.append(stft(x.double(), n_fft, hop))
        rs = []
        for a, e in ranges:
            if a == 0:
                rs.append((0, e + b))
            elif e == T - 1:
                rs.append((a - b, e))
            else:
                rs.append((a + b, e + b))
        masks.append(frame_mask(T, rs))
    clean = torch.stack(clean)
    spec = torch.stack(spec)                                                   # [B,F,T] complex128
    mask = torch.stack(masks)                                                  # [B,T]
    known = torch.stack([spec.real, spec.imag], 1).float() * mask[:, None, None, :]
    mag = spec.abs()[:, None].expand(B, V, F, T)
    tm = (mag * (1.0 + perturb * torch.from_numpy(rng.uniform(-1, 1, (B, V, F, T))))).float()
    phase = torch.from_numpy(rng.uniform(-math.pi, math.pi, (B, V, F, T))).float()
    return {"n_fft": n_fft, "hop": hop, "T": T, "L": L, "F": F, "clean": clean, "spec": spec, "mask": mask, "known": known,
            "target_mag": tm.contiguous(), "init_phase": phase.contiguous()}


def run_case(z, n_iter, mu, dtype, target_mag=None, init_phase=None):
    """the restatement on every (item, variation) of make_case's dict -> (waves [B,V,L], d [B,V,n_iter], tnorm [B,V]) float64"""
    tm = z["target_mag"] if target_mag is None else target_mag
    ph = z["init_phase"] if init_phase is None else init_phase
    B, V = tm.shape[:2]
    Kn = torch.complex(z["known"][:, 0].double(), z["known"][:, 1].double())
    W = torch.zeros(B, V, z["L"], dtype=torch.float64)
    D = torch.zeros(B, V, n_iter, dtype=torch.float64)
    N = torch.zeros(B, V, dtype=torch.float64)
    for b in range(B):
        for v in range(V):
            x, d, tn = griffin_lim_gap(tm[b, v], Kn[b], z["mask"][b], ph[b, v] if ph.dim() == 4 else ph[b], n_iter, mu,
                                       z["n_fft"], z["hop"], z["L"], dtype)
            W[b, v], D[b, v], N[b, v] = x.double(), d.double(), tn
    return W, D, N


def rel_l2(a, b):
    return float(torch.linalg.norm((a.double() - b.double()).reshape(-1)) / torch.linalg.norm(b.double().reshape(-1)))
