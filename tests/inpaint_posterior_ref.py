"""Restatement of the posterior samples of inpainted gaps (csrc/inpaint_posterior.hip) with torch on
the CPU, on top of tests/inpaint_validator_ref.py (clean phase) and tests/gl_gap_ref.py (Griffin-Lim).  Parametrised by
dtype: float64 is the specification, float32 the error yardstick.

The rule, sample s of item b, k ascending:
    x = pred[b];  for k: x = x + z[b, s, k] * pc[b, k];  mag = exp(x * std + mean)
"""
import torch

import gl_gap_ref as GR
import inpaint_validator_ref as VR


def sample_log_mag(pred, pc, z, dtype):
    """pred [B,1,F,T], pc [B,K,F,T], z [B,S,K] -> x [B,S,F,T] in `dtype`, the sum taken k ascending"""
    pred, pc, z = (torch.as_tensor(t).to(dtype) for t in (pred, pc, z))
    B, S, K = z.shape
    x = pred.expand(B, S, *pred.shape[2:]).clone()
    for k in range(K):
        x = x + z[:, :, k, None, None] * pc[:, k, None]
    return x


def sample_magnitudes(pred, pc, z, mean, std, dtype):
    """-> mag [B,S,F,T] = exp(x std + mean) in `dtype`"""
    mean, std = torch.as_tensor(mean).to(dtype), torch.as_tensor(std).to(dtype)
    return torch.exp(sample_log_mag(pred, pc, z, dtype) * std + mean)


def sample_waveforms(pred, pc, clean_spec, z, mean, std, n_fft, hop, dtype, length=None):
    """clean-phase samples [B,S,L]: the magnitudes on the phase of clean_spec [B,2,F,T] through torch.istft, every
    operation in `dtype` (the lines of inpaint_validator_ref.pc_variation_chain, with the sampled magnitude)"""
    mag = sample_magnitudes(pred, pc, z, mean, std, dtype)
    clean_spec = torch.as_tensor(clean_spec).to(dtype)
    window = torch.hann_window(n_fft, dtype=dtype)
    B, S = mag.shape[:2]
    out = []
    for b in range(B):
        clean_phase = torch.angle(torch.complex(clean_spec[b, 0], clean_spec[b, 1]))
        cs, sn = torch.cos(clean_phase), torch.sin(clean_phase)
        out.append(torch.stack([torch.istft(torch.complex(mag[b, s] * cs, mag[b, s] * sn), n_fft=n_fft, hop_length=hop,
                                            win_length=n_fft, window=window, length=length) for s in range(S)]))
    return torch.stack(out)


def one_hot_coefficients(B, K, alphas):
    """z [B, K A, K]: row k A + a is alphas[a] e_k"""
    alphas = torch.as_tensor(alphas, dtype=torch.float32).reshape(-1)
    A = alphas.numel()
    z = torch.zeros(K, A, K)
    for k in range(K):
        z[k, :, k] = alphas
    return z.reshape(1, K * A, K).expand(B, K * A, K).contiguous()


def sample_waveforms_blind(pred, pc, known, mask, z, mean, std, phi0, n_iter, mu, n_fft, hop, L, dtype):
    """Griffin-Lim samples: magnitudes by the rule in `dtype`, then gl_gap_ref.griffin_lim_gap; V = S + 1 with the
    prediction (z = 0) last.  known [B,2,F,T], mask [B,T], phi0 [B,F,T] -> (waves [B,S+1,L], d [B,S+1,n_iter], tnorm
    [B,S+1]) float64"""
    z = torch.as_tensor(z)
    B, S, K = z.shape
    zz = torch.cat([z.float(), torch.zeros(B, 1, K)], 1)
    mag = sample_magnitudes(pred, pc, zz, mean, std, dtype)
    Kn = torch.complex(known[:, 0].double(), known[:, 1].double())
    W = torch.zeros(B, S + 1, L, dtype=torch.float64)
    D = torch.zeros(B, S + 1, n_iter, dtype=torch.float64)
    N = torch.zeros(B, S + 1, dtype=torch.float64)
    for b in range(B):
        for v in range(S + 1):
            x, d, tn = GR.griffin_lim_gap(mag[b, v], Kn[b], mask[b], phi0[b], n_iter, mu, n_fft, hop, L, dtype)
            W[b, v], D[b, v], N[b, v] = x.double(), d.double(), tn
    return W, D, N


def stats(y):
    """fp64 mean and unbiased std over dim 1 of samples [B,S,...]"""
    y = y.double()
    return y.mean(1), y.std(1, unbiased=True)


def tiling(B, S, K, T, n_fft, hop, L, stats=0, no_stage=False):
    """the rule of nppc_inp_post_sample_shape -> (tiles, samples per tile, workspace bytes, staged, LDS bytes)"""
    TILE, FILL, MAX_TILES, LDS_STAGE = 8, 1024, 32, 65536
    F = n_fft // 2 + 1
    n = -(-S // TILE)
    if stats:
        fill = min(max(-(-FILL // (B * -(-L // 256))), 1), MAX_TILES)
        n = min(n, fill)
    per = -(-S // n)
    tiles = -(-S // per)
    work = 16 * tiles * B * ((L if stats & 1 else 0) + (F * T if stats & 2 else 0))
    nfr = (254 + n_fft) // hop + 1
    base = 16 * n_fft + 8 * nfr * F
    full = base + (16 + 4 * (K + 1)) * nfr * F
    staged = (not no_stage) and full <= LDS_STAGE
    return tiles, per, work, int(staged), full if staged else base
