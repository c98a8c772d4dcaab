"""Small numpy / torch oracle of the inpainting validator (nppc_audio/inpainting/validator/validator_nppc_model.py of the
reference), restated so that every stage can be run in float64, or in float32 exactly as the reference runs it.

istft             torch.istft as the reference calls it (validator_nppc_model.py:563-567, :615-619: n_fft, hop_length,
                  win_length = n_fft, periodic hann window, center=True), written out: inverse real DFT of every frame,
                  window, overlap-add, division by the window envelope, centre cut
pc_variation_chain  save_pc_audio_variations' arithmetic (:553-561 clean path, :602-619 variations) with torch.istft
metric_rows / gram  the rows behind compute_metrics (:742-828): directions, pred - clean (:813), the gap-only errors of
                  compute_rmse (:758-762)
"""
import numpy as np
import torch


def natural_length(n_fft, hop, T):
    """torch.istft(center=True, length=None): n_fft + hop (T - 1) samples of overlap-add minus n_fft // 2 at each end"""
    return n_fft + hop * (T - 1) - 2 * (n_fft // 2)


def istft(re, im, n_fft, hop, length=None):
    """float64 inverse STFT of [B, F, T] planes (numpy).  The inverse real DFT ignores the imaginary part of bin 0 and,
    for even n_fft, of the Nyquist bin, which counts once (torch.fft.irfft's convention)."""
    re, im = np.asarray(re, np.float64), np.asarray(im, np.float64)
    B, F, T = re.shape
    assert F == n_fft // 2 + 1
    n = np.arange(n_fft)
    k = np.arange(F)
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft) / n_fft           # [F, N], phases reduced exactly
    wgt = np.full(F, 2.0)
    wgt[0] = 1.0
    if n_fft % 2 == 0:
        wgt[-1] = 1.0
    C = wgt[:, None] * np.cos(ang) / n_fft
    S = -wgt[:, None] * np.sin(ang) / n_fft
    S[0] = 0.0
    if n_fft % 2 == 0:
        S[-1] = 0.0
    frames = np.einsum("bft,fn->btn", re, C) + np.einsum("bft,fn->btn", im, S)  # [B, T, N]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    full = n_fft + hop * (T - 1)
    y = np.zeros((B, full))
    env = np.zeros(full)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += frames[:, t] * win
        env[t * hop:t * hop + n_fft] += win ** 2
    start = n_fft // 2
    end = start + length if length is not None else full - n_fft // 2
    kept_end = min(end, full)
    if env[start:kept_end].min() < 1e-11:
        raise ValueError("window overlap add min < 1e-11")
    out = np.zeros((B, end - start))
    out[:, :kept_end - start] = y[:, start:kept_end] / env[start:kept_end]
    return out


def torch_istft(re, im, n_fft, hop, length=None, dtype=torch.float64):
    """the reference's own call (:563-567), on the CPU in `dtype`"""
    re, im = torch.as_tensor(re).to(dtype), torch.as_tensor(im).to(dtype)
    window = torch.hann_window(n_fft, dtype=dtype)
    return torch.istft(torch.complex(re, im), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window, length=length)


def pc_variation_chain(clean_norm, pred, pc, clean_spec, alphas, mean, std, n_fft, hop, dtype):
    """save_pc_audio_variations :553-561 and :602-619 for a batch, every operation in `dtype` on the CPU:
    -> (variations [B, K, A, L], clean_audio [B, L])"""
    cast = lambda t: torch.as_tensor(t).to(dtype)
    clean_norm, pred, pc, clean_spec, alphas = (cast(t) for t in (clean_norm, pred, pc, clean_spec, alphas))
    mean, std = cast(mean), cast(std)
    window = torch.hann_window(n_fft, dtype=dtype)
    inv = lambda z: torch.istft(z, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window)
    B, K = pc.shape[:2]
    outs, cleans = [], []
    for b in range(B):
        clean_phase = torch.angle(torch.complex(clean_spec[b, 0], clean_spec[b, 1]))                      # :553-554
        clean_mag_linear = torch.exp(clean_norm[b, 0] * std + mean) - 1e-6                                # :557-558
        cleans.append(inv(torch.complex(clean_mag_linear * torch.cos(clean_phase), clean_mag_linear * torch.sin(clean_phase))))
        per_k = []
        for i in range(K):
            per_a = []
            for alpha in alphas:
                modified_mag = pred[b, 0] + alpha * pc[b, i]                                              # :608
                modified_mag_linear = torch.exp(modified_mag * std + mean)                                # :609-610
                per_a.append(inv(torch.complex(modified_mag_linear * torch.cos(clean_phase),
                                               modified_mag_linear * torch.sin(clean_phase))))            # :611-619
            per_k.append(torch.stack(per_a))
        outs.append(torch.stack(per_k))
    return torch.stack(outs), torch.stack(cleans)


def metric_rows(nppc, mc, pred, mean, clean, mask):
    """[2n + 3, N] float64 rows of one item: directions as stored, the fp32 differences widened (the device forms them
    in fp32 as well): pred - clean (:813), (pred - clean)[mask == 0] and (mean - clean)[mask == 0] (:758-762)"""
    f = lambda t: np.asarray(t, np.float32).reshape(-1)
    n = np.asarray(nppc).shape[1]
    hole = (f(mask) == 0).astype(np.float32)
    e = f(pred) - f(clean)
    rows = [np.asarray(nppc, np.float32).reshape(n, -1), np.asarray(mc, np.float32).reshape(n, -1),
            e[None], (e * hole)[None], ((f(mean) - f(clean)) * hole)[None]]
    return np.concatenate(rows).astype(np.float64)


def gram(rows):
    return rows @ rows.T
