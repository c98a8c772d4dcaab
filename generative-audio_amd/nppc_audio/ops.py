"""Thin host wrappers over the element-wise / front-end entry points of libnppc_hip.so.

Each function validates shapes the way the reference call site would fail, allocates the outputs
with torch (device memory plumbing only) and enqueues the HIP kernel on the current stream.
"""
import torch

from . import _hip as H

EPS32 = float(torch.finfo(torch.float32).eps)   # audio_zen/constant.py:8


def _f32c(x):
    H.require_gpu()
    if not x.is_cuda:
        raise RuntimeError("NPPC-audio HIP ops take device tensors")
    return x.contiguous().float()


def stft_frames(lengths, hop):
    """frame count of the centred STFT of `lengths` samples: 1 + L // hop (int, list or tensor, elementwise)"""
    if isinstance(lengths, torch.Tensor):
        return 1 + torch.div(lengths, hop, rounding_mode="floor")
    if isinstance(lengths, (list, tuple)):
        return [1 + int(n) // hop for n in lengths]
    return 1 + int(lengths) // hop


def ragged_lengths(lengths, B, Lmax, min_len, device):
    """(device int32 [B], host list) of a ragged batch's per-item lengths, checked on the host: 0 < min_len < L_b <= Lmax.
    A device tensor is read back once for the check."""
    host = torch.as_tensor(lengths).reshape(-1).tolist() if isinstance(lengths, torch.Tensor) else [int(n) for n in lengths]
    if len(host) != B:
        raise ValueError(f"lengths has {len(host)} entries for a batch of {B}")
    for b, n in enumerate(host):
        if n != int(n) or n > Lmax:
            raise ValueError(f"item {b}: length {n} exceeds the padded length {Lmax}")
        if n <= min_len:
            raise ValueError(f"item {b}: length {n} is too short (needs more than {min_len} samples)")
    return torch.tensor(host, dtype=torch.int32).to(device), [int(n) for n in host]


def stft(wave, nfft, hop, want_mag=True, lengths=None):
    """utils.py:107-147 / trainer.py:349-355: centred, periodic-hann, onesided STFT.
    wave [B,L] -> (mag|None, real, imag) each [B,F,T].

    lengths [B] (ragged batch, wave zero- or otherwise padded to L): item b is the STFT of its first L_b samples alone
    (reflect padding at its own end) in frames t < 1 + L_b // hop; later frames are 0 and samples past L_b are not read."""
    wave = _f32c(wave)
    if wave.dim() == 1:
        wave = wave[None]
    B, L = wave.shape
    F, T = nfft // 2 + 1, 1 + L // hop
    re = torch.empty(B, F, T, dtype=torch.float32, device=wave.device)
    im = torch.empty_like(re)
    mag = torch.empty_like(re) if want_mag else None
    if lengths is not None:
        dl, _ = ragged_lengths(lengths, B, L, nfft // 2, wave.device)
        H.call("nppc_stft_ragged", wave, L, dl, re, im, mag, B, T, nfft, hop, H.stream())
        return mag, re, im
    H.call("nppc_stft", wave, re, im, mag, B, L, nfft, hop, H.stream())
    return mag, re, im


def drop_band(x, num_groups=2):
    """audio_zen/acoustics/feature.py:254-285 on [B,C,F,T]."""
    B, C, F, T = x.shape
    assert B > num_groups, f"Batch size = {B}, num_groups = {num_groups}. The batch size should larger than the num_groups."
    if num_groups <= 1:
        return x
    x = _f32c(x)
    Fo = (F - F % num_groups) // num_groups
    out = torch.empty(B, C, Fo, T, dtype=torch.float32, device=x.device)
    H.call("nppc_dropband", x, out, B, C, F, T, num_groups, H.stream())
    return out


def cirm_build_compress(n_re, n_im, c_re, c_im, num_groups=1):
    """mask.py:24-54 + trainer.py:359-362: compressed cIRM in [B,2,F',T], drop-band applied."""
    n_re, n_im, c_re, c_im = (_f32c(t) for t in (n_re, n_im, c_re, c_im))
    B, F, T = n_re.shape
    assert B > num_groups, f"Batch size = {B}, num_groups = {num_groups}. The batch size should larger than the num_groups."
    Fo = F if num_groups <= 1 else (F - F % num_groups) // num_groups
    out = torch.empty(B, 2, Fo, T, dtype=torch.float32, device=n_re.device)
    H.call("nppc_cirm_build_compress", n_re, n_im, c_re, c_im, out, B, F, T, num_groups, EPS32, H.stream())
    return out


def cirm_build_compress_ragged(n_re, n_im, c_re, c_im, frames):
    """cirm_build_compress of a ragged batch, no drop-band: [B,F,T] x4 + device int32 frames [B] -> [B,2,F,T]; item b is
    built on its frames t < T_b and is 0 from T_b on (the inputs are not read there)."""
    n_re, n_im, c_re, c_im = (_f32c(t) for t in (n_re, n_im, c_re, c_im))
    B, F, T = n_re.shape
    frames = frames.to(device=n_re.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, 2, F, T, dtype=torch.float32, device=n_re.device)
    H.call("nppc_cirm_build_compress_ragged", n_re, n_im, c_re, c_im, out, frames, B, F, T, EPS32, H.stream())
    return out


def cirm_decompress_apply_conj(crm, n_re, n_im, want_dec=False):
    """mask.py:57-60 then utils.py:241-249 (-> :75-79 with real/imag swapped = conj(mask)*noisy).
    crm [B,2,F,T] compressed; n_re/n_im [B,F,T] -> (dec [B,F,T,2]|None, enh_mag, enh_real, enh_imag)."""
    crm, n_re, n_im = _f32c(crm), _f32c(n_re), _f32c(n_im)
    B, _, F, T = crm.shape
    emag = torch.empty(B, F, T, dtype=torch.float32, device=crm.device)
    ere, eim = torch.empty_like(emag), torch.empty_like(emag)
    dec = torch.empty(B, F, T, 2, dtype=torch.float32, device=crm.device) if want_dec else None
    H.call("nppc_cirm_decompress_apply_conj", crm, n_re, n_im, dec, emag, ere, eim, B, F, T, H.stream())
    return dec, emag, ere, eim


def cirm_decompress_apply(crm, n_re, n_im):
    """decompress_cIRM + TRUE complex product mask*noisy (utils.py:37-58: model_outputs_to_waveforms' mask application).
    crm [B,2,F,T] compressed -> (enh_mag, enh_real, enh_imag) [B,F,T]."""
    crm, n_re, n_im = _f32c(crm), _f32c(n_re), _f32c(n_im)
    B, _, F, T = crm.shape
    emag = torch.empty(B, F, T, dtype=torch.float32, device=crm.device)
    ere, eim = torch.empty_like(emag), torch.empty_like(emag)
    H.call("nppc_cirm_decompress_apply", crm, n_re, n_im, None, emag, ere, eim, B, F, T, H.stream())
    return emag, ere, eim


def istft_natural_length(nfft, hop, T):
    """samples torch.istft(center=True) returns with length=None: hop (T - 1), plus 1 for odd n_fft"""
    return hop * (T - 1) + (nfft & 1)


def istft_envelope_min(nfft, hop, T, length):
    """smallest window envelope sum_t hann^2 inside the samples torch.istft keeps (it raises below 1e-11); host numpy"""
    import numpy as np
    w2 = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)) ** 2
    env = np.zeros(nfft + hop * (T - 1))
    for t in range(T):
        env[t * hop:t * hop + nfft] += w2
    kept = env[nfft // 2:nfft // 2 + length]
    return float(kept.min()) if kept.size else 0.0


def _istft_fft_kernel_takes(nfft, hop):
    return nfft in (64, 128, 256, 512) and hop > 0 and nfft % hop == 0 and nfft // hop <= 8


def istft_any(re, im, nfft, hop, length=None, out=None):
    """torch.istft(n_fft, hop, win_length=n_fft, hann window, center=True, length=length) for any n_fft <= 512,
    1 <= hop <= n_fft, ceil(n_fft / hop) <= 8 (the inpainting configuration is 255 / 128): [B,F,T] x2 -> [B,length].
    length=None: torch's default, hop (T - 1) (+ 1 for odd n_fft); a longer length zero-fills the tail as torch does.
    out: optional [B, >= length] fp32 device tensor to write into (nothing past `length` is written).
    ValueError where torch raises: the window envelope inside the kept range is below 1e-11."""
    re, im = _f32c(re), _f32c(im)
    B, F, T = re.shape
    if F != nfft // 2 + 1 or im.shape != re.shape:
        raise ValueError(f"istft: planes {tuple(re.shape)} / {tuple(im.shape)} do not fit n_fft {nfft}")
    length = check_istft_any_config(nfft, hop, T, length)
    if out is None:
        out = torch.empty(B, length, dtype=torch.float32, device=re.device)
    assert out.dim() == 2 and out.shape[0] == B and out.shape[1] >= length and out.dtype == torch.float32
    with envelope_refusal(nfft, hop, T, length):
        H.call("nppc_istft_any", re, im, F * T, out, out.shape[1], B, T, nfft, hop, length, H.stream())
    return out


def check_istft_any_config(nfft, hop, T, length):
    """the shape rules of nppc_istft_any as ValueErrors; -> the length to produce (torch's default for None)"""
    if nfft < 2 or nfft > 512 or not (1 <= hop <= nfft) or -(-nfft // hop) > 8:
        raise ValueError(f"istft: n_fft {nfft} / hop {hop} outside 2 <= n_fft <= 512, 1 <= hop <= n_fft, ceil(n_fft / hop) <= 8")
    length = istft_natural_length(nfft, hop, T) if length is None else int(length)
    if T < 1 or length <= 0:
        raise ValueError(f"istft: {T} frame(s) of n_fft {nfft} / hop {hop} give no samples")
    return length


class envelope_refusal:
    """Around a launch whose other arguments were checked already: the entry point's one remaining NPPC_EBADARG is the
    window envelope (computed once, in C, before the launch), reported as the ValueError torch.istft would raise."""

    def __init__(self, nfft, hop, T, length):
        self.args = (nfft, hop, T, length)

    def __enter__(self):
        return self

    def __exit__(self, kind, err, tb):
        if kind is RuntimeError and "bad argument" in str(err):
            nfft, hop, T, length = self.args
            low = istft_envelope_min(nfft, hop, T, length)
            if low >= 1e-11:
                return False
            raise ValueError(f"istft: window overlap add min {low:.3g} < 1e-11 for n_fft {nfft}, hop {hop}, {T} frames "
                             "(torch.istft raises here too)") from err
        return False


def istft(re, im, nfft, hop, length=None, lengths=None):
    """torch.istft(n_fft, hop, win_length=n_fft, hann window, center=True, length=length): [B,F,T] x2 -> [B,length]
    (utils.py:60-70, nppc_audio/validator.py:136-143).  Power-of-two n_fft with n_fft % hop == 0 runs the radix-2 kernel;
    every other configuration (any n_fft <= 512, see istft_any) the direct inverse DFT.  length=None: torch's default.

    lengths [B] (ragged batch, L_b <= length, 1 + L_b // hop <= T): item b is torch.istft(length=L_b) of its first
    1 + L_b // hop frames alone; samples L_b .. length-1 are 0."""
    if lengths is None and not _istft_fft_kernel_takes(nfft, hop):
        return istft_any(re, im, nfft, hop, length)
    re, im = _f32c(re), _f32c(im)
    B, F, T = re.shape
    assert F == nfft // 2 + 1
    if length is None:
        length = istft_natural_length(nfft, hop, T)
    out = torch.empty(B, length, dtype=torch.float32, device=re.device)
    if lengths is not None:
        dl, host = ragged_lengths(lengths, B, length, 0, re.device)
        for b, n in enumerate(host):
            if stft_frames(n, hop) > T:
                raise ValueError(f"item {b}: length {n} needs {stft_frames(n, hop)} frames, the input has {T}")
        H.call("nppc_istft_ragged", re, im, out, length, dl, B, T, nfft, hop, H.stream())
        return out
    H.call("nppc_istft", re, im, out, B, T, nfft, hop, length, H.stream())
    return out


def model_outputs_to_waveforms(enhanced_masks, noisy_reals, noisy_imags, orig_length, nfft=512, hop=256, lengths=None):
    """utils.py:37-72: compressed cIRM [B,2,F,T] + noisy STFT [B,1,F,T] -> enhanced waveforms [B, orig_length].
    lengths [B]: a ragged batch (istft's `lengths`); samples past an item's length are 0."""
    _, ere, eim = cirm_decompress_apply(enhanced_masks, noisy_reals.squeeze(1), noisy_imags.squeeze(1))
    return istft(ere, eim, nfft, hop, orig_length, lengths=lengths)


def crm_mse_ragged(n_re, n_im, c_re, c_im, crm, frames):
    """per-item cIRM MSE of a ragged batch (no drop-band): [B,F,T] x4 + compressed cIRM [B,2,F,T] + device int32 frames [B]
    -> fp64 [B], item b averaged over its 2 x F x T_b elements (the target of cirm_build_compress)."""
    n_re, n_im, c_re, c_im, crm = (_f32c(t) for t in (n_re, n_im, c_re, c_im, crm))
    B, F, T = n_re.shape
    assert crm.shape == (B, 2, F, T), "the ragged forward keeps all F bins"
    frames = frames.to(device=n_re.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, dtype=torch.float64, device=n_re.device)
    H.call("nppc_crm_mse_ragged", n_re, n_im, c_re, c_im, crm, frames, B, F, T, EPS32, out, H.stream())
    return out


def crm_directions_to_spectrograms(w_mat, noisy_re, noisy_im):
    """NPPCAudioValidator._crm_directions_to_spectograms (nppc_audio/validator.py:55-102): every PC direction
    w_mat[:, k] (compressed cIRM [B,2,F,T]) is decompressed and applied to the noisy STFT with the TRUE complex product
    (utils.crm_to_spectogram, utils.py:252-256).  w_mat [B,K,2,F,T], noisy_re/im [B,F,T] -> (real, imag) [B,K,F,T]."""
    B, K, _, F, T = w_mat.shape
    re = torch.empty(B, K, F, T, dtype=torch.float32, device=w_mat.device)
    im = torch.empty_like(re)
    for k in range(K):
        _, r, i = cirm_decompress_apply(w_mat[:, k], noisy_re, noisy_im)
        re[:, k], im[:, k] = r, i
    return re, im


def pc_direction_waveforms(pred_crm, w_mat, alphas, noisy_re, noisy_im, length, nfft=512, hop=256):
    """PC synthesis of the validator (nppc_audio/validator.py:148-302): waveforms of `enhanced + alpha * PC_k` for every
    direction k and every alpha, all (K * len(alphas) + 1) inverse STFTs as ONE batched overlap-add launch.
    pred_crm [B,2,F,T] (compressed), w_mat [B,K,2,F,T], alphas: sequence of floats -> (enhanced [B,length],
    variants [B,K,len(alphas),length])."""
    B, K = w_mat.shape[:2]
    _, e_re, e_im = cirm_decompress_apply(pred_crm, noisy_re, noisy_im)
    d_re, d_im = crm_directions_to_spectrograms(w_mat, noisy_re, noisy_im)
    a = torch.as_tensor(list(alphas), dtype=torch.float32, device=w_mat.device)
    A = a.numel()
    v_re = (e_re[:, None, None] + a[None, None, :, None, None] * d_re[:, :, None]).reshape(B * K * A, *e_re.shape[1:])
    v_im = (e_im[:, None, None] + a[None, None, :, None, None] * d_im[:, :, None]).reshape(B * K * A, *e_im.shape[1:])
    waves = istft(torch.cat((e_re, v_re)), torch.cat((e_im, v_im)), nfft, hop, length)
    return waves[:B], waves[B:].view(B, K, A, length)
