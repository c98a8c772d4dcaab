"""Posterior samples from the NPPC directions (csrc/posterior.hip; specification tests/posterior_ref.py).

The net predicts a restoration and K directions whose norms are the predicted spread, i.e. the distribution
    m = pred_crm + sum_k z_k w_k,   z_k ~ N(0, 1)
in the compressed-cIRM domain where NPPCLoss is defined.  `sample_waveforms` turns coefficients z [B,S,K] into S waveforms
per item, and / or their statistics, in one fused launch (mask build, complex product, inverse STFT): no [B*S,F,T] plane is
ever materialised.  `PosteriorSampler` wraps it around a checkpoint.  The K-direction Gaussian is the model's statement of
the posterior, not the true one; metrics.nppc_direction_scores says how calibrated it is.
"""
import ctypes
from pathlib import Path
from typing import Literal, Optional

import pydantic
import torch

from . import _hip as H
from . import ops
from .nppc_model import NPPCModel, NPPCModelConfig

__all__ = ["draw_coefficients", "as_coefficients", "sample_tiling", "check_sample_args", "sample_waveforms",
           "PosteriorSamplerConfig", "PosteriorSampler", "MAX_K", "TILE", "MAX_STAT_S", "DOMAINS"]

MAX_K = 16               # NPPC_POST_MAX_K, the engine's cap on the directions
TILE = 8                 # NPPC_POST_TILE
MAX_STAT_S = 4096        # NPPC_POST_MAX_STAT_S
DOMAINS = {"compressed": 0, "decompressed": 1}


def draw_coefficients(B, S, K, seed=None, generator=None, complex_coeffs=False, temperature=1.0, device="cuda"):
    """z [B,S,K,2] fp32 for sample_waveforms: torch.randn on `device` (seeded by `seed`, or drawn from `generator`).
    Real by default (imaginary part 0), as the validator's alphas are: temperature * randn(B,S,K).  complex_coeffs=True:
    circular normals with E|z|^2 = temperature^2, i.e. temperature * randn(B,S,K,2) / sqrt(2)."""
    if B < 1 or S < 1 or K < 0:
        raise ValueError(f"draw_coefficients: B {B}, S {S}, K {K}")
    if seed is not None and generator is not None:
        raise ValueError("draw_coefficients: pass seed or generator, not both")
    device = torch.device(device)
    if seed is not None:
        generator = torch.Generator(device=device)
        generator.manual_seed(int(seed))
    if complex_coeffs:
        z = torch.randn(B, S, K, 2, generator=generator, device=device, dtype=torch.float32)
        return z * (float(temperature) * 0.5 ** 0.5)
    z = torch.zeros(B, S, K, 2, device=device, dtype=torch.float32)
    z[..., 0] = torch.randn(B, S, K, generator=generator, device=device, dtype=torch.float32) * float(temperature)
    return z


def as_coefficients(coeffs):
    """[B,S,K] real, [B,S,K] complex or [B,S,K,2] -> [B,S,K,2] fp32 contiguous (a real coefficient has imaginary part 0)"""
    if not isinstance(coeffs, torch.Tensor):
        raise ValueError("coeffs is a tensor [B,S,K] (real or complex) or [B,S,K,2]")
    if coeffs.is_complex():
        if coeffs.dim() != 3:
            raise ValueError(f"complex coeffs are [B,S,K], got {tuple(coeffs.shape)}")
        return torch.view_as_real(coeffs.to(torch.complex64)).contiguous()
    if coeffs.dim() == 3:
        return torch.stack((coeffs.float(), torch.zeros_like(coeffs, dtype=torch.float32)), dim=-1).contiguous()
    if coeffs.dim() == 4 and coeffs.shape[-1] == 2:
        return coeffs.float().contiguous()
    raise ValueError(f"coeffs are [B,S,K] or [B,S,K,2], got {tuple(coeffs.shape)}")


def config_ok(nfft, hop):
    return nfft in (64, 128, 256, 512) and hop > 0 and nfft % hop == 0 and nfft // hop <= 8


def sample_tiling(B, S, K, T, nfft, hop, length, stats=0):
    """(tiles, samples per tile, workspace bytes) of nppc_post_sample_shape; needs no GPU.  stats: bit 0 time, bit 1 spectrum"""
    tiles, per, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    try:
        H.call("nppc_post_sample_shape", B, S, K, T, nfft, hop, length, stats, ctypes.byref(tiles), ctypes.byref(per),
               ctypes.byref(nbytes))
    except RuntimeError as e:
        raise ValueError(f"posterior sampling: B {B}, S {S}, K {K}, T {T}, n_fft {nfft}, hop {hop}, length {length}: {e}") from e
    return tiles.value, per.value, nbytes.value


def check_sample_args(pred_shape, w_shape, re_shape, im_shape, z_shape, length, nfft, hop, lengths, domain, samples, stats,
                      spec_stats):
    """every refusal of sample_waveforms as a ValueError, from shapes alone (no GPU, no launch) -> (B, S, K, F, T, host lengths)"""
    if not config_ok(nfft, hop):
        raise ValueError(f"posterior sampling: n_fft {nfft} / hop {hop} outside n_fft in (64, 128, 256, 512), "
                         "n_fft % hop == 0, n_fft / hop <= 8")
    if domain not in DOMAINS:
        raise ValueError(f"domain must be one of {sorted(DOMAINS)}, got {domain!r}")
    if not (samples or stats or spec_stats):
        raise ValueError("posterior sampling: nothing asked for (samples, stats and spec_stats are all off)")
    F = nfft // 2 + 1
    if len(pred_shape) != 4 or pred_shape[1] != 2 or pred_shape[2] != F:
        raise ValueError(f"pred_crm is [B,2,{F},T], got {tuple(pred_shape)}")
    B, _, _, T = pred_shape
    if len(w_shape) != 5 or tuple(w_shape[:1]) + tuple(w_shape[2:]) != (B, 2, F, T):
        raise ValueError(f"w_mat is [B,K,2,F,T] = [{B},K,2,{F},{T}], got {tuple(w_shape)}")
    K = w_shape[1]
    if K > MAX_K:
        raise ValueError(f"{K} directions: at most {MAX_K}")
    if tuple(re_shape) != (B, F, T) or tuple(im_shape) != (B, F, T):
        raise ValueError(f"the noisy planes are [{B},{F},{T}], got {tuple(re_shape)} and {tuple(im_shape)}")
    if len(z_shape) != 4 or z_shape[0] != B or z_shape[2] != K or z_shape[3] != 2 or z_shape[1] < 1:
        raise ValueError(f"coefficients are [{B},S,{K}], got {tuple(z_shape[:3])}")
    S = z_shape[1]
    if (stats or spec_stats) and not 2 <= S <= MAX_STAT_S:
        raise ValueError(f"statistics need 2 <= S <= {MAX_STAT_S} samples, got {S}")
    length = int(length)
    if length < 1 or ops.stft_frames(length, hop) > T:
        raise ValueError(f"length {length} needs {ops.stft_frames(max(length, 0), hop)} frames (at least 1 sample), the planes have {T}")
    host = None
    if lengths is not None:
        host = [int(n) for n in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(host) != B:
            raise ValueError(f"lengths has {len(host)} entries for a batch of {B}")
        for b, n in enumerate(host):
            if n > length:
                raise ValueError(f"item {b}: length {n} exceeds the padded length {length}")
            if n <= nfft // 2:
                raise ValueError(f"item {b}: length {n} is too short (needs more than {nfft // 2} samples)")
    return B, S, K, F, T, host


def sample_waveforms(pred_crm, w_mat, noisy_re, noisy_im, coeffs, length, nfft=512, hop=256, lengths=None, domain="compressed",
                     samples=True, stats=False, spec_stats=False):
    """Waveforms of the posterior samples m_s = pred_crm + sum_k z_sk w_k (domain "compressed": combined, then decompressed;
    "decompressed": the validator's linear convention, decompress(pred) + sum_k z_sk decompress(w_k)), each applied to the
    noisy STFT with the true complex product and inverted as ops.istft does, in one fused launch.

    pred_crm [B,2,F,T] compressed, w_mat [B,K,2,F,T], noisy_re / noisy_im [B,F,T] (or [B,1,F,T]), coeffs [B,S,K] real or
    complex, or [B,S,K,2].  lengths [B]: a ragged batch as ops.istft's (samples past an item's end are 0).
    -> dict: "samples" [B,S,length] (samples=True); "mean", "std" [B,length] over the samples (stats=True); "mag_mean",
    "mag_std" [B,F,T] of |X_s| (spec_stats=True).  With samples=False nothing of size S is allocated.
    ValueError before any launch for what the kernel does not take (check_sample_args)."""
    z = as_coefficients(coeffs)
    if noisy_re.dim() == 4:
        noisy_re, noisy_im = noisy_re.squeeze(1), noisy_im.squeeze(1)
    B, S, K, F, T, host = check_sample_args(pred_crm.shape, w_mat.shape, noisy_re.shape, noisy_im.shape, z.shape, length, nfft,
                                            hop, lengths, domain, samples, stats, spec_stats)
    length = int(length)
    flags = (1 if stats else 0) | (2 if spec_stats else 0)
    _, _, nbytes = sample_tiling(B, S, K, T, nfft, hop, length, flags)
    pred_crm, w_mat, noisy_re, noisy_im, z = (ops._f32c(t) for t in (pred_crm, w_mat, noisy_re, noisy_im, z))
    dev = pred_crm.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {}
    if samples:
        out["samples"] = new(B, S, length)
    if stats:
        out["mean"], out["std"] = new(B, length), new(B, length)
    if spec_stats:
        out["mag_mean"], out["mag_std"] = new(B, F, T), new(B, F, T)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
    dl = torch.tensor(host, dtype=torch.int32).to(dev) if host is not None else None
    with torch.cuda.device(dev):
        H.call("nppc_post_sample", pred_crm, w_mat, noisy_re, noisy_im, z, dl, DOMAINS[domain], B, S, K, T, nfft, hop, length,
               out.get("samples"), out.get("mean"), out.get("std"), out.get("mag_mean"), out.get("mag_std"), work, nbytes,
               H.stream())
    return out


class PosteriorSamplerConfig(pydantic.BaseModel):
    nppc_audio_model_configuration: NPPCModelConfig
    checkpoint_path: str
    device: Literal["cpu", "cuda"] = "cuda"


class PosteriorSampler:
    """Posterior samples of noisy clips from an NPPC checkpoint: the model's front and forward run once per batch, then
    sample_waveforms.  `model=` takes an NPPCModel that is already loaded (config may then be None)."""

    def __init__(self, config: Optional[PosteriorSamplerConfig] = None, model=None):
        if model is None:
            self.device = torch.device(config.device)
            model = NPPCModel(config.nppc_audio_model_configuration)
            path = Path(config.checkpoint_path).expanduser().absolute()
            if not path.exists():
                raise FileNotFoundError(f"Model file not found: {path}")
            model.load_state_dict(torch.load(path.as_posix(), map_location="cpu")["model_state_dict"])
            model.to(self.device)
        else:
            self.device = torch.device(model.device)
        self.config = config
        self.nppc_model = model.eval()

    def _stft(self):
        st = self.nppc_model.config.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        return st

    def outputs(self, noisy, lengths=None):
        """(pred_crm [B,2,F,T], w_mat [B,K,2,F,T], noisy re, im [B,F,T]) of noisy [B,L]: one front, one forward"""
        H.require_gpu()
        if noisy.dim() != 2:
            raise ValueError(f"Expected noisy shape [B,L], got {tuple(noisy.shape)}")
        noisy = noisy.to(self.device).float().contiguous()
        with torch.no_grad():
            w_mat = self.nppc_model(noisy, lengths=lengths)
            f = self.nppc_model._front(noisy, lengths=lengths)
        if w_mat.shape[-2] != f["re"].shape[-2]:
            raise ValueError("the directions cover fewer bins than the STFT (drop-band is a training-time layout): "
                             "put the model in eval mode")
        return f["pred_crm"], w_mat, f["re"], f["im"]

    def sample(self, noisy, n_samples=8, seed=None, coeffs=None, lengths=None, domain="compressed", complex_coeffs=False,
               temperature=1.0, samples=True, stats=False, spec_stats=False):
        """noisy [B,L] -> the dict of sample_waveforms plus "coeffs" [B,S,K,2] and "enhanced" [B,L] (the z = 0 waveform,
        ops.model_outputs_to_waveforms).  coeffs=None draws n_samples with draw_coefficients(seed=...)."""
        st = self._stft()
        pred_crm, w_mat, re, im = self.outputs(noisy, lengths)
        B, K = w_mat.shape[:2]
        z = as_coefficients(coeffs).to(self.device) if coeffs is not None else draw_coefficients(
            B, n_samples, K, seed=seed, complex_coeffs=complex_coeffs, temperature=temperature, device=self.device)
        L = noisy.shape[1]
        out = sample_waveforms(pred_crm, w_mat, re, im, z, L, st.nfft, st.hop_length, lengths=lengths, domain=domain,
                               samples=samples, stats=stats, spec_stats=spec_stats)
        out["coeffs"] = z
        out["enhanced"] = ops.model_outputs_to_waveforms(pred_crm, re[:, None], im[:, None], L, st.nfft, st.hop_length, lengths=lengths)
        return out

    def score_spread(self, noisy, clean, n_samples=16, metrics=("STOI", "SI_SDR"), lengths=None, seed=None, coeffs=None,
                     domain="compressed", sr=16000):
        """The spread of downstream scores under the posterior: every sample of every item scored against `clean` [B,L] by
        the ragged metrics (B * S rows in one call per metric).  -> {metric: {"enhanced", "mean", "std", "min", "max"}}, each a
        list of B floats (std over the samples, unbiased; 0 for one sample); only these are read by the host."""
        from .metrics import REGISTERED_METRICS
        for m in metrics:
            if m not in REGISTERED_METRICS:
                raise ValueError(f"{m} is not registered. Registered metrics: {sorted(REGISTERED_METRICS)}")
        if clean.shape != noisy.shape:
            raise ValueError("Clean and noisy audio must have the same shape")
        r = self.sample(noisy, n_samples=n_samples, seed=seed, coeffs=coeffs, lengths=lengths, domain=domain)
        B, S, L = r["samples"].shape
        clean = clean.to(self.device).float().contiguous()
        host = [L] * B if lengths is None else [int(n) for n in torch.as_tensor(lengths).reshape(-1).tolist()]
        ref = torch.cat((clean, clean[:, None].expand(B, S, L).reshape(B * S, L)))
        est = torch.cat((r["enhanced"], r["samples"].reshape(B * S, L)))
        rows = host + [n for n in host for _ in range(S)]
        out = {}
        for m in metrics:
            v = REGISTERED_METRICS[m](ref, est, sr=sr, lengths=rows).double()
            e, s = v[:B], v[B:].view(B, S)
            sd = s.std(dim=1) if S > 1 else torch.zeros(B, dtype=torch.float64, device=s.device)
            table = torch.stack((e, s.mean(dim=1), sd, s.amin(dim=1), s.amax(dim=1))).cpu()
            out[m] = {k: table[i].tolist() for i, k in enumerate(("enhanced", "mean", "std", "min", "max"))}
        return out

