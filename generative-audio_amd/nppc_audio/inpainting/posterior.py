"""Posterior samples of inpainted gaps (csrc/inpaint_posterior.hip; specification
tests/inpaint_posterior_ref.py).

The direction net's output is Gram-Schmidt'd: K orthogonal, un-normalised directions w_k, zero on known frames, whose norms
are the predicted spread.  In the normalised log-magnitude domain, where the loss is defined, the model states
    x = pred + sum_k z_k w_k,   z_k ~ N(0, 1) real
and a magnitude sample is exp(x std + mean).  `sample_waveforms` turns coefficients z [B,S,K] into S waveforms per item on
the clean recording's phase (held-out data), and / or their statistics, in one fused launch; `sample_waveforms_blind` does
it without the clean phase, by gap-constrained Griffin-Lim (phase.py) with the sampled magnitudes formed on the fly.  No
[B,S,F,T] stack is ever formed.  `InpaintingPosteriorSampler` wraps both around a checkpoint.  The K-direction Gaussian is
the model's statement of the posterior, not the true one.
"""
import ctypes
from typing import Optional

import torch

from .. import _hip as H
from .. import ops
from .. import posterior as SE
from . import phase as PH

__all__ = ["draw_coefficients", "as_coefficients", "sample_shape", "check_sample_args", "sample_waveforms",
           "sample_waveforms_blind", "InpaintingPosteriorSampler", "MAX_K", "TILE", "MAX_STAT_S"]

MAX_K = 16               # NPPC_INP_POST_MAX_K
TILE = 8                 # NPPC_INP_POST_TILE
MAX_STAT_S = 4096        # NPPC_INP_POST_MAX_STAT_S
MAX_V = 65535            # variations of one Griffin-Lim call (S + 1)


def draw_coefficients(B, S, K, seed=None, generator=None, temperature=1.0, device="cuda"):
    """z [B,S,K] fp32: the real parts of nppc_audio.posterior.draw_coefficients (temperature * randn), so a seed means the
    same coefficients in both modules"""
    return SE.draw_coefficients(B, S, K, seed=seed, generator=generator, temperature=temperature, device=device)[..., 0].contiguous()


def as_coefficients(coeffs):
    """[B,S,K] real -> fp32 contiguous.  A real log-magnitude has no use for a complex coefficient: ValueError."""
    if not isinstance(coeffs, torch.Tensor):
        raise ValueError("coeffs is a real tensor [B,S,K]")
    if coeffs.is_complex():
        raise ValueError("complex coefficients have no meaning for a real log-magnitude: coeffs are real [B,S,K]")
    if coeffs.dim() != 3:
        raise ValueError(f"coeffs are [B,S,K], got {tuple(coeffs.shape)}")
    return coeffs.float().contiguous()


def sample_shape(B, S, K, T, n_fft=255, hop_length=128, length=None, stats=0, no_stage=False):
    """nppc_inp_post_sample_shape; needs no GPU.  stats: bit 0 time, bit 1 spectrum.  -> dict(length, tiles, tile_samples,
    work_bytes, staged (the planes of a workgroup live in LDS) and lds_bytes of the path the shape takes)"""
    L = ops.istft_natural_length(n_fft, hop_length, T) if length is None else int(length)
    tiles, per, staged, nbytes, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    try:
        with ops.envelope_refusal(n_fft, hop_length, T, L):
            H.call("nppc_inp_post_sample_shape", B, S, K, T, n_fft, hop_length, L, stats, 1 if no_stage else 0,
                   ctypes.byref(tiles), ctypes.byref(per), ctypes.byref(nbytes), ctypes.byref(staged), ctypes.byref(lds))
    except (RuntimeError, ctypes.ArgumentError, OverflowError) as e:
        raise ValueError(f"inpainting posterior: B {B}, S {S}, K {K}, T {T}, n_fft {n_fft}, hop {hop_length}, length {L}: {e}") from e
    return {"length": L, "tiles": tiles.value, "tile_samples": per.value, "work_bytes": nbytes.value,
            "staged": bool(staged.value), "lds_bytes": lds.value}


def check_sample_args(pred_shape, pc_shape, clean_shape, z_shape, n_fft, hop_length, length, samples, stats, spec_stats):
    """every refusal of sample_waveforms as a ValueError, from shapes alone (no GPU, no launch) -> (B, S, K, F, T, L)"""
    if not (samples or stats or spec_stats):
        raise ValueError("inpainting posterior: nothing asked for (samples, stats and spec_stats are all off)")
    if n_fft > 512:
        raise ValueError(f"inpainting posterior: n_fft {n_fft} > 512")
    if len(pc_shape) != 4:
        raise ValueError(f"pc_directions_mag is [B,K,F,T], got {tuple(pc_shape)}")
    B, K, F, T = pc_shape
    if F != n_fft // 2 + 1:
        raise ValueError(f"{F} frequency bins do not fit n_fft {n_fft}")
    if K > MAX_K:
        raise ValueError(f"{K} directions: at most {MAX_K}")
    if tuple(pred_shape) != (B, 1, F, T):
        raise ValueError(f"pred_spec_mag is [{B},1,{F},{T}], got {tuple(pred_shape)}")
    if clean_shape is not None and tuple(clean_shape) != (B, 2, F, T):
        raise ValueError(f"clean_spec is [{B},2,{F},{T}], got {tuple(clean_shape)}")
    if len(z_shape) != 3 or z_shape[0] != B or z_shape[2] != K or z_shape[1] < 1:
        raise ValueError(f"coefficients are [{B},S,{K}] with S >= 1, got {tuple(z_shape)}")
    S = z_shape[1]
    if (stats or spec_stats) and not 2 <= S <= MAX_STAT_S:
        raise ValueError(f"statistics need 2 <= S <= {MAX_STAT_S} samples, got {S}")
    L = ops.check_istft_any_config(n_fft, hop_length, T, length)
    if ops.istft_envelope_min(n_fft, hop_length, T, L) < 1e-11:
        raise ValueError(f"istft: window overlap add min < 1e-11 for n_fft {n_fft}, hop {hop_length}, {T} frames")
    return B, S, K, F, T, L


def _scalar(v, dev):
    return torch.as_tensor(v, dtype=torch.float32).to(dev).reshape(1).contiguous()


def sample_waveforms(pred_spec_mag, pc_directions_mag, clean_spec, coeffs, mean, std, n_fft=255, hop_length=128, length=None,
                     samples=True, stats=False, spec_stats=False, no_stage=False):
    """Waveforms of the posterior samples on the clean phase:
        samples[b,s] = istft(exp((pred[b] + sum_k coeffs[b,s,k] pc[b,k]) std + mean) exp(i angle(clean[b])))
    pred_spec_mag [B,1,F,T], pc_directions_mag [B,K,F,T] (normalised log-magnitudes), clean_spec [B,2,F,T], coeffs [B,S,K]
    real, mean / std the batch statistics of preprocess_data (device scalars, read on the device).  At coeffs = alpha e_k
    this is pc_audio_variations[b,k] at alpha, bit for bit.
    -> dict: "samples" [B,S,L] (samples=True); "mean", "std" [B,L] over the samples (stats=True); "mag_mean", "mag_std"
    [B,F,T] of the linear magnitudes (spec_stats=True).  With samples=False nothing of size S is allocated.  no_stage=True
    forces the path that re-reads the planes from global memory (measurements).  ValueError before any launch for what
    the kernel does not take (check_sample_args)."""
    z = as_coefficients(coeffs)
    B, S, K, F, T, L = check_sample_args(pred_spec_mag.shape, pc_directions_mag.shape, clean_spec.shape, z.shape, n_fft,
                                         hop_length, length, samples, stats, spec_stats)
    flags = (1 if stats else 0) | (2 if spec_stats else 0)
    nbytes = sample_shape(B, S, K, T, n_fft, hop_length, L, flags, no_stage)["work_bytes"]
    H.require_gpu()
    pred, pc, cs = (ops._f32c(t) for t in (pred_spec_mag, pc_directions_mag, clean_spec))
    dev = pc.device
    z = z.to(dev)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {}
    if samples:
        out["samples"] = new(B, S, L)
    if stats:
        out["mean"], out["std"] = new(B, L), new(B, L)
    if spec_stats:
        out["mag_mean"], out["mag_std"] = new(B, F, T), new(B, F, T)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        H.call("nppc_inp_post_sample", pred, pc, cs, _scalar(mean, dev), _scalar(std, dev), z, B, S, K, T, n_fft, hop_length, L,
               1 if no_stage else 0, out.get("samples"), out.get("mean"), out.get("std"), out.get("mag_mean"),
               out.get("mag_std"), work, nbytes, H.stream())
    return out


def sample_waveforms_blind(pred_spec_mag, pc_directions_mag, masked_spec, mask, coeffs, mean, std, n_iter=32, momentum=0.0,
                           init_phase=None, n_fft=255, hop_length=128, length=None, max_span=None, long_spans=False,
                           long_max_span=None):
    """sample_waveforms without the clean phase, mirroring phase.pc_audio_variations_blind: masked_spec [B,2,F,T] (the
    damaged recording's STFT), mask [B,T] or [B,1,F,T], coeffs [B,S,K] real -> (samples [B,S,L], restored [B,L], info):
        samples[b,s] = griffin_lim_gap(exp((pred[b] + sum_k coeffs[b,s,k] pc[b,k]) std + mean), ...)
        restored[b]  = the same at coeffs = 0
    from one call with V = S + 1 (the prediction last); info as griffin_lim_gap.  At coeffs = alpha e_k the sample is
    pc_audio_variations_blind's variation, bit for bit.  Time-domain statistics of these are a torch reduction over dim 1."""
    z = as_coefficients(coeffs)
    pred, pc, known = PH._f32c(pred_spec_mag), PH._f32c(pc_directions_mag), PH._f32c(masked_spec)
    if pc.dim() != 4:
        raise ValueError(f"pc_directions_mag {tuple(pc.shape)}: want [B,K,F,T]")
    B, K, F, T = pc.shape
    if pred.shape != (B, 1, F, T):
        raise ValueError(f"pred_spec_mag {tuple(pred.shape)} does not fit directions {tuple(pc.shape)}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{K} directions: between 1 and {MAX_K}")
    if z.shape[0] != B or z.shape[2] != K or z.shape[1] < 1:
        raise ValueError(f"coefficients are [{B},S,{K}] with S >= 1, got {tuple(z.shape)}")
    S = z.shape[1]
    if S + 1 > MAX_V:
        raise ValueError(f"{S} samples: at most {MAX_V - 1} per call")
    mask = PH._f32c(mask)
    if mask.dim() == 4:
        mask = mask[:, 0, 0, :].contiguous()
    V = S + 1
    sh, init_phase, w = PH._prepare(known, mask, init_phase, V, F, T, n_fft, hop_length, length, n_iter, momentum, max_span,
                                    long_spans, long_max_span)
    suffix, tail = PH._tail(max_span, long_spans, long_max_span)
    if init_phase.dim() != 3:
        raise ValueError("sample_waveforms_blind takes one initial phase per item, [B,F,T]")
    dev = pc.device
    with ops.envelope_refusal(n_fft, hop_length, T, sh["length"]):
        H.call("nppc_gl_gap_post" + suffix, pred, pc, _scalar(mean, dev), _scalar(std, dev), z.to(dev), known, mask, init_phase,
               w["out"], w["dist"], w["tn"], w["status"], w["work"], w["work"].numel(), B, K, S, T, n_fft, hop_length,
               sh["length"], n_iter, float(momentum), *tail, H.stream())
    info = {"inconsistency": w["dist"], "target_norm": w["tn"], "status": w["status"]}
    return w["out"][:, :S], w["out"][:, S], info


class InpaintingPosteriorSampler:
    """Posterior samples of damaged clips from an inpainting NPPC checkpoint (loaded as NPPCModelValidator loads it; or
    `model=` an NPPCModel that is already loaded, config may then be None)."""

    def __init__(self, config=None, model=None):
        if model is None:
            from .validator.validator_nppc_model import NPPCModelValidator
            val = NPPCModelValidator(config)
            model, self.device = val.model, val.device
        else:
            self.device = next(model.parameters()).device
        self.config = config
        self.model = model.eval()

    def sample(self, masked_spec, mask, clean_spec=None, n_samples=8, seed=None, coeffs=None, phase="clean", stats=False,
               spec_stats=False, temperature=1.0, n_fft=255, hop_length=128, gl_iters=32, long_spans=False):
        """masked_spec [B,2,F,T], mask [B,T] (1 = known), clean_spec [B,2,F,T] (phase="clean" needs it: ValueError
        without) -> dict: "coeffs" [B,S,K] (coeffs=None draws n_samples with draw_coefficients(seed=...)), "samples"
        [B,S,L], and
          phase="clean":        "mean", "std" (stats=True), "mag_mean", "mag_std" (spec_stats=True) of sample_waveforms;
          phase="griffin_lim":  "restored" [B,L], "phase_info" of sample_waveforms_blind; "mean", "std" (stats=True) by a
                                torch reduction; spec_stats as above (they do not depend on the phase).
        preprocess_data, the direction net and the restorer run once."""
        from .utils import preprocess_data
        if phase not in ("clean", "griffin_lim"):
            raise ValueError(f"phase = {phase!r}: 'clean' or 'griffin_lim'")
        if phase == "clean" and clean_spec is None:
            raise ValueError("phase='clean' borrows the clean recording's phase: pass clean_spec, or phase='griffin_lim'")
        H.require_gpu()
        self.model.eval()
        with torch.no_grad():
            masked_spec, mask = masked_spec.to(self.device), mask.to(self.device)
            ref = masked_spec if clean_spec is None else clean_spec.to(self.device)
            _, mask4, masked_norm, mean, std = preprocess_data(ref, masked_spec, mask, plot_mean_std=True)
            mask4 = mask4.contiguous()
            pc = self.model(masked_norm, mask4)
            pred = self.model.get_pred_spec_mag_norm(masked_norm, mask4)
            B, K = pc.shape[:2]
            z = as_coefficients(coeffs).to(self.device) if coeffs is not None else draw_coefficients(
                B, n_samples, K, seed=seed, temperature=temperature, device=self.device)
            if phase == "clean":
                out = sample_waveforms(pred, pc, ref, z, mean, std, n_fft, hop_length, stats=stats, spec_stats=spec_stats)
            else:
                smp, restored, info = sample_waveforms_blind(pred, pc, masked_spec, mask4, z, mean, std, n_iter=gl_iters,
                                                             n_fft=n_fft, hop_length=hop_length, long_spans=long_spans)
                out = {"samples": smp, "restored": restored, "phase_info": info}
                if stats:
                    if z.shape[1] < 2:
                        raise ValueError(f"statistics need at least 2 samples, got {z.shape[1]}")
                    out["mean"], out["std"] = smp.mean(1), smp.std(1)
                if spec_stats:
                    out.update(sample_waveforms(pred, pc, masked_spec, z, mean, std, n_fft, hop_length, samples=False,
                                                spec_stats=True))
        out["coeffs"] = z
        return out
