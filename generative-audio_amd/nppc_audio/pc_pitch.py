"""f0 contours of the speech-enhancement validator's PC audio: `enhanced + alpha * PC_k` for every direction and alpha
(ops.pc_direction_waveforms, nppc_audio/validator.py:148-302 of the reference), tracked by pitch.pyin on the device."""
import torch

from . import ops
from . import pitch as PT

__all__ = ["pc_direction_pitch"]


def pc_direction_pitch(model, noisy, alphas, fmin=80.0, fmax=400.0, sr=16000):
    """model: a loaded NPPCModel in eval mode; noisy [B, L] on the device; alphas: sequence of floats ->
    {'enhanced' [B,L], 'variations' [B,K,A,L] (exactly ops.pc_direction_waveforms' outputs), 'f0_clean' [B,T] (the contour of
    `enhanced`), 'voiced_flag_clean', 'voiced_prob_clean', 'f0' [B,K,A,T], 'voiced_flag', 'voiced_prob', 'summary'}."""
    st = model.config.stft_configuration
    with torch.no_grad():
        w_mat = model(noisy)
        front = model._front(noisy)
        enhanced, variations = ops.pc_direction_waveforms(front["pred_crm"], w_mat, alphas, front["re"], front["im"],
                                                          noisy.shape[-1], st.nfft, st.hop_length)
        out = PT.contours_of_variations(enhanced, variations, fmin=fmin, fmax=fmax, sr=sr)
    out["enhanced"], out["variations"] = enhanced, variations
    return out
