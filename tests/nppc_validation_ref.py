"""Shared fixtures of the NPPC validation tests (tests/test_nppc_validation_*.py): the tiny NPPC configuration and weights of
the forward / train-step tests (fixture g0_tiny), clips of the lengths tests/test_ragged_inference_gpu.py uses, and a numpy
restatement of nppc_audio.metrics.nppc_direction_scores."""
import os

import numpy as np
import torch

from oracle import weights as W

# g0_tiny STFT (nfft 64, hop 32, look-ahead 2): T = 125, 10 (the shortest legal clip: the TSSE kernel of 10), 127, 126, 132
# frames -> T + la = 127 (one short of a 128-row tile), 12, 129 (one past it), 128 (on it), 134
LENGTHS = [3970, 288, 4040, 4001, 4200]
# Which synthetic clips: fixed by the ORACLE's own error, computed on the CPU before any kernel ran.  The limits these tests
# take from the uniform tests hold on clips where fp32 itself is good enough: on most clips the oracle evaluated in fp32 (the
# reference's precision) is 2e-6 .. 4e-5 from its fp64 evaluation in w_mat, but the laplace norm of the signed real / imag
# maps (mean + 1e-5 ~ 1e-5 in the divisor) makes a few clips noise-limited in fp32 -- clip 172 at 4040 samples: 9.8e-4 in
# the oracle's own fp32, twice the 5e-4 limit, and 8.2e-4 on the MI355X (of the 72 clip / length pairs 170..181 x six
# lengths scanned, that one, and four more between 1e-4 and 2.5e-4).  Clips FIRST_CLIP .. FIRST_CLIP + 4 all have an
# fp32-oracle w_mat within ORACLE_FP32_FLOOR = 5e-5 (a tenth of that limit) of fp64; the w_mat test asserts it.  Clip 172
# stays a case of its own, with bounds from the oracle's fp32 error (test_ragged_w_mat_on_a_clip_that_fp32_cannot_resolve).
FIRST_CLIP = 173
ORACLE_FP32_FLOOR = 5e-5


def clips(lengths, first=FIRST_CLIP):
    out = []
    for i, n in enumerate(lengths):
        noisy, clean = W.synth_batch(1, n, first_clip=first + i)
        out.append((torch.from_numpy(noisy[0]), torch.from_numpy(clean[0])))
    return out


def padded(xs, fill=0.0):
    L = max(x.numel() for x in xs)
    out = torch.full((len(xs), L), fill, dtype=torch.float32)
    for i, x in enumerate(xs):
        out[i, :x.numel()] = x
    return out


def nppc_weights(c):
    spec = W.nppc_spec(c["K"], num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    return {k: torch.from_numpy(v) for k, v in W.make_weights(spec, c["seed"]).items()}


def model_config(c, precision, tmp_path, g_pc=None):
    """NPPCModelConfig of fixture configuration c (tests/test_train_step_gpu.py::build_model), restorer checkpoint written
    under tmp_path"""
    from nppc_audio.nppc_model import NPPCModelConfig
    wts = nppc_weights(c)
    pre = "pretrained_restoration_model."
    ck = os.path.join(str(tmp_path), "restorer.tar")
    torch.save({"model": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    common = dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"], precision=precision)
    return NPPCModelConfig(
        pretrained_restoration_model_configuration=dict(common, num_groups_in_drop_band=c["G_rest"]),
        pretrained_restoration_model_path=ck,
        audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(
            common, num_groups_in_drop_band=c["G_pc"] if g_pc is None else g_pc, n_directions=c["K"])),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda"), wts


def build_model(c, precision, tmp_path, g_pc=None):
    from nppc_audio.nppc_model import NPPCModel
    cfg, wts = model_config(c, precision, tmp_path, g_pc)
    model = NPPCModel(cfg)
    model.load_state_dict(wts, strict=True)
    return model, wts


def oracle_step_alone(noisy, clean, P, c, step):
    """oracle/nppc_ref.nppc_step of ONE clip (a batch of one never drop-bands; nppc_step's band_drop asserts B > groups):
    -> (w_mat, log of nppc_loss) in the dtype of noisy / P"""
    from oracle import nppc_ref as R
    stft = (c["nfft"], c["hop"], c["nfft"])
    w, pred, parts = R.nppc_forward(noisy[None], P, c["K"], stft=stft, g_rest=1, g_pc=1, sb_neighbors=c["sbn"])
    _, c_re, c_im = R.stft_parts(clean[None], *stft)
    gt = R.ideal_mask(parts["re"][:, 0], parts["im"][:, 0], c_re[:, 0], c_im[:, 0])
    return w, R.nppc_loss(w, gt, pred, step)[2]


def direction_scores_np(err_norm, err_proj_mag, w_norms):
    """plain-loop restatement of metrics.nppc_direction_scores"""
    en, pm, wn = (np.asarray(a, np.float64) for a in (err_norm, err_proj_mag, w_norms))
    B, K = pm.shape
    cap = np.zeros((B, K))
    for b in range(B):
        acc = 0.0
        for k in range(K):
            acc += pm[b, k] ** 2
            cap[b, k] = acc
    pooled = np.array([sum(cap[b, k] * en[b] ** 2 for b in range(B)) / sum(en[b] ** 2 for b in range(B)) for k in range(K)])
    cal = np.array([np.sqrt(np.mean(pm[:, k] ** 2)) / np.sqrt(np.mean(wn[:, k] ** 2)) for k in range(K)])
    return dict(captured=cap, residual=1 - cap, captured_mean=cap.mean(0), residual_mean=1 - cap.mean(0),
                captured_pooled=pooled, residual_pooled=1 - pooled, calibration=cal, calibration_item=pm / wn)
