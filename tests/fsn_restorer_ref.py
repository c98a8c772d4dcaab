"""Shared by the FullSubNet+ restorer-trainer tests: the two fixture configurations and the oracle's restatement of one
Trainer_Finetune step (fullsubnet_plus/trainer/trainer.py:316-353) -- STFT, drop-banded compressed cIRM target, forward,
MSE, autograd, clip_grad_norm_(10), Adam(1e-3, (0.9, 0.999)) -- in whatever dtype the weights are given."""
import math

import torch

from oracle import nppc_ref as R
from oracle import weights as W

# tiny: the g0_tiny shapes; c257: full F with a short clip.  G = num_groups_in_drop_band of the model; clip =
# clip_grad_norm_value (fsr_tiny: the train.toml 10, inactive at these gradient norms of ~0.3; fsr_c257: 0.1, active).
CONFIGS = {
    "fsr_tiny": dict(F=33, sbn=3, sbh=16, nfft=64, hop=32, B=4, G=2, L=1024, seed=21, first_clip=0, clip=10.0),
    "fsr_c257": dict(F=257, sbn=15, sbh=384, nfft=512, hop=256, B=3, G=2, L=4096, seed=22, first_clip=8, clip=0.1),
}
LR, BETAS, CLIP = 1e-3, (0.9, 0.999), 10.0


def weights(c):
    spec = W.restorer_spec(num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    return W.make_weights(spec, c["seed"])


def batch(c, first_clip=None):
    return W.synth_batch(c["B"], c["L"], first_clip=c["first_clip"] if first_clip is None else first_clip)


def loss_and_output(P, noisy, clean, c):
    """(loss, cRM [B,2,F',T], gt [B,2,F',T]) of one batch; noisy / clean [B,L] tensors of P's dtype"""
    mag, re, im = R.stft_parts(noisy, c["nfft"], c["hop"], c["nfft"])
    _, cre, cim = R.stft_parts(clean, c["nfft"], c["hop"], c["nfft"])
    B = noisy.shape[0]
    G = c["G"] if B > 1 else 1
    gt = R.ideal_mask(re[:, 0], im[:, 0], cre[:, 0], cim[:, 0])
    if B > 1:
        gt = R.band_drop(gt, G)
    out = R.restorer_forward(mag, re, im, P, groups=G, sb_neighbors=c["sbn"])
    loss = ((gt - out) ** 2).mean()
    return loss, out, gt


def clip_norm(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))


def train_steps(P, noisy, clean, c, n_steps, record=None, clip=CLIP):
    """n_steps Trainer_Finetune steps on the same batch, in place on P (leaf tensors); record(step, loss, out, grads,
    total_norm) sees each step's unclipped gradients before its update"""
    state = {}
    for t in range(1, n_steps + 1):
        for v in P.values():
            v.requires_grad_(True)
        loss, out, _ = loss_and_output(P, noisy, clean, c)
        names = list(P)
        gs = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names])))
        total = clip_norm(gs)
        if record is not None:
            record(t, loss.detach(), out.detach(), gs, total)
        coef = min(1.0, clip / (total + 1e-6))
        gs = {k: g * coef for k, g in gs.items()}
        with torch.no_grad():
            det = {k: v.detach() for k, v in P.items()}
            R.adam_step(det, gs, state, t, lr=LR, b1=BETAS[0], b2=BETAS[1])
    return P
