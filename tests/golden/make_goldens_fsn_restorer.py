#!/usr/bin/env python3
"""Generate the speech-enhancement restorer-trainer fixtures (tests/golden/fsr_*.npz) by RUNNING THE REFERENCE (CPU, fp32).

Same rules as make_goldens.py: runs only in the build container, imports the reference from /root/reference where it
lies (with the same empty placeholder modules for the absent third-party packages), writes data only.  The reference's
own FullSubNet_Plus (fullsubnet_plus/model/fullsubnet_plus.py) is built from its FullSubNetPlusConfig and fed
oracle/weights.py weights through load_state_dict; batches come from W.synth_batch.  Two iterations of the body of
Trainer_Finetune._train_epoch (fullsubnet_plus/trainer/trainer.py:323-349) run with the reference's own helpers: stft,
mag_phase, build_complex_ideal_ratio_mask, drop_band, then mse_loss (train.toml [loss_function]), backward,
clip_grad_norm_(clip) and Adam(lr 1e-3, betas (0.9, 0.999)) (train.toml [optimizer]; use_amp = false, so the scaler is an
identity).  Then the validation loss of _validation_epoch (:379-398): one clip at a time, cIRM without drop-band, mean.

Each fixture holds: the batch, the step-1 model output [B, 2, F', T] and loss, a leading slice of every parameter
gradient of step 1 (plus max |g| and L2 of the whole tensor), the clip total norm of both steps, a leading slice of every
parameter after steps 1 and 2, the step-2 loss and the validation loss.

Usage:  python tests/golden/make_goldens_fsn_restorer.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import weights as W  # noqa: E402
from make_goldens import install_placeholders, to_t  # noqa: E402
from fsn_restorer_ref import BETAS, CONFIGS, LR  # noqa: E402

SLICE = 128


def small(a, n=SLICE):
    return np.ascontiguousarray(a).reshape(-1)[:n].copy()


def run_config(name, c, out_dir):
    from FullSubNet_plus.speech_enhance.fullsubnet_plus.model.fullsubnet_plus import FullSubNet_Plus, FullSubNetPlusConfig
    from FullSubNet_plus.speech_enhance.audio_zen.acoustics.feature import drop_band, mag_phase, stft
    from FullSubNet_plus.speech_enhance.audio_zen.acoustics.mask import build_complex_ideal_ratio_mask

    torch.manual_seed(0)
    spec = W.restorer_spec(num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    wts = W.make_weights(spec, c["seed"])
    model = FullSubNet_Plus(FullSubNetPlusConfig(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                                 num_groups_in_drop_band=c["G"]))
    sd = model.state_dict()
    assert list(sd.keys()) == list(spec.keys()), "state-dict names/order differ from oracle/weights.py restorer_spec"
    model.load_state_dict(to_t(wts), strict=True)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=LR, betas=BETAS)
    torch_stft = lambda y: stft(y, c["nfft"], c["hop"], c["nfft"])        # noqa: E731  (base_trainer.py:52)

    noisy_np, clean_np = W.synth_batch(c["B"], c["L"], first_clip=c["first_clip"])
    noisy, clean = torch.from_numpy(noisy_np), torch.from_numpy(clean_np)
    out = {"noisy": noisy_np, "clean": clean_np}
    meta = {"config": c, "slice": SLICE, "n_params": len(spec)}
    params = dict(model.named_parameters())

    def loss_of(noisy, clean, drop):
        noisy_complex = torch_stft(noisy)
        clean_complex = torch_stft(clean)
        noisy_mag, _ = mag_phase(noisy_complex)
        gt = build_complex_ideal_ratio_mask(noisy_complex, clean_complex)                       # [B, F, T, 2]
        if drop:
            gt = drop_band(gt.permute(0, 3, 1, 2), model.num_groups_in_drop_band).permute(0, 2, 3, 1)
        cRM = model(noisy_mag.unsqueeze(1), noisy_complex.real.unsqueeze(1), noisy_complex.imag.unsqueeze(1))
        return torch.nn.functional.mse_loss(gt, cRM.permute(0, 2, 3, 1)), cRM

    for it in (1, 2):
        opt.zero_grad()
        loss, cRM = loss_of(noisy, clean, True)
        loss.backward()
        meta[f"step{it}.loss"] = float(loss.detach())
        if it == 1:
            out["step1.output"] = cRM.detach().numpy()
            gn = {}
            for n, p in params.items():
                g = p.grad.numpy()
                out[f"step1.grad.{n}"] = small(g)
                gn[n] = [float(np.abs(g).max()), float(np.sqrt((g.astype(np.float64) ** 2).sum()))]
            meta["step1.grad_absmax_l2"] = gn
        tn = torch.nn.utils.clip_grad_norm_(model.parameters(), c["clip"])
        meta[f"step{it}.clip_total_norm"] = float(tn)
        opt.step()
        for n, p in params.items():
            out[f"step{it}.param.{n}"] = small(p.detach().numpy())

    with torch.no_grad():                         # _validation_epoch: batch size one, no drop-band
        vl = [float(loss_of(noisy[i:i + 1], clean[i:i + 1], False)[0]) for i in range(c["B"])]
    meta["validate.loss"] = float(np.mean(vl))

    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    sz = os.path.getsize(path) / 1e6
    assert sz < 1.0, sz
    print(f"[{name}] wrote {len(out)} arrays, {sz:.2f} MB; loss {meta['step1.loss']:.6f} -> {meta['step2.loss']:.6f}, "
          f"clip total norm {meta['step1.clip_total_norm']:.4g} / {meta['step2.clip_total_norm']:.4g} (clip {c['clip']}), "
          f"validate {meta['validate.loss']:.6f}")
    return meta


def main():
    install_placeholders()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    metas = [run_config(name, CONFIGS[name], HERE) for name in (sys.argv[1:] or list(CONFIGS))]
    if not sys.argv[1:]:
        # one fixture at the train.toml clip (10: inactive at these norms), one where clip_grad_norm_ scales the gradient
        assert any(m["step1.clip_total_norm"] > m["config"]["clip"] for m in metas)


if __name__ == "__main__":
    main()
