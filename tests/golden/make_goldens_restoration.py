#!/usr/bin/env python3
"""Generate the restorer-trainer golden fixtures (tests/golden/rst_*.npz) by RUNNING THE REFERENCE (CPU, fp32).

Same rules as make_goldens_inpainting.py: runs only in the build container, imports the reference from
/root/reference where it lies (with the same empty placeholder modules for the absent third-party packages), writes
data only.  The reference's own InpaintingTrainer (nppc_audio/inpainting/trainer/restoration_trainer.py) is built
with UNetConfig(1, 1, dropout=0) and the yaml's Adam arguments; weights come from oracle/weights.py (unet_spec(1, 1),
seeded numpy), batches from W.synth_inpaint_batch.  Two steps of the reference's loop body (base_step, zero_grad,
backward, clip_grad_norm_(5), Adam step), then validate().

Each fixture holds: the batch (clean spectrogram and frame mask), the composite output on the gap frames and
the loss of step 1, a leading slice of every parameter gradient
(plus max |g| and L2 of the whole tensor), the clip total norm, a leading slice of every parameter and every BatchNorm
running buffer after steps 1 and 2, and the validate() loss.

Usage:  python tests/golden/make_goldens_restoration.py
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

from oracle import weights as W  # noqa: E402
from make_goldens import install_placeholders, to_t  # noqa: E402

SLICE = 256


class MemDataset(torch.utils.data.Dataset):
    def __init__(self, cfg):
        pass

    def __len__(self):
        return 1

    def __getitem__(self, i):
        raise IndexError


def small(a, n=SLICE):
    return np.ascontiguousarray(a).reshape(-1)[:n].copy()


def gap_values(out, mask):
    """out [B,1,F,T] -> the columns of the missing frames (mask 0), [n_gap_frames, F] in (item, frame) order"""
    return np.ascontiguousarray(out[:, 0].transpose(0, 2, 1)[mask == 0])


def run_config(name, c, out_dir):
    from nppc_audio.inpainting.trainer import restoration_trainer as ref_tr

    torch.manual_seed(0)
    B, T = c["B"], c["T"]
    spec = W.unet_spec(1, 1)
    wts = W.make_weights(spec, c["seed"])
    masked, mask, clean = W.synth_inpaint_batch(B, T, c["nfft"], c["hop"])

    ref_tr.AudioInpaintingDataset = MemDataset
    cfg = ref_tr.InpaintingTrainerConfig(
        model_configuration=dict(in_channels=1, out_channels=1, dropout=0.0),
        data_configuration=dict(clean_path=".", stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"],
                                                                         win_length=c["nfft"]), use_vad=False),
        dataloader_configuration=dict(batch_size=B, num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.5, 0.999])),
        device="cpu")
    tr = ref_tr.InpaintingTrainer(cfg)
    net = tr.model.net
    sd = net.state_dict()
    assert list(sd.keys()) == list(spec.keys()), "state-dict names/order differ from oracle/weights.py unet_spec"
    net.load_state_dict(to_t(wts), strict=True)
    assert tr.model.training

    tm, tk, tc = torch.from_numpy(masked), torch.from_numpy(mask), torch.from_numpy(clean)
    audio = torch.zeros(B, 1, 8)                       # masked_audio: carried through base_step's log only
    # the masked spectrogram is clean * mask (exact for a 0/1 frame mask): the tests rebuild it, it is not stored
    assert np.array_equal(masked, clean * mask[:, None, None, :])
    out = {"mask_frames": mask, "clean_spec": clean}
    meta = {"config": c, "slice": SLICE, "n_params": len(list(net.parameters()))}
    params = dict(net.named_parameters())

    for it in (1, 2):
        loss, log = tr.base_step((tm, tk, tc, audio))
        tr.optimizer.zero_grad()
        loss.backward()
        meta[f"step{it}.loss"] = float(loss.detach())
        if it == 1:
            # the composite equals the normalised input on the known frames: only the gap frames carry the U-Net
            out["step1.output_gap"] = gap_values(log["output"].numpy(), mask)
            gn = {}
            for n, p in params.items():
                g = p.grad.numpy()
                out[f"step1.grad.{n}"] = small(g)
                gn[n] = [float(np.abs(g).max()), float(np.sqrt((g.astype(np.float64) ** 2).sum()))]
            meta["step1.grad_absmax_l2"] = gn
        tn = torch.nn.utils.clip_grad_norm_(tr.model.parameters(), max_norm=5)
        meta[f"step{it}.clip_total_norm"] = float(tn)
        tr.optimizer.step()
        for n, v in net.state_dict().items():
            if v.is_floating_point():
                out[f"step{it}.state.{n}"] = small(v.detach().numpy())
            else:
                meta[f"step{it}.state.{n}"] = int(v)

    val_loss = tr.validate([(tm, tk, tc, audio, {})])
    assert tr.model.training
    meta["validate.loss"] = float(val_loss)

    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **out)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    sz = os.path.getsize(os.path.join(out_dir, name + ".npz")) / 1e6
    print(f"[{name}] wrote {len(out)} arrays, {sz:.2f} MB; loss {meta['step1.loss']:.6f} -> {meta['step2.loss']:.6f}, "
          f"clip total norm {meta['step1.clip_total_norm']:.4g} / {meta['step2.clip_total_norm']:.4g}, "
          f"validate {val_loss:.6f}")
    return meta


CONFIGS = {
    # small spectrogram, odd sizes (floor-mode pooling, pad-to-skip on both axes); the U-Net widths are fixed
    "rst_tiny": dict(nfft=63, hop=32, T=37, B=3, seed=41),
    # reference yaml shape (nfft 255 / hop 128 -> F=128) at reduced batch and length
    "rst_c3s": dict(nfft=255, hop=128, T=101, B=2, seed=42),
}


def main():
    install_placeholders()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    metas = [run_config(name, CONFIGS[name], HERE) for name in (sys.argv[1:] or list(CONFIGS))]
    if not sys.argv[1:]:
        # the fixtures must exercise clip_grad_norm_ actually scaling the gradient
        assert any(m["step1.clip_total_norm"] > 5 or m["step2.clip_total_norm"] > 5 for m in metas), \
            [(m["step1.clip_total_norm"], m["step2.clip_total_norm"]) for m in metas]


if __name__ == "__main__":
    main()
