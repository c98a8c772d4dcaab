"""CPU: the restorer trainer (nppc_audio/inpainting/trainer/restoration_trainer.py) -- the fp64 oracle composition of its
step against the reference's own InpaintingTrainer (tests/golden/rst_*.npz, make_goldens_restoration.py), config parsing
of the reference yaml's trainer section, and the construction errors.

`restorer_step` below is the fp64 reference of one training step that the GPU tests use too: oracle.inpaint_ref's
train-mode U-Net (optionally with given dropout keep masks), the RestorationWrapper composite, the masked spectral MSE
(restoration_trainer.py:189-191), autograd, clip_grad_norm_(5) and Adam(0.5, 0.999)."""
import numpy as np
import pytest
import torch
import yaml

from golden_util import load, rel
from oracle import inpaint_ref as R
from oracle import weights as W

LR = 1e-4


def is_pre_bn_bias(name):
    """bias of a convolution that feeds a BatchNorm: exactly zero gradient (the batch mean absorbs it)"""
    return name.endswith((".0.bias", ".3.bias")) and not name.startswith("outc")


def trainable(P):
    return [k for k in P if P[k].is_floating_point() and "running_" not in k]


def masked_mse(out, clean, mask4):
    om = 1 - mask4
    return ((out - clean) ** 2 * om).sum() / (om.sum() + 1e-6)


def restorer_step(P, masked, mask, clean, keep=None, p_drop=0.0, new_stats=None):
    """loss and gradient of every trainable tensor of the fp64 restorer (train-mode BatchNorm) -> (loss, {name: grad}, out)"""
    names = trainable(P)
    leaves = {k: P[k].detach().requires_grad_(True) for k in names}
    Q = dict(P)
    Q.update(leaves)
    cn, mask4, mn, _, _ = R.preprocess(clean, masked, mask)
    x = R.unet_forward(mn, Q, "", train=True, new_stats=new_stats, keep=keep, p_drop=p_drop)
    out = mn * mask4 + x * (1 - mask4)
    loss = masked_mse(out, cn, mask4)
    grads = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))
    return loss.detach(), grads, out.detach()


def restorer_validate(P, masked, mask, clean):
    cn, mask4, mn, _, _ = R.preprocess(clean, masked, mask)
    with torch.no_grad():
        x = R.unet_forward(mn, P, "", train=False)
        return float(masked_mse(mn * mask4 + x * (1 - mask4), cn, mask4))


def fixture_batch(z):
    """(masked_spec [B,2,F,T], mask_frames [B,T], clean_spec [B,2,F,T]) float32 numpy of an rst_* fixture; the masked
    spectrogram is not stored: it is clean * mask, exactly as the generator checked"""
    mask, clean = z["mask_frames"], z["clean_spec"]
    return clean * mask[:, None, None, :], mask, clean


def gap_values(out, mask):
    """composite [B,1,F,T] -> its columns on the missing frames (mask 0), [n_gap_frames, F] (make_goldens_restoration.py)"""
    out, mask = np.asarray(out), np.asarray(mask)
    return out[:, 0].transpose(0, 2, 1)[mask == 0]


def oracle_run(meta, z, steps=2):
    """the reference loop body in fp64: per step the loss, gradients, clip total norm, then the state after the step"""
    c = meta["config"]
    P = {k: torch.from_numpy(np.asarray(v)).double() if v.dtype.kind == "f" else torch.from_numpy(np.asarray(v))
         for k, v in W.make_weights(W.unet_spec(1, 1), c["seed"]).items()}
    batch = [torch.from_numpy(a).double() for a in fixture_batch(z)]
    adam, res = {}, []
    for it in range(1, steps + 1):
        new_stats = {}
        loss, grads, out = restorer_step(P, *batch, new_stats=new_stats)
        coef, total = R.clip_coef(grads.values(), 5.0)
        params = {k: P[k] for k in grads}
        R.adam_step(params, {k: g * coef for k, g in grads.items()}, adam, it, lr=LR, b1=0.5, b2=0.999)
        P.update(params)
        P.update(new_stats)
        res.append(dict(loss=float(loss), grads=grads, out=out, total=total, state={k: v.clone() for k, v in P.items()}))
    return res, restorer_validate(P, *batch), P


@pytest.mark.parametrize("name", ["rst_tiny", "rst_c3s"])
def test_fp64_oracle_reproduces_the_reference_trainer(name):
    z, meta = load(name)
    res, val, _ = oracle_run(meta, z)
    w0 = {k: np.asarray(v) for k, v in W.make_weights(W.unet_spec(1, 1), meta["config"]["seed"]).items()}
    assert rel(gap_values(res[0]["out"].numpy(), z["mask_frames"]), z["step1.output_gap"]) < 1e-4
    for it in (1, 2):
        r = res[it - 1]
        assert abs(r["loss"] - meta[f"step{it}.loss"]) < 1e-5 * abs(meta[f"step{it}.loss"]), (it, r["loss"])
        assert abs(r["total"] - meta[f"step{it}.clip_total_norm"]) < 1e-4 * meta[f"step{it}.clip_total_norm"]
    assert max(meta["step1.clip_total_norm"], meta["step2.clip_total_norm"]) > 5.0      # the clip is active
    # every parameter gradient of step 1 (leading slice + whole-tensor L2)
    assert len(res[0]["grads"]) == meta["n_params"]
    for n, g in res[0]["grads"].items():
        absmax, l2 = meta["step1.grad_absmax_l2"][n]
        if is_pre_bn_bias(n):
            assert float(g.abs().max()) < 1e-12 and absmax < 1e-5
            continue
        want = z["step1.grad." + n]
        got = g.numpy().reshape(-1)[: want.size]
        assert np.abs(got - want).max() < 1e-2 * absmax, n
        assert abs(float(g.norm()) - l2) < 1e-3 * l2, n
    # parameters after one and two clipped Adam steps (update = state after - initial weights); BatchNorm running buffers
    for it in (1, 2):
        st = res[it - 1]["state"]
        for n, v in st.items():
            key = f"step{it}.state.{n}"
            if key not in z.files:
                assert int(v) == meta[key], n          # num_batches_tracked
                continue
            want = z[key]
            got = v.numpy().reshape(-1)[: want.size]
            if "running_" in n:
                assert rel(got, want) < 1e-4, (it, n)
            elif is_pre_bn_bias(n):
                continue        # the reference's fp32 gradient here is rounding noise; Adam turns its sign into +-lr
            else:
                w = w0[n].reshape(-1)[: want.size]
                d = np.abs((got - w) - (want - w))
                assert (d > 0.05 * LR * it + 1e-7).sum() <= max(1, 1e-2 * d.size) and np.median(d) < 2e-6, (it, n)
    assert abs(val - meta["validate.loss"]) < 1e-4 * abs(meta["validate.loss"])


# trainer section of nppc_audio/inpainting/scripts/train/config/config.yaml (reference)
REF_YAML = """
inpainting_training_configuration:
  use_wandb: true
  wandb_project_name: "generative-audio"
  wandb_run_name: "restoration-inpainting-model-128ms-gap-size"
  wandb_artifact_name: "restoration_model"
  wandb_tags:
    - "128ms_gap"
    - "use_vad"
    - "2.044sec_audio_len"
    - "libriSpeech_dataset"
    - "dropout_0.2"
  device: "cuda"
  model_configuration:
    in_channels: 1
    out_channels: 1
    dropout: 0.2
  data_configuration:
    clean_path: "../../../../../../data/LibriSpeech/LibriSpeech/train-clean-360"
    sample_rate: 16000
    missing_length_seconds: 0.128
    missing_start_seconds: 0.4
    sub_sample_length_seconds: 2.044
    target_dB_FS: -25.0
    target_dB_FS_floating_value: 0
    use_vad: true
    stft_configuration:
      nfft: 255
      win_length: 255
      hop_length: 128
  dataloader_configuration:
    batch_size: 128
    shuffle: true
    num_workers: 8
    pin_memory: true
  optimizer_configuration:
    type: "Adam"
    args:
      lr: 1.0e-4
      betas: [0.5, 0.999]
"""


def yaml_config(**override):
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainerConfig
    d = yaml.safe_load(REF_YAML)["inpainting_training_configuration"]
    d.update(override)
    return InpaintingTrainerConfig(**d)


def test_reference_yaml_trainer_section_parses():
    cfg = yaml_config()
    assert cfg.model_configuration.in_channels == 1 and cfg.model_configuration.out_channels == 1
    assert cfg.model_configuration.dropout == 0.2 and cfg.model_configuration.precision == "bf16"
    assert cfg.data_configuration.stft_configuration.nfft == 255 and cfg.data_configuration.stft_configuration.hop_length == 128
    assert cfg.data_configuration.sub_sample_length_seconds == 2.044 and cfg.data_configuration.use_vad
    assert cfg.dataloader_configuration.batch_size == 128
    assert cfg.optimizer_configuration.type == "Adam"
    assert cfg.optimizer_configuration.args == {"lr": 1e-4, "betas": [0.5, 0.999]}
    assert cfg.use_wandb and cfg.wandb_tags[-1] == "dropout_0.2" and cfg.wandb_artifact_name == "restoration_model"
    assert cfg.max_grad_norm == 5.0 and cfg.device == "cuda"
    # the saved config round-trips (save_checkpoint stores model_dump(mode="json"))
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainerConfig
    assert InpaintingTrainerConfig(**cfg.model_dump(mode="json")) == cfg


def test_construction_errors():
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainer
    with pytest.raises(NotImplementedError, match="wandb"):
        InpaintingTrainer(yaml_config(), dataset=[1])
    with pytest.raises(ValueError, match="dataset"):
        InpaintingTrainer(yaml_config(use_wandb=False))
