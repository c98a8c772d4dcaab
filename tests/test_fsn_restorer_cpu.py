"""CPU: FullSubNetPlusTrainer configuration (train.toml defaults), construction errors, the checkpoint layout
(base_trainer.py:173-184) and its strict load into FullSubNet_Plus / through nppc_model.preload_model, the bench tool's
argument handling, and the fp64 oracle step the GPU tests compare against."""
import os
import sys

import numpy as np
import pytest
import torch

from fsn_restorer_ref import CONFIGS, batch, loss_and_output, train_steps, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Mem(torch.utils.data.Dataset):
    def __init__(self, n=4, L=1024):
        self.x = torch.zeros(n, L)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.x[i]


def tiny_cfg(**kw):
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainerConfig
    c = CONFIGS["fsr_tiny"]
    d = dict(model_configuration=dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                      num_groups_in_drop_band=c["G"], precision="fp32"),
             dataloader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False),
             stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cpu")
    d.update(kw)
    return FullSubNetPlusTrainerConfig(**d)


def test_config_defaults_follow_train_toml():
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainerConfig
    cfg = FullSubNetPlusTrainerConfig(model_configuration={})
    assert cfg.optimizer_configuration.type == "Adam"
    assert cfg.optimizer_configuration.args["lr"] == 1e-3
    assert tuple(cfg.optimizer_configuration.args["betas"]) == (0.9, 0.999)
    assert cfg.clip_grad_norm_value == 10.0
    st = cfg.stft_configuration
    assert (st.nfft, st.hop_length, st.win_length) == (512, 256, 512)
    assert cfg.model_configuration.precision == "bf16" and cfg.model_configuration.num_freqs == 257
    assert cfg.data_configuration is None and cfg.device == "cuda"
    cfg2 = FullSubNetPlusTrainerConfig.model_validate(dict(
        model_configuration=dict(num_groups_in_drop_band=2, precision="fp32"),
        data_configuration=dict(data_path=".", dataset=dict(clean_path="c", noisy_path="n", snr_range=[-5, 20])),
        dataloader_configuration=dict(batch_size=18), optimizer_configuration=dict(type="Adam", args=dict(lr=5e-4)),
        clip_grad_norm_value=5))
    assert cfg2.data_configuration.dataset.snr_range == (-5, 20) and cfg2.clip_grad_norm_value == 5.0
    assert cfg2.model_configuration.num_groups_in_drop_band == 2


def test_construction_errors():
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer
    with pytest.raises(ValueError, match="larger than the num_groups"):
        FullSubNetPlusTrainer(tiny_cfg(dataloader_configuration=dict(batch_size=2)), dataset=_Mem())
    bad_model = dict(num_freqs=33, sb_num_neighbors=3, sb_model_hidden_size=16, sequence_model="GRU")
    with pytest.raises(NotImplementedError):
        FullSubNetPlusTrainer(tiny_cfg(model_configuration=bad_model), dataset=_Mem())
    with pytest.raises(ValueError, match="bins"):
        FullSubNetPlusTrainer(tiny_cfg(stft_configuration=dict(nfft=128, hop_length=64, win_length=128)), dataset=_Mem())
    with pytest.raises(NotImplementedError):
        FullSubNetPlusTrainer(tiny_cfg(stft_configuration=dict(nfft=64, hop_length=32, win_length=48)), dataset=_Mem())
    with pytest.raises(ValueError, match="dataset"):
        FullSubNetPlusTrainer(tiny_cfg())


def test_checkpoint_layout_and_strict_load(tmp_path):
    from nppc_audio.fullsubnet import FullSubNet_Plus
    from nppc_audio.nppc_model import preload_model
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer
    cfg = tiny_cfg()
    tr = FullSubNetPlusTrainer(cfg, dataset=_Mem())
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights(CONFIGS["fsr_tiny"]).items()}, strict=True)
    path = tr.save_checkpoint(os.path.join(str(tmp_path), "ck", "latest_model.tar"))
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"epoch", "step", "best_score", "optimizer", "scaler", "model"}
    assert ck["epoch"] == 0 and ck["step"] == 0 and ck["scaler"] == {}
    assert set(ck["optimizer"]) == {"state", "param_groups"} and ck["optimizer"]["param_groups"][0]["lr"] == 1e-3
    assert len(ck["model"]) == len(list(tr.model.parameters()))
    fresh = FullSubNet_Plus(cfg.model_configuration)
    fresh.load_state_dict(ck["model"], strict=True)
    for n, p in fresh.named_parameters():
        assert torch.equal(p, dict(tr.model.named_parameters())[n]), n
    loaded = preload_model(path, FullSubNet_Plus(cfg.model_configuration))
    assert torch.equal(loaded.sb_model.fc_output_layer.weight, tr.model.sb_model.fc_output_layer.weight)


def test_bench_tool_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_fsn_restorer as b
    finally:
        sys.path.pop(0)
    a = b.parse([])
    assert (a.batch, a.seconds, a.groups, a.precision, a.steps, a.warmup) == (18, 3.072, 2, "both", 10, 3)
    a = b.parse(["--batch", "32", "--seconds", "4", "--precision", "fp32"])
    assert (a.batch, a.seconds, a.precision) == (32, 4.0, "fp32")
    for bad in (["--batch", "2"], ["--steps", "0"], ["--seconds", "0"], ["--precision", "fp16"], ["--groups", "0"]):
        with pytest.raises(SystemExit):
            b.parse(bad)


@pytest.mark.parametrize("name", ["fsr_tiny"])
def test_oracle_step_is_consistent(name):
    """the fp64 oracle of the GPU tests: the MSE's gradient is 2 (cRM - gt) / N, and one Adam step moves every weight by
    at most lr, most of them by lr (the first Adam step is lr * g / (|g| + eps))"""
    c = CONFIGS[name]
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in weights(c).items()}
    noisy, clean = (torch.from_numpy(a).double() for a in batch(c))
    loss, out, gt = loss_and_output(P, noisy, clean, c)
    Fo = (c["F"] - c["F"] % c["G"]) // c["G"]
    assert tuple(out.shape) == (c["B"], 2, Fo, 1 + c["L"] // c["hop"]) and out.shape == gt.shape
    (g_out,) = torch.autograd.grad(loss, [out])
    assert torch.allclose(g_out, 2 * (out - gt).detach() / out.numel())
    w0 = {k: v.detach().clone() for k, v in P.items()}
    seen = []
    train_steps(P, noisy, clean, c, 1, record=lambda t, l, o, gs, tot: seen.append((float(l), tot)))
    assert abs(seen[0][0] - float(loss.detach())) < 1e-12 and seen[0][1] > 0
    step = np.concatenate([(P[k].detach() - w0[k]).abs().reshape(-1).numpy() for k in P])
    assert step.max() <= 1e-3 * (1 + 1e-9) and np.median(step) > 0.5e-3


def ill_conditioned(n):
    """real / imag full-band branches: offline_laplace_norm of signed maps, noise-limited in fp32 (test_train_step_gpu.py)"""
    return "_real." in n or "_imag." in n


def fixture_tol(n):
    """error / max|g| of a reference fp32 gradient against fp64 (the policy of test_train_step_gpu.py's reference check)"""
    return 0.1 if ill_conditioned(n) else (2e-2 if ".prelu" in n else 5e-3)


def oracle_run(z, c):
    """the fp64 oracle through two Trainer_Finetune steps on the fixture's batch, then the validation loss"""
    P = {k: torch.from_numpy(v).double() for k, v in weights(c).items()}
    noisy, clean = torch.from_numpy(z["noisy"]).double(), torch.from_numpy(z["clean"]).double()
    rec = {}

    def record(t, loss, out, gs, total):
        rec[t] = dict(loss=float(loss), out=out.numpy(), grads={k: v.numpy() for k, v in gs.items()}, total=total)
        if t == 2:
            rec["w1"] = {k: v.detach().numpy().copy() for k, v in P.items()}
    train_steps(P, noisy, clean, c, 2, record=record, clip=c["clip"])
    rec["w2"] = {k: v.detach().numpy().copy() for k, v in P.items()}
    with torch.no_grad():
        rec["validate"] = float(np.mean([float(loss_and_output(P, noisy[i:i + 1], clean[i:i + 1], c)[0])
                                         for i in range(c["B"])]))
    return rec


def weights_off(got, w0, want, t, lr=1e-3):
    """share of the elements whose update differs by more than 5 % of lr per step, pooled over (well, ill)-conditioned"""
    off = {"well": [0, 0], "ill": [0, 0]}
    for n in want:
        d = np.abs((got(n) - w0[n]) - (want[n] - w0[n]))
        tag = "ill" if ill_conditioned(n) else "well"
        off[tag][0] += int((d > 0.05 * lr * t + 1e-9).sum())
        off[tag][1] += d.size
    return {k: a / b for k, (a, b) in off.items()}


@pytest.mark.parametrize("name", ["fsr_tiny", "fsr_c257"])
def test_fp64_oracle_reproduces_the_reference_fixture(name):
    """tests/golden/fsr_*.npz were made by the reference's FullSubNet_Plus and Trainer_Finetune loop body in fp32
    (make_goldens_fsn_restorer.py); the fp64 oracle the GPU tests also use must reproduce them at the fp32 floor"""
    from golden_util import load, rel
    z, meta = load(name)
    c = meta["config"]
    assert c == CONFIGS[name]
    assert np.array_equal(z["noisy"], batch(c)[0]) and np.array_equal(z["clean"], batch(c)[1])
    r = oracle_run(z, c)
    S = meta["slice"]
    assert abs(r[1]["loss"] - meta["step1.loss"]) / meta["step1.loss"] < 1e-5
    assert rel(z["step1.output"], r[1]["out"]) < 3e-4
    bad = {}
    for n, (amax, l2) in meta["step1.grad_absmax_l2"].items():
        g = r[1]["grads"][n]
        err = float(np.abs(g.reshape(-1)[:S] - z[f"step1.grad.{n}"]).max() / (amax + 1e-30))
        assert abs(np.abs(g).max() - amax) <= fixture_tol(n) * amax + 1e-30, n
        assert abs(np.sqrt((g ** 2).sum()) - l2) <= fixture_tol(n) * l2 + 1e-30, n
        if err > fixture_tol(n):
            bad[n] = err
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert abs(r[1]["total"] - meta["step1.clip_total_norm"]) / meta["step1.clip_total_norm"] < 1e-4
    w0 = {n: v.reshape(-1)[:S] for n, v in weights(c).items()}
    for t in (1, 2):
        want = {n: z[f"step{t}.param.{n}"] for n in meta["step1.grad_absmax_l2"]}
        off = weights_off(lambda n: r[f"w{t}"][n].reshape(-1)[:S], w0, want, t)
        assert off["well"] <= 0.002 and off["ill"] <= 0.05, (t, off)
    # after one update the two runs part (elements at the gradient noise floor took opposite Adam steps).  The step-2
    # gradient norm is the loosest: at fsr_c257 it grows from 0.28 to 1.7 after the update and is carried by the
    # ill-conditioned real / imag branches (measured 7.7e-2 apart; limit 2x that)
    assert abs(r[2]["loss"] - meta["step2.loss"]) / meta["step2.loss"] < 1e-3
    assert abs(r[2]["total"] - meta["step2.clip_total_norm"]) / meta["step2.clip_total_norm"] < 0.15
    # the validation loss runs on the weights after step 2: fsr_c257 measured 2.2e-2 apart (fsr_tiny 1.1e-6)
    assert abs(r["validate"] - meta["validate.loss"]) / meta["validate.loss"] < 5e-2
    print(name, "oracle vs reference: loss2", abs(r[2]["loss"] - meta["step2.loss"]) / meta["step2.loss"],
          "clip2", abs(r[2]["total"] - meta["step2.clip_total_norm"]) / meta["step2.clip_total_norm"],
          "validate", abs(r["validate"] - meta["validate.loss"]) / meta["validate.loss"])
