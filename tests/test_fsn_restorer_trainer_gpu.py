"""GPU: the FullSubNet+ restorer trainer (nppc_audio/restorer_trainer.py) -- the sub-band unfold backward and the cIRM MSE
kernels through the C ABI against fp64, the whole Trainer_Finetune step (output, loss, every gradient, clip norm, weights
after two Adam steps) against the fp64 oracle, train-mode vs inference forward, repeatability, and the
trainer -> checkpoint -> NPPCModel hand-off."""
import os

import numpy as np
import pytest
import torch

from fsn_restorer_ref import CONFIGS, LR, batch, train_steps, weights
from golden_util import rel
from oracle import nppc_ref as R

pytestmark = pytest.mark.gpu
PRECS = [("fp32", 1, torch.float32), ("bf16", 0, torch.bfloat16)]
SB_FWD_LIMIT = {"fp32": 1e-5, "bf16": 9e-3}      # test_forward_gpu.TAP_LIMITS["sb"]: the sub-band output of the forward


def rup(a, b):
    return (a + b - 1) // b * b


class _Mem(torch.utils.data.Dataset):
    def __init__(self, noisy, clean):
        self.n, self.c = torch.as_tensor(noisy), torch.as_tensor(clean)

    def __len__(self):
        return self.n.shape[0]

    def __getitem__(self, i):
        return self.n[i], self.c[i]


def ill_conditioned(n):
    """real / imag full-band branches: laplace norm of signed maps, noise-limited in fp32 (test_train_step_gpu.py)"""
    return "_real." in n or "_imag." in n


def make_trainer(c, precision, clip=10.0, G=None):
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer, FullSubNetPlusTrainerConfig
    cfg = FullSubNetPlusTrainerConfig(
        model_configuration=dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                 num_groups_in_drop_band=c["G"] if G is None else G, precision=precision),
        dataloader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False, shuffle=False),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]),
        clip_grad_norm_value=clip, device="cuda")
    noisy, clean = batch(c)
    tr = FullSubNetPlusTrainer(cfg, dataset=_Mem(noisy, clean))
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights(c).items()}, strict=True)
    return tr, (torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda())


# ---- 1a. sub-band unfold backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype", PRECS)
@pytest.mark.parametrize("B,F,nb,G,Tv", [(3, 33, 3, 2, 45), (4, 34, 3, 2, 130), (3, 9, 7, 2, 20), (5, 17, 5, 2, 129),
                                         (1, 17, 5, 2, 7), (4, 257, 15, 2, 19), (3, 33, 3, 1, 11)])
def test_unfold_backward_matches_fp64_autograd(pname, prec, dtype, B, F, nb, G, Tv, record_err):
    from nppc_audio import _hip as Hh
    from nppc_audio.engine import unfold_multiplicity
    g = torch.Generator().manual_seed(B * 1000 + F * 10 + nb)
    W = 2 * nb + 1
    nfeat = W + 3
    KX = rup(nfeat + 1, 16)
    Tp = rup(Tv, 128)
    ldX = rup(F, 64) + 64
    Geff = G if B > 1 else 1
    # the attention-scaled magnitude (rounded to the staging precision) and the three full-band outputs
    x0 = (torch.rand(B, 1, F, Tv, generator=g, dtype=torch.float64) + 0.1).to(dtype).double().requires_grad_(True)
    fb = torch.rand(B, 3, F, Tv, generator=g, dtype=torch.float64).to(dtype).double()
    unf = R.subband_unfold(x0, nb)                                       # [B, F, W, Tv]
    sb_raw = torch.cat([unf, fb.permute(0, 2, 1, 3)], dim=2)             # [B, F, nfeat, Tv]
    sb = R.laplace_norm(sb_raw)
    if B > 1:
        sb = R.band_drop(sb.permute(0, 2, 1, 3), Geff).permute(0, 2, 1, 3)   # [B, Fo, nfeat, Tv]
    Fo = sb.shape[1]
    dy = torch.randn(sb.shape, generator=g, dtype=torch.float64).to(dtype).double()
    (gx,) = torch.autograd.grad((sb * dy).sum(), [x0])
    sc = (1.0 / (sb_raw.detach().mean(dim=(1, 2, 3)) + 1e-5)).float()
    D = (sb.detach() * dy).sum(dim=(1, 2, 3))                            # [B'] in drop-band order
    dx = torch.zeros(Tv, B * Fo, KX, dtype=dtype)
    dx[:, :, :nfeat] = dy.permute(3, 0, 1, 2).reshape(Tv, B * Fo, nfeat).to(dtype)
    init = (torch.randn(B, Tp, ldX, generator=g) * 0.1).to(dtype)
    outs = []
    for _ in range(2):
        dX0 = init.clone().cuda()
        Hh.call("nppc_subband_unfold_bwd", prec, dx.cuda(), sc.cuda(), D.cuda(), torch.from_numpy(unfold_multiplicity(F, nb)).cuda(),
                dX0, ldX, B, F, Tp, Tv, nb, G, KX, Hh.stream())
        torch.cuda.synchronize()
        outs.append(dX0.cpu())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    got = outs[0]
    # untouched: the frames past Tv and the columns past F
    assert torch.equal(got[:, Tv:], init[:, Tv:]) and torch.equal(got[:, :, F:], init[:, :, F:])
    want = init[:, :Tv, :F].double() + gx[:, 0].permute(0, 2, 1)
    err = float((got[:, :Tv, :F].double() - want).abs().max() / gx.abs().max())
    record_err(f"unfold_bwd.{pname}", err, 2e-5 if pname == "fp32" else 2e-2)


# ---- 1b. cIRM MSE ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,T,G", [(3, 33, 17, 2), (4, 257, 13, 2), (5, 31, 9, 3), (2, 9, 5, 1), (1, 7, 3, 1)])
def test_crm_mse_matches_fp64(B, F, T, G, record_err):
    from nppc_audio import ops
    from nppc_audio.restorer_trainer import crm_mse
    g = torch.Generator().manual_seed(B * 100 + F + T)
    nr, ni, cr, ci = (torch.randn(B, F, T, generator=g) for _ in range(4))
    Fo = F if G <= 1 else (F - F % G) // G
    crm = (torch.randn(B, 2, Fo, T, generator=g) * 3).requires_grad_(True)
    gt64 = R.ideal_mask(nr.double(), ni.double(), cr.double(), ci.double())
    if G > 1:
        gt64 = R.band_drop(gt64, G)
    crm64 = crm.detach().double().requires_grad_(True)
    loss64 = ((gt64 - crm64) ** 2).mean()
    (0.7 * loss64).backward()
    runs = []
    for _ in range(2):
        x = crm.detach().cuda().requires_grad_(True)
        loss, gt = crm_mse(x, nr.cuda(), ni.cuda(), cr.cuda(), ci.cuda(), G)
        (0.7 * loss).backward()
        torch.cuda.synchronize()
        runs.append((loss.cpu(), gt.cpu(), x.grad.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"
    loss, gt, dcrm = runs[0]
    record_err("crm_mse.loss", abs(float(loss) - float(loss64)) / float(loss64), 1e-5)
    record_err("crm_mse.gt", rel(gt.numpy(), gt64.numpy()), 1e-5)
    record_err("crm_mse.grad", rel(dcrm.numpy(), crm64.grad.numpy()), 1e-5)
    if B > G:         # the target is the one nppc_cirm_build_compress builds
        assert torch.equal(gt, ops.cirm_build_compress(nr.cuda(), ni.cuda(), cr.cuda(), ci.cuda(), G).cpu())


# ---- 2. whole Trainer_Finetune step against the fp64 oracle --------------------------------------------------------------
_ORACLE = {}


def fp64_oracle(name, clip):
    key = (name, clip)
    if key not in _ORACLE:
        c = CONFIGS[name]
        P = {k: torch.from_numpy(v).double() for k, v in weights(c).items()}
        noisy, clean = (torch.from_numpy(a).double() for a in batch(c))
        rec = {}

        def record(t, loss, out, gs, total):
            rec[t] = dict(loss=float(loss), out=out.numpy(), grads={k: v.numpy() for k, v in gs.items()}, total=total)
            if t == 2:
                rec["w1"] = {k: v.detach().numpy().copy() for k, v in P.items()}
        train_steps(P, noisy, clean, c, 2, record=record, clip=clip)
        rec["w2"] = {k: v.detach().numpy().copy() for k, v in P.items()}
        _ORACLE[key] = rec
    return _ORACLE[key]


# bf16 limits, error / max|grad| per family of the well-conditioned tensors (PReLU slopes, scalars, excluded): 2 x the worst
# measured on the two fixtures (attention 0.0210, TCN 0.2646, full-band Linear 0.1078, sub-band LSTM + head 0.00469)
BF16_GRAD_LIMITS = {"attention": 0.042, "tcn": 0.529, "fb_fc": 0.215, "sb_model": 0.0093}
# the other bf16 limits, 2 x the worst measured against either the fp64 oracle or the reference fixture: relative loss
# (steps 1 and 2) 4.67e-4, step-1 output 8.72e-3, clip norm 2.33e-4, cosine deficit of the gradient 4.07e-6, validation
# loss after two steps 5.06e-2; weights off by > 5 % of lr: well-conditioned 0.42, real / imag 0.228 (fsr_tiny step 2)
BF16_LIMITS = {"loss": 9.3e-4, "output1": 1.74e-2, "clip_norm": 4.6e-4, "cos_deficit": 8e-6, "validate": 0.1}


def family(n):
    return ("sb_model" if n.startswith("sb_model.") else "attention" if n.startswith("channel_attention") else
            "tcn" if ".sequence_model." in n else "fb_fc")


@pytest.mark.parametrize("name,precision", [("fsr_tiny", "fp32"), ("fsr_c257", "fp32"), ("fsr_tiny", "bf16"),
                                            ("fsr_c257", "bf16")])
def test_two_trainer_steps_match_fp64_oracle(name, precision, record_err):
    """step 1: loss, output, clip norm and every gradient; steps 1 and 2: the weights.  The step-2 gradients are not
    compared: Adam's first step moves every element by about lr * sign(g), so elements whose gradient is at the noise
    floor (the real / imag branches, PReLU slopes) take opposite steps in fp32 and fp64 and the two runs part."""
    c = CONFIGS[name]
    clip = 0.1                       # below the gradient norm (about 0.27 here): the clip is active
    ref = fp64_oracle(name, clip)
    fp32 = precision == "fp32"
    tr, bt = make_trainer(c, precision, clip=clip)
    params = dict(tr.model.named_parameters())
    w0 = {k: v.detach().cpu().numpy().copy() for k, v in params.items()}
    for t in (1, 2):
        loss, log = tr.train_step(bt)
        torch.cuda.synchronize()
        r = ref[t]
        record_err(f"loss{t}", abs(float(loss) - r["loss"]) / r["loss"], (1e-5 if t == 1 else 1e-4) if fp32 else BF16_LIMITS["loss"])
        if t == 1 or fp32:
            # (after one update the outputs part measurably: elements at the gradient noise floor took opposite Adam steps,
            # and the real / imag branches are ill-conditioned; bf16 step 2 is held through the loss and the weights)
            record_err(f"output{t}", rel(log["cRM"].cpu().numpy(), r["out"]), (3e-4 if t == 1 else 2e-2) if fp32 else BF16_LIMITS["output1"])
        if t == 1:
            record_err("clip_norm", abs(float(log["grad_norm"]) - r["total"]) / r["total"], 1e-5 if fp32 else BF16_LIMITS["clip_norm"])
            eng = tr.model.engine()
            worst = {}
            dot = n_g = n_r = 0.0
            for n in params:
                gg = eng.fp.gview(n).detach().cpu().double().numpy()
                rg = r["grads"][n]
                worst[n] = float(np.abs(gg - rg).max() / (np.abs(rg).max() + 1e-300))
                dot, n_g, n_r = dot + float((gg * rg).sum()), n_g + float((gg * gg).sum()), n_r + float((rg * rg).sum())
            # the magnitude-branch attention reads the gradient of the unfold columns (nppc_subband_unfold_bwd)
            att = max(v for n, v in worst.items() if n.startswith("channel_attention."))
            print(name, precision, "worst:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])
            record_err("grad.cos_deficit", 1.0 - dot / np.sqrt(n_g * n_r), 1e-6 if fp32 else BF16_LIMITS["cos_deficit"])
            if fp32:
                record_err("grad.channel_attention", att, 1e-3)
                record_err("grad.well_conditioned", max(v for n, v in worst.items() if not ill_conditioned(n)), 1e-2)
                record_err("grad.ill_conditioned", max(v for n, v in worst.items() if ill_conditioned(n)), 0.25)
            else:
                fam = {}
                for n, v in worst.items():
                    if not ill_conditioned(n) and ".prelu" not in n:
                        fam[family(n)] = max(fam.get(family(n), 0.0), v)
                record_err("grad.channel_attention", att, BF16_GRAD_LIMITS["attention"])
                for k, v in fam.items():
                    record_err(f"grad.{k}", v, BF16_GRAD_LIMITS[k])
        # weights after the step: the Adam update is about lr per element; the share of elements whose update is off by
        # more than 5 % of lr per step, pooled over the well- and the ill-conditioned tensors
        wr = ref[f"w{t}"]
        off = {"well": [0, 0], "ill": [0, 0]}
        for n, p in params.items():
            d = np.abs((p.detach().cpu().numpy() - w0[n]) - (wr[n] - w0[n])).reshape(-1)
            tag = "ill" if ill_conditioned(n) else "well"
            off[tag][0] += int((d > 0.05 * LR * t + 1e-9).sum())
            off[tag][1] += d.size
        lim = {"well": 0.002, "ill": 0.05} if fp32 else {"well": 0.8, "ill": 0.45}   # bf16: 2 x the worst measured (0.42, 0.228)
        for tag, (k, m) in off.items():
            record_err(f"weights{t}.{tag}.frac_off", k / m, lim[tag])


@pytest.mark.parametrize("name,precision", [("fsr_tiny", "fp32"), ("fsr_c257", "fp32"), ("fsr_tiny", "bf16"),
                                            ("fsr_c257", "bf16")])
def test_two_trainer_steps_match_reference_fixture(name, precision, record_err):
    """the same two steps against tests/golden/fsr_*.npz, made by the REFERENCE's FullSubNet_Plus and Trainer_Finetune loop
    body in fp32 (make_goldens_fsn_restorer.py) at the fixture's clip (fsr_tiny: train.toml's 10, inactive; fsr_c257:
    0.1, active): step-1 loss, output, clip norm and gradient slices, weights after steps 1 and 2, the step-2 loss and
    the validation loss.  Gradients: error / max|g| of the tensor, the reference's own fp32 floor of
    test_train_step_gpu.py (5e-3, PReLU slopes 2e-2, real / imag branches 0.1) in fp32; bf16 families as above."""
    from golden_util import load
    z, meta = load(name)
    c = meta["config"]
    assert c == CONFIGS[name]
    fp32 = precision == "fp32"
    S = meta["slice"]
    tr, _ = make_trainer(c, precision, clip=c["clip"])
    bt = (torch.from_numpy(z["noisy"]).cuda(), torch.from_numpy(z["clean"]).cuda())
    params = dict(tr.model.named_parameters())
    w0 = {n: v.reshape(-1)[:S] for n, v in weights(c).items()}
    for t in (1, 2):
        loss, log = tr.train_step(bt)
        torch.cuda.synchronize()
        ref_loss = meta[f"step{t}.loss"]
        if t == 1:
            record_err("loss1", abs(float(loss) - ref_loss) / ref_loss, 1e-5 if fp32 else BF16_LIMITS["loss"])
            record_err("output1", rel(log["cRM"].cpu().numpy(), z["step1.output"]), 3e-4 if fp32 else BF16_LIMITS["output1"])
            record_err("clip_norm1", abs(float(log["grad_norm"]) - meta["step1.clip_total_norm"]) / meta["step1.clip_total_norm"],
                       1e-5 if fp32 else BF16_LIMITS["clip_norm"])
            eng = tr.model.engine()
            worst, fam = {}, {}
            for n, (amax, _) in meta["step1.grad_absmax_l2"].items():
                g = eng.fp.gview(n).detach().cpu().numpy().reshape(-1)[:S]
                worst[n] = float(np.abs(g - z[f"step1.grad.{n}"]).max() / (amax + 1e-30))
            att = max(v for n, v in worst.items() if n.startswith("channel_attention."))
            print(name, precision, "vs reference, worst:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])
            if fp32:
                record_err("grad.channel_attention", att, 5e-3)
                bad = {n: v for n, v in worst.items()
                       if v > (0.1 if ill_conditioned(n) else (2e-2 if ".prelu" in n else 5e-3))}
                assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
            else:
                for n, v in worst.items():
                    if not ill_conditioned(n) and ".prelu" not in n:
                        fam[family(n)] = max(fam.get(family(n), 0.0), v)
                record_err("grad.channel_attention", att, BF16_GRAD_LIMITS["attention"])
                for k, v in fam.items():
                    record_err(f"grad.{k}", v, BF16_GRAD_LIMITS[k])
        else:
            # after one update the runs part (elements at the gradient noise floor took opposite Adam steps): the loss
            record_err("loss2", abs(float(loss) - ref_loss) / ref_loss, 1e-3 if fp32 else BF16_LIMITS["loss"])
        off = {"well": [0, 0], "ill": [0, 0]}
        for n, p in params.items():
            d = np.abs((p.detach().cpu().numpy().reshape(-1)[:S] - w0[n]) - (z[f"step{t}.param.{n}"] - w0[n]))
            tag = "ill" if ill_conditioned(n) else "well"
            off[tag][0] += int((d > 0.05 * LR * t + 1e-9).sum())
            off[tag][1] += d.size
        lim = {"well": 0.002, "ill": 0.05} if fp32 else {"well": 0.8, "ill": 0.45}
        for tag, (k, m) in off.items():
            record_err(f"weights{t}.{tag}.frac_off", k / m, lim[tag])
    # validation: one clip at a time (no drop-band), mean loss, no gradients; on the weights after step 2
    val = tr.validate([(bt[0][i:i + 1], bt[1][i:i + 1]) for i in range(c["B"])])
    # fp32: the fp64 oracle itself is 2.2e-2 from the reference here (test_fsn_restorer_cpu.py)
    record_err("validate", abs(val - meta["validate.loss"]) / meta["validate.loss"], 5e-2 if fp32 else BF16_LIMITS["validate"])


def test_train_forward_equals_inference_forward(record_err):
    for name, prec in (("fsr_tiny", "fp32"), ("fsr_c257", "fp32"), ("fsr_c257", "bf16")):
        c = CONFIGS[name]
        tr, (noisy, _) = make_trainer(c, prec)
        from nppc_audio import ops
        mag, re, im = ops.stft(noisy, c["nfft"], c["hop"])
        out_train = tr.model(mag[:, None], re[:, None], im[:, None])
        assert out_train.requires_grad
        with torch.no_grad():
            out_inf = tr.model(mag[:, None], re[:, None], im[:, None])
        record_err(f"{name}.{prec}", rel(out_train.detach().cpu().numpy(), out_inf.cpu().numpy()), SB_FWD_LIMIT[prec])


def test_two_runs_agree(record_err):
    """two identical two-step runs.  DEVIATION from the issue, which asks for bit-identical weights: the new kernels are
    bit-identical on repeat (tested above), but the step as a whole cannot promise it.  Existing kernels -- the TCN
    GroupNorm statistics, the sub-band mean, the staging backward's D and nppc_sumsq -- reduce with fp64 atomics whose
    last bits follow the arrival order.  Measured: of three runs of an earlier form of this test that asserted equality, one
    failed; the other two gave max |dw| = 0.  Held: the share of weights that
    differ by more than 1e-3 lr."""
    c = CONFIGS["fsr_tiny"]
    flats = []
    for _ in range(2):
        tr, bt = make_trainer(c, "bf16")
        for _ in range(2):
            tr.train_step(bt)
        torch.cuda.synchronize()
        flats.append(tr.model.engine().fp.flat.detach().cpu().clone())
    d = (flats[0] - flats[1]).abs()
    print("two runs: max |dw|", float(d.max()), "elements differing", int((d > 0).sum()), "of", d.numel())
    record_err("frac_differing", float((d > 1e-6).double().mean()), 1e-3)


def test_frozen_restorer_forward_unchanged_under_no_grad():
    """the inference path NPPC uses: frozen parameters with grad enabled and no_grad give the same bits"""
    c = CONFIGS["fsr_tiny"]
    tr, (noisy, _) = make_trainer(c, "bf16", G=1)
    from nppc_audio import ops
    mag, re, im = ops.stft(noisy, c["nfft"], c["hop"])
    with torch.no_grad():
        a = tr.model(mag[:, None], re[:, None], im[:, None])
    for p in tr.model.parameters():
        p.requires_grad_(False)
    b = tr.model(mag[:, None], re[:, None], im[:, None])
    assert not b.requires_grad and torch.equal(a, b)


def test_checkpoint_into_nppc_model_and_one_nppc_step(tmp_path):
    from nppc_audio.fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
    from nppc_audio.nppc_model import NPPCModel, NPPCModelConfig
    from nppc_audio.trainer import nppc_base_step
    c = CONFIGS["fsr_tiny"]
    tr, bt = make_trainer(c, "fp32")
    hist = tr.train(n_steps=2, checkpoint_dir=str(tmp_path), save_flag=False)
    assert len(hist) == 2 and all(np.isfinite(hist))
    path = tr.save_checkpoint(os.path.join(str(tmp_path), "restorer.tar"))
    ck = torch.load(path, map_location="cpu")
    assert {"epoch", "best_score", "optimizer", "scaler", "model"} <= set(ck)
    common = dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"], precision="fp32")
    fresh = FullSubNet_Plus(FullSubNetPlusConfig(**common))
    fresh.load_state_dict(ck["model"], strict=True)
    cfg = NPPCModelConfig(
        pretrained_restoration_model_configuration=dict(common, num_groups_in_drop_band=1),
        pretrained_restoration_model_path=path,
        audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(common, num_groups_in_drop_band=2,
                                                                               n_directions=2)),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda")
    model = NPPCModel(cfg)
    noisy, clean = bt
    pred = model.get_pred_crm(noisy)
    # the trained net's own eval output: one clip at a time (B = 1: no drop-band, whatever G the trainer used)
    from nppc_audio import ops
    mag, re, im = ops.stft(noisy, c["nfft"], c["hop"])
    with torch.no_grad():
        own = torch.cat([tr.model(mag[i:i + 1, None], re[i:i + 1, None], im[i:i + 1, None]) for i in range(noisy.shape[0])])
    assert rel(pred.cpu().numpy(), own.cpu().numpy()) < 1e-5
    for n, p in model.pretrained_restoration_model.named_parameters():
        assert torch.equal(p.detach().cpu(), dict(tr.model.named_parameters())[n].detach().cpu()), n
    _, obj, _ = nppc_base_step(model, bt, 500, 500, 1.0)
    obj.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(obj))
    g = model.audio_pc_wrapper.net.sb_model.fc_output_layer.weight.grad
    assert g is not None and bool(torch.isfinite(g).all())
