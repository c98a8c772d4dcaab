"""GPU: the restorer trainer (nppc_audio/inpainting/trainer/restoration_trainer.py) -- the fused dropout + BatchNorm +
LeakyReLU backward and the masked spectral MSE kernels through the C ABI, the whole train step against the reference's
InpaintingTrainer fixtures (dropout 0) and against the fp64 oracle fed the tapped keep bits (dropout 0.2), and the
trainer -> checkpoint -> NPPCModel hand-off."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import load, rel
from oracle import weights as W
from test_restoration_cpu import LR, fixture_batch, gap_values, is_pre_bn_bias, restorer_step
from unet_halo import Halo

pytestmark = pytest.mark.gpu
PRECS = [("fp32", 1, torch.float32, 2e-5), ("bf16", 0, torch.bfloat16, 3e-2)]


def q(x, dtype):
    return x.to(dtype).float()


def keep_nchw(keep, B, H, W_, C):
    """[rows][C] u8 keep bits of nppc_dropout (haloed rows) -> [B,C,H,W] float"""
    return keep.reshape(B, H + 2, W_ + 2, C)[:, 1:-1, 1:-1].permute(0, 3, 1, 2).float().cpu()


# ---- 1. fused dropout + BatchNorm + LeakyReLU backward ---------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,dtype,tol", PRECS)
@pytest.mark.parametrize("B,H,W_,C", [(3, 7, 11, 64), (2, 5, 9, 512), (1, 9, 5, 128)])
def test_fused_dropout_bn_backward_matches_autograd(pname, prec, dtype, tol, B, H, W_, C, record_err):
    from nppc_audio import _hip as Hh
    p, seed, stream_id = 0.2, 0x1234_5678_9ABC, 6
    g = torch.Generator().manual_seed(C + H)
    x = q(torch.randn(B, C, H, W_, generator=g) * 2 + 0.5, dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    s = Hh.stream()
    X = Halo(B, H, W_, C, dtype).put(x)
    Y = Halo(B, H, W_, 2 * C, dtype)                   # the block output is a channel slice of a concat buffer
    st = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    ss = torch.empty(4 * C, dtype=torch.float32, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    Hh.call("nppc_bn_stats", prec, X.t, C, X.P, C, st, s)
    Hh.call("nppc_bn_finalize", st, gamma.cuda(), beta.cuda(), rm, rv, ss, C, float(B * H * W_), 1e-5, 0.1, 1, s)
    Hh.call("nppc_bn_act", prec, X.t, C, Y.t, 2 * C, ss, C, B, H, W_, 0.2, s)
    keep = torch.empty(X.P * C, dtype=torch.uint8, device="cuda")
    Hh.call("nppc_dropout", prec, Y.t, 2 * C, X.P, C, p, seed, stream_id, keep, s)
    torch.cuda.synchronize()
    km = keep_nchw(keep, B, H, W_, C)
    assert 0.77 < float(km.mean()) < 0.83
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = F.leaky_relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5), 0.2) * km / (1 - p)
    assert rel(Y.get(C), yr.detach()) < tol
    d1, d2 = q(torch.randn(B, C, H, W_, generator=g), dtype), q(torch.randn(B, C, H, W_, generator=g), dtype)
    yr.backward(d1 + d2)
    DA, DB = Halo(B, H, W_, C, dtype).put(d1), Halo(B, H, W_, 3 * C, dtype).put(d2, C)
    DX = Halo(B, H, W_, C, dtype)
    S = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    Hh.call("nppc_bn_bwd_dropout", prec, DA.t, C, DB.t[C:], 3 * C, Y.t, 2 * C, X.t, C, ss, S, DX.t, C, dgam, dbet, C, B, H, W_,
            0.2, p, seed, stream_id, s)
    torch.cuda.synchronize()
    record_err("dx", rel(DX.get(C), xr.grad), tol * 3)
    record_err("dgamma", rel(dgam.cpu(), gr.grad), tol * 3)
    record_err("dbeta", rel(dbet.cpu(), br.grad), tol * 3)
    assert DX.halo_is_zero()
    # p = 0: bit for bit the plain BatchNorm backward
    out = {}
    for name in ("nppc_bn_bwd", "nppc_bn_bwd_dropout"):
        DX0 = Halo(B, H, W_, C, dtype)
        dg0, db0 = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        extra = (0.0, seed, stream_id) if name == "nppc_bn_bwd_dropout" else ()
        Hh.call(name, prec, DA.t, C, DB.t[C:], 3 * C, Y.t, 2 * C, X.t, C, ss, S, DX0.t, C, dg0, db0, C, B, H, W_, 0.2, *extra, s)
        torch.cuda.synchronize()
        out[name] = (DX0.t.clone(), dg0.clone(), db0.clone())
    for a, b in zip(out["nppc_bn_bwd"], out["nppc_bn_bwd_dropout"]):
        assert torch.equal(a, b)


# ---- 2. masked spectral MSE -----------------------------------------------------------------------------------------
def _mse_ref(out, clean, m):
    om = (1 - m)[:, None, None, :].expand_as(out)
    return ((out - clean) ** 2 * om).sum() / (om.sum() + 1e-6)


@pytest.mark.parametrize("B,Fq,T,kind", [(3, 32, 37, "gap"), (2, 128, 101, "gap"), (2, 17, 9, "known"), (2, 17, 9, "missing"),
                                         (5, 128, 257, "random")])
def test_masked_mse_loss_and_gradient(B, Fq, T, kind, record_err):
    from nppc_audio.inpainting.trainer.restoration_trainer import masked_spectral_mse
    g = torch.Generator().manual_seed(B * T + Fq)
    out, clean = torch.randn(B, 1, Fq, T, generator=g), torch.randn(B, 1, Fq, T, generator=g)
    m = torch.ones(B, T)
    if kind == "gap":
        m[:, T // 3: T // 3 + 5] = 0
    elif kind == "missing":
        m.zero_()
    elif kind == "random":
        m = (torch.rand(B, T, generator=g) > 0.3).float()
    od = out.double().requires_grad_(True)
    ref = _mse_ref(od, clean.double(), m.double())
    ref.backward(torch.tensor(0.7, dtype=torch.float64))
    oc = out.cuda().requires_grad_(True)
    loss = masked_spectral_mse(oc, clean.cuda(), m.cuda())
    loss.backward(torch.tensor(0.7, device="cuda"))
    torch.cuda.synchronize()
    if kind == "known":                # denominator 1e-6: loss and gradient exactly 0
        assert float(loss) == 0.0 and float(oc.grad.abs().max()) == 0.0
        return
    record_err("loss", abs(float(loss) - float(ref)) / abs(float(ref)), 1e-6)
    record_err("grad", rel(oc.grad.cpu(), od.grad), 1e-6)
    # deterministic: no float atomics, the same inputs give the same bits
    again = masked_spectral_mse(oc.detach(), clean.cuda(), m.cuda())
    assert torch.equal(again, loss.detach())


# ---- 3 - 5. the whole train step ------------------------------------------------------------------------------------
class Mem(torch.utils.data.Dataset):
    def __init__(self, z):
        self.items = fixture_batch(z)

    def __len__(self):
        return self.items[1].shape[0]

    def __getitem__(self, i):
        return tuple(torch.from_numpy(a[i]) for a in self.items)


def trainer_for(z, meta, precision, dropout, opt="Adam"):
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainer, InpaintingTrainerConfig
    c = meta["config"]
    cfg = InpaintingTrainerConfig(
        model_configuration=dict(in_channels=1, out_channels=1, dropout=dropout, precision=precision),
        data_configuration=dict(clean_path=".", stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"])),
        dataloader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type=opt, args=dict(lr=LR, betas=[0.5, 0.999])), device="cuda")
    tr = InpaintingTrainer(cfg, dataset=Mem(z))
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.unet_spec(1, 1), c["seed"]).items()}
    tr.model.net.load_state_dict(wts, strict=True)
    batch = tuple(torch.from_numpy(a).cuda() for a in fixture_batch(z))
    return tr, wts, batch


def grad_errors(got, want_slices, meta_absmax):
    """per-tensor max error / max |g| on the fixture slices, cosine and norm ratio over all of them"""
    worst, dot, ng, nr = {}, 0.0, 0.0, 0.0
    for n, want in want_slices.items():
        wd = np.asarray(want, np.float64).reshape(-1)
        gd = got[n].double().cpu().numpy().reshape(-1)[: wd.size]
        worst[n] = float(np.abs(gd - wd).max() / (meta_absmax[n] + 1e-300))
        dot += float((gd * wd).sum())
        ng += float((gd * gd).sum())
        nr += float((wd * wd).sum())
    return worst, dot / np.sqrt(ng * nr), np.sqrt(ng / nr)


@pytest.mark.parametrize("name,precision", [("rst_tiny", "fp32"), ("rst_c3s", "fp32"), ("rst_tiny", "bf16"), ("rst_c3s", "bf16")])
def test_two_train_steps_match_the_reference_trainer(name, precision, record_err):
    """dropout 0: composite output, loss, every gradient, clip norm of the fused clipped Adam, weights and BatchNorm buffers
    after one and two steps, validate() loss -- against the reference's own InpaintingTrainer"""
    z, meta = load(name)
    fp32 = precision == "fp32"
    tr, wts, batch = trainer_for(z, meta, precision, 0.0)
    net = tr.model.net
    for it in (1, 2):
        loss, log = tr.train_step(batch)
        torch.cuda.synchronize()
        record_err(f"loss{it}", abs(float(loss) - meta[f"step{it}.loss"]) / meta[f"step{it}.loss"], 2e-4 if fp32 else 3e-2)
        record_err(f"clip_norm{it}", abs(float(log["grad_norm"]) - meta[f"step{it}.clip_total_norm"]) /
                   meta[f"step{it}.clip_total_norm"], 2e-3 if fp32 else 5e-2)
        if it == 1:
            record_err("output_gap", rel(gap_values(log["output"].cpu().numpy(), z["mask_frames"]), z["step1.output_gap"]),
                       2e-4 if fp32 else 5e-2)
            eng = net.engine()
            got = {n: eng.fp.gview(n) for n, _ in net.named_parameters()}
            want = {n: z["step1.grad." + n] for n in got if not is_pre_bn_bias(n)}
            for n in got:
                if is_pre_bn_bias(n):
                    assert float(got[n].abs().max()) == 0.0, n
            absmax = {n: meta["step1.grad_absmax_l2"][n][0] for n in want}
            worst, cos, ratio = grad_errors(got, want, absmax)
            top = max(worst, key=worst.get)
            print(name, precision, f"cos={cos:.7f} ratio={ratio:.5f} worst {top} {worst[top]:.2e}")
            if fp32:
                record_err("grad_worst_tensor", worst[top], 2e-2)
                record_err("grad_cos", 1 - cos, 1e-5)
            else:
                record_err("grad_cos", 1 - cos, 2e-2)
            record_err("grad_norm_ratio", abs(ratio - 1), 1e-3 if fp32 else 0.1)
        sd = net.state_dict()
        for n, v in sd.items():
            key = f"step{it}.state.{n}"
            if key not in z.files:
                assert int(v) == meta[key], n
                continue
            want_v = z[key]
            got_v = v.detach().cpu().numpy().reshape(-1)[: want_v.size]
            if "running_" in n:
                record_err(f"bn_buffers{it}", rel(got_v, want_v), 2e-4 if fp32 else 2e-2)
            elif not is_pre_bn_bias(n):
                w0 = wts[n].numpy().reshape(-1)[: want_v.size]
                d = np.abs((got_v - w0) - (want_v - w0))
                if fp32:
                    assert (d > 0.05 * LR * it + 1e-7).sum() <= max(1, 1e-2 * d.size) and np.median(d) < 2e-6, (it, n)
                else:
                    # Adam's first steps move each weight by about lr * sign(g): a bf16 gradient flips the sign of the
                    # near-zero entries, so only the bulk of the update is checked
                    assert float((d > 0.5 * LR * it).mean()) < 0.2 and np.median(d) < 0.25 * LR * it, (it, n)
    val = tr.validate([tuple(t.cpu() for t in batch)])
    assert net.training and tr.model.training
    record_err("validate", abs(val - meta["validate.loss"]) / meta["validate.loss"], 2e-4 if fp32 else 3e-2)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dropout_step_matches_the_oracle_with_the_tapped_keep_bits(precision, record_err):
    """dropout 0.2 in the differentiated pass: loss and the gradient of every tensor against the fp64 oracle fed the keep
    bits the forward drew; the bits are Bernoulli(0.8) and the next step draws new ones"""
    z, meta = load("rst_tiny")
    fp32 = precision == "fp32"
    tr, wts, batch = trainer_for(z, meta, precision, 0.2)
    net = tr.model.net
    net.dropout_tap = {}
    loss, log = tr.base_step(batch)
    tr.optimizer.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    taps = dict(net.dropout_tap)
    assert set(taps) == {"down3", "down4", "up1", "up2"}
    eng = net.engine()
    B = batch[0].shape[0]
    keep = {blk: keep_nchw(k, B, *eng.lv[level], C).double() for blk, (k, level, C) in taps.items()}
    frac = float(sum(k.sum() for k in keep.values()) / sum(k.numel() for k in keep.values()))
    assert 0.77 < frac < 0.83, frac
    P = {k: v.double() if v.is_floating_point() else v.clone() for k, v in wts.items()}
    ref_loss, ref_grads, ref_out = restorer_step(P, *[torch.from_numpy(a).double() for a in fixture_batch(z)],
                                                 keep=keep, p_drop=0.2)
    record_err("loss", abs(float(loss) - float(ref_loss)) / float(ref_loss), 1e-4 if fp32 else 3e-2)
    record_err("output", rel(log["output"].cpu(), ref_out), 2e-4 if fp32 else 5e-2)
    got = {n: p.grad for n, p in net.named_parameters()}
    assert all(g is not None for g in got.values())
    want = {n: g.numpy() for n, g in ref_grads.items() if not is_pre_bn_bias(n)}
    absmax = {n: float(np.abs(w).max()) for n, w in want.items()}
    worst, cos, ratio = grad_errors(got, want, absmax)
    top = max(worst, key=worst.get)
    print(precision, f"cos={cos:.7f} ratio={ratio:.5f} worst {top} {worst[top]:.2e}")
    if fp32:
        record_err("grad_worst_tensor", worst[top], 2e-2)
        record_err("grad_cos", 1 - cos, 1e-5)
    else:
        record_err("grad_cos", 1 - cos, 2e-2)
    record_err("grad_norm_ratio", abs(ratio - 1), 1e-3 if fp32 else 0.1)
    # the next pass draws new bits
    net.dropout_tap = {}
    tr.train_step(batch)
    torch.cuda.synchronize()
    assert not torch.equal(net.dropout_tap["down4"][0], taps["down4"][0])


def test_train_checkpoint_feeds_the_nppc_model(tmp_path):
    """train(n_steps=3) -> save_checkpoint -> NPPCModel loads it strictly; its frozen restorer reproduces the trainer's
    eval-mode output bit for bit, and an NPPC inpainting train step runs on it"""
    from nppc_audio.inpainting.nppc.nppc_model import NPPCModel, NPPCModelConfig
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer, NPPCAudioInpaintingTrainerConfig
    from nppc_audio.inpainting.utils import preprocess_data
    z, meta = load("rst_tiny")
    c = meta["config"]
    tr, _, batch = trainer_for(z, meta, "fp32", 0.2)
    hist = tr.train(n_steps=3, checkpoint_dir=str(tmp_path / "ck"), save_flag=True, val_dataloader=[tuple(t.cpu() for t in batch)])
    assert len(hist) == 3 and all(np.isfinite(hist)) and tr.step == 3 and tr.loss_history == hist
    files = sorted(os.listdir(tmp_path / "ck"))
    assert any(f.startswith("checkpoint_final_") for f in files)
    metrics = json.load(open(tmp_path / "ck" / next(f for f in files if f.startswith("metrics_final_"))))
    assert metrics["total_steps"] == 3 and metrics["training_config"]["nfft"] == c["nfft"]
    path = str(tmp_path / "restorer.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert ck["step"] == 3 and set(ck) == {"model_state_dict", "optimizer_state_dict", "step", "config"}

    rcfg = dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32")
    model = NPPCModel(NPPCModelConfig(pretrained_restoration_model_configuration=rcfg, pretrained_restoration_model_path=path,
                                      audio_pc_wrapper_configuration=dict(n_dirs=2, model_configuration=dict(
                                          in_channels=2, out_channels=2, precision="fp32")), device="cuda"))
    cn, mask4, mn = preprocess_data(batch[2], batch[0], batch[1])
    tr.model.eval()
    with torch.no_grad():
        mine = tr.model(mn, mask4)
        theirs = model.pretrained_restoration_model(mn, mask4)
    torch.cuda.synchronize()
    assert torch.equal(mine, theirs)
    tr.model.train()

    ncfg = NPPCAudioInpaintingTrainerConfig(
        nppc_model_configuration=dict(pretrained_restoration_model_configuration=rcfg, pretrained_restoration_model_path=path,
                                      audio_pc_wrapper_configuration=dict(n_dirs=2, model_configuration=dict(
                                          in_channels=2, out_channels=2, precision="fp32")), device="cuda"),
        data_configuration=dict(clean_path=".", stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"])),
        dataloader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.5, 0.999])), device="cuda")
    ntr = NPPCAudioInpaintingTrainer(ncfg, dataset=Mem(z))
    _, obj, _ = ntr.train_step(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obj))
