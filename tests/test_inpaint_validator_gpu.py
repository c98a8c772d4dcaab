"""GPU: the inpainting validator (csrc/inpaint_validator.hip and its Python surface) against torch.istft, the fp64 oracle
chain (tests/inpaint_validator_ref.py), the reference's compute_metrics fixture and the trainer's own base_step.

Limits of the transform tests are measured inside the test from the reference library's own fp32 path (torch.istft /
the fp32 torch chain on the CPU against the same computation in fp64): the kernel may err at most twice as much."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import inpaint_validator_ref as VR
from test_inpaint_gpu import build_trainer, load
from test_inpaint_validator_cpu import check_against_fixture, stacked_fixture

pytestmark = pytest.mark.gpu
CONFIGS = [(255, 128), (254, 127), (100, 25), (512, 256)]


def planes(B, n_fft, T, seed):
    g = torch.Generator().manual_seed(seed)
    F = n_fft // 2 + 1
    return torch.randn(B, F, T, generator=g), torch.randn(B, F, T, generator=g)


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- inverse STFT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_istft_any_against_torch_istft(n_fft, hop, record_err):
    from nppc_audio import ops
    for B in (1, 3):
        for T in (2, 9, 37, 500):
            re, im = planes(B, n_fft, T, 1000 * B + T + n_fft)
            nat = VR.natural_length(n_fft, hop, T)
            for kind, length in (("natural", None), ("shorter", max(1, nat - max(3, nat // 3))), ("longer", nat + n_fft + 5)):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                  # torch warns that it pads a longer length
                    ref = VR.torch_istft(re, im, n_fft, hop, length, torch.float64).numpy()
                    f32 = VR.torch_istft(re, im, n_fft, hop, length, torch.float32).numpy()
                got = ops.istft_any(re.cuda(), im.cuda(), n_fft, hop, length).cpu().numpy()     # the new kernel at every size
                assert got.shape == ref.shape == (B, nat if length is None else length)
                yard, err = relmax(f32, ref), relmax(got, ref)
                print(f"istft {n_fft}/{hop} B={B} T={T} {kind}: kernel {err:.3e}  torch fp32 {yard:.3e}")
                record_err(f"{n_fft}/{hop}/B{B}/T{T}/{kind}", err, 2 * yard)
                if kind == "natural":
                    yard_nat = yard
                if kind == "longer":
                    full = n_fft + hop * (T - 1) - n_fft // 2
                    assert np.all(got[:, full:] == 0.0) and np.all(ref[:, full:] == 0.0)
                    # torch's fp32 yardstick is loose here (its fp32 window barely resolves the last samples), so the
                    # first `nat` samples are also held to the natural-length yardstick, relative to their own peak
                    record_err(f"{n_fft}/{hop}/B{B}/T{T}/longer_head", relmax(got[:, :nat], ref[:, :nat]), 2 * yard_nat)


def test_istft_default_length_and_power_of_two_path_unchanged():
    """ops.istft keeps the radix-2 kernel where it took the configuration before; length=None is torch's default"""
    from nppc_audio import _hip as Hh
    from nppc_audio import ops
    re, im = planes(2, 512, 9, 3)
    re, im = re.cuda(), im.cuda()
    out = torch.empty(2, 2048, device="cuda")
    Hh.call("nppc_istft", re, im, out, 2, 9, 512, 256, 2048, Hh.stream())
    assert torch.equal(ops.istft(re, im, 512, 256, 2048), out)
    assert ops.istft(re, im, 512, 256).shape == (2, 2048)
    r2, i2 = planes(1, 255, 9, 4)
    assert ops.istft(r2.cuda(), i2.cuda(), 255, 128).shape == (1, 1025)
    with pytest.raises(ValueError, match="window overlap add min"):
        ops.istft_any(*(t.cuda() for t in planes(1, 100, 4, 1)), 100, 100)


@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_istft_any_is_batch_independent_repeatable_and_stays_in_bounds(n_fft, hop):
    from nppc_audio import ops
    B, T = 3, 37
    re, im = (t.cuda() for t in planes(B, n_fft, T, 7))
    a = ops.istft_any(re, im, n_fft, hop)
    assert torch.equal(a, ops.istft_any(re, im, n_fft, hop))                              # two runs
    for b in range(B):
        assert torch.equal(a[b:b + 1], ops.istft_any(re[b:b + 1], im[b:b + 1], n_fft, hop))   # alone == in the batch
    # a length shorter than the natural one by more than n_fft: frames that cannot reach a kept sample are never summed,
    # and nothing past `length` is written
    nat = VR.natural_length(n_fft, hop, T)
    L = nat - n_fft - 50
    assert L > 0
    dead = torch.arange(T) * hop >= L + n_fft // 2
    assert int(dead.sum()) >= 1
    r0, i0 = re.clone(), im.clone()
    r0[:, :, dead.cuda()] = 0.0
    i0[:, :, dead.cuda()] = 0.0
    r1, i1 = re.clone(), im.clone()
    r1[:, :, dead.cuda()] = 3e38
    i1[:, :, dead.cuda()] = 3e38
    buf = torch.full((B, L + 300), 123.0, device="cuda")
    got = ops.istft_any(r1, i1, n_fft, hop, L, out=buf)
    want = ops.istft_any(r0, i0, n_fft, hop, L)
    assert bool(torch.isfinite(got[:, :L]).all()) and torch.equal(got[:, :L], want)
    assert bool((buf[:, L:] == 123.0).all())
    ref = VR.torch_istft(re.cpu(), im.cpu(), n_fft, hop, L).numpy()
    f32 = VR.torch_istft(re.cpu(), im.cpu(), n_fft, hop, L, torch.float32).numpy()
    assert relmax(want.cpu().numpy(), ref) < 2 * relmax(f32, ref)


# ---- PC audio variations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("n_fft,hop,T", [(255, 128, 37), (254, 127, 9), (512, 256, 9)])
def test_pc_variations_against_the_oracle_chain(K, n_fft, hop, T, record_err):
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas, pc_audio_variations
    B, F = 2, n_fft // 2 + 1
    g = torch.Generator().manual_seed(100 * K + T)
    # |normalised log-magnitude| <= 4 for every alpha in [-3, 3] and std <= 3: exp stays finite in the fp32 chain
    pred = (torch.rand(B, 1, F, T, generator=g) * 2 - 1) * 2.0
    pc = (torch.rand(B, K, F, T, generator=g) * 2 - 1) * 0.6
    clean_norm = (torch.rand(B, 1, F, T, generator=g) * 2 - 1) * 4.0
    clean_spec = torch.randn(B, 2, F, T, generator=g)
    zero = torch.rand(B, 1, F, T, generator=g) < 0.05
    # some bins exactly zero: the product leaves +0 or -0 by the sign of the value it wipes, so both of torch.angle's
    # zero cases occur (angle(0 + 0i) = 0, and atan2's +-pi for a real part of -0)
    clean_spec = clean_spec * (~zero)
    assert bool(((clean_spec[:, 0] == 0) & ~torch.signbit(clean_spec[:, 0])).any()) and bool(((clean_spec[:, 0] == 0) & torch.signbit(clean_spec[:, 0])).any())
    assert int(zero.sum()) > 0 and bool((clean_spec[:, 0][zero[:, 0]] == 0).all())
    mean, std = torch.tensor(-1.0), torch.tensor(2.5)
    alphas = default_alphas()
    assert float((pred.abs() + 3 * pc.abs().amax(1, keepdim=True)).max()) <= 4.0
    ref_v, ref_c = VR.pc_variation_chain(clean_norm, pred, pc, clean_spec, alphas, mean, std, n_fft, hop, torch.float64)
    f32_v, f32_c = VR.pc_variation_chain(clean_norm, pred, pc, clean_spec, alphas, mean, std, n_fft, hop, torch.float32)
    assert bool(torch.isfinite(f32_v).all()) and bool(torch.isfinite(f32_c).all()) and bool(torch.isfinite(ref_v).all())
    got_v, got_c = pc_audio_variations(clean_norm.cuda(), pred.cuda(), pc.cuda(), clean_spec.cuda(), alphas, mean.cuda(),
                                       std.cuda(), n_fft=n_fft, hop_length=hop)
    assert got_v.shape == ref_v.shape == (B, K, 13, VR.natural_length(n_fft, hop, T)) and got_c.shape == ref_c.shape

    def worst(x, ref):                                                 # per waveform, relative to its own peak
        d = (x.double() - ref).abs().amax(-1) / ref.abs().amax(-1)
        return float(d.max())

    ev, yv = worst(got_v.cpu(), ref_v), worst(f32_v, ref_v)
    ec, yc = worst(got_c.cpu(), ref_c), worst(f32_c, ref_c)
    print(f"variations K={K} {n_fft}/{hop}: kernel {ev:.3e} (fp32 chain {yv:.3e}); clean {ec:.3e} (fp32 chain {yc:.3e})")
    record_err("variations", ev, 2 * yv)
    record_err("clean", ec, 2 * yc)
    # determinism: two runs, and an item alone
    again_v, again_c = pc_audio_variations(clean_norm.cuda(), pred.cuda(), pc.cuda(), clean_spec.cuda(), alphas, mean.cuda(),
                                           std.cuda(), n_fft=n_fft, hop_length=hop)
    assert torch.equal(again_v, got_v) and torch.equal(again_c, got_c)
    one_v, one_c = pc_audio_variations(clean_norm[1:].cuda(), pred[1:].cuda(), pc[1:].cuda(), clean_spec[1:].cuda(), alphas,
                                       mean.cuda(), std.cuda(), n_fft=n_fft, hop_length=hop)
    assert torch.equal(one_v[0], got_v[1]) and torch.equal(one_c[0], got_c[1])


# ---- batched metrics -----------------------------------------------------------------------------------------------------------
def scalars(m):
    return np.array([m["nppc"]["rmse"], m["nppc"]["residual_error"], m["mc_dropout"]["rmse"], m["mc_dropout"]["residual_error"]])


def test_compute_metrics_batch_on_the_stacked_reference_fixture():
    from nppc_audio.inpainting.mc_baseline import compute_metrics_batch
    z, t, n = stacked_fixture()
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    ms = compute_metrics_batch(d["nppc"].view(2, n, 32, 40), d["mc"].view(2, n, 32, 40), d["pred"].view(2, 1, 32, 40),
                               d["mean"].view(2, 1, 32, 40), d["clean"].view(2, 1, 32, 40), d["mask"].view(2, 1, 32, 40))
    assert len(ms) == 2
    for case, m in zip("ab", ms):
        check_against_fixture(z, case, m)


@pytest.mark.parametrize("B,n,Fq,T", [(1, 1, 32, 41), (2, 1, 32, 41), (4, 1, 32, 41), (1, 5, 32, 41), (2, 5, 32, 41), (4, 5, 32, 41),
                                      # the C3 shape: N = 64000 >= 8192, where compute_metrics folds 8 chunks per pair with
                                      # atomics and the batched kernel one strided sum per thread (different orders)
                                      (2, 5, 128, 500), (1, 1, 128, 500)])
def test_compute_metrics_batch_against_compute_metrics_item_by_item(B, n, Fq, T, record_err):
    from nppc_audio.inpainting import mc_baseline as MB
    g = torch.Generator().manual_seed(10 * B + n)
    nppc = torch.randn(B, n, Fq, T, generator=g) * torch.rand(B, n, 1, 1, generator=g) * 3
    mc = torch.randn(B, n, Fq, T, generator=g) + 0.7 * nppc
    clean = torch.randn(B, 1, Fq, T, generator=g)
    pred = clean + 0.3 * torch.randn(B, 1, Fq, T, generator=g) + 0.2 * nppc[:, :1]
    mean = clean + 0.4 * torch.randn(B, 1, Fq, T, generator=g)
    mask = torch.ones(B, 1, Fq, T)
    for b in range(B):
        mask[b, :, :, 5 + 3 * b:12 + 3 * b] = 0
    dev = [t.cuda() for t in (nppc, mc, pred, mean, clean, mask)]
    ms = MB.compute_metrics_batch(*dev)
    G = MB.metrics_gram_batch(*dev)
    assert torch.equal(G, MB.metrics_gram_batch(*dev))                               # two runs
    assert torch.equal(G, G.transpose(1, 2))
    rows = np.stack([VR.gram(VR.metric_rows(*(t[b:b + 1].numpy() for t in (nppc, mc, pred, mean, clean, mask)))) for b in range(B)])
    record_err("gram_vs_numpy_fp64", np.abs(G.cpu().numpy() - rows).max() / np.abs(rows).max(), 1e-12)
    for b in range(B):
        one = MB.compute_metrics(*(t[b:b + 1] for t in dev))
        assert torch.equal(MB.metrics_gram_batch(*(t[b:b + 1] for t in dev))[0], G[b])   # alone == in the batch, bit for bit
        record_err(f"scalars_b{b}", np.abs(scalars(ms[b]) - scalars(one)).max(), 2e-6 * scalars(one).max())
        record_err(f"angles_b{b}", np.abs(np.array(ms[b]["principal_angles"]) - np.array(one["principal_angles"])).max(), 1e-3)


# ---- trainer.validate ----------------------------------------------------------------------------------------------------------
def held_out(z, shift):
    """held-out batches from the fixture's clean spectrograms: rolled in time, a fresh 6-frame gap in every item"""
    clean = torch.from_numpy(np.roll(z["clean_spec"], shift, axis=-1).copy())
    B, _, _, T = clean.shape
    mask = torch.ones(B, T)
    for b in range(B):
        mask[b, 4 + 5 * b + shift:10 + 5 * b + shift] = 0
    return clean * mask[:, None, None, :], mask, clean


def state_snapshot(tr):
    snap = {"sd." + k: v.detach().clone() for k, v in tr.nppc_model.state_dict().items()}
    for i, (p, st) in enumerate(tr.optimizer.state.items()):
        for k, v in st.items():
            if torch.is_tensor(v):
                snap[f"opt.{i}.{k}"] = v.detach().clone()
    return snap


def test_validate_equals_mean_base_step_and_leaves_no_trace(tmp_path):
    z, meta = load("inp_tiny")
    tr, _, batch = build_trainer(meta, "fp32", tmp_path, z)
    tr.train_step(batch)                                            # Adam state and moved BatchNorm buffers exist
    five = lambda b: (*b, torch.zeros(3, 1, 8), [{"i": 0}])        # the five-tuple of the reference's collate_fn
    loader = [held_out(z, 1), five(held_out(z, 3))]
    before = state_snapshot(tr)
    flags = {n: m.training for n, m in tr.nppc_model.named_modules()}
    assert tr.nppc_model.pc_wrapper.training and not tr.nppc_model.pretrained_restoration_model.training
    avg_obj, avg_rec = tr.validate(loader)
    after = state_snapshot(tr)
    assert set(before) == set(after) and any(k.endswith("running_mean") for k in before) and any(k.startswith("opt.") for k in before)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert flags == {n: m.training for n, m in tr.nppc_model.named_modules()}
    # the test's own computation of the same means
    tr.nppc_model.eval()
    objs, recs = [], []
    with torch.no_grad():
        for b in loader:
            rec, obj, _ = tr.base_step(tuple(t.cuda() for t in b[:3]))
            objs.append(obj.item())
            recs.append(rec.mean().item())
    tr.nppc_model.train()
    assert isinstance(avg_obj, float) and isinstance(avg_rec, float)
    assert avg_obj == sum(objs) / 2 and avg_rec == sum(recs) / 2
    with pytest.raises(ValueError, match="no batches"):
        tr.validate([])


def test_train_with_a_validation_loader_keeps_history_and_the_trajectory(tmp_path, record_err):
    z, meta = load("inp_tiny")
    loader = [held_out(z, 1), held_out(z, 3)]

    def run(val):
        torch.manual_seed(0)
        tr, _, _ = build_trainer(meta, "fp32", tmp_path, z)
        tr.config.log_interval = 2
        tr.train(n_steps=4, checkpoint_dir=str(tmp_path / "ck"), save_flag=False, val_dataloader=val)
        return tr, torch.cat([p.detach().reshape(-1) for p in tr.nppc_model.pc_wrapper.parameters()]).double().cpu()

    tr0, w0 = run(None)
    tr1, w1 = run(None)
    trv, wv = run(loader)
    assert tr0.val_loss_history == [] and tr0.val_reconst_err_history == [] and tr0.step == 4
    assert len(trv.val_loss_history) == 2 and len(trv.val_reconst_err_history) == 2 and trv.step == 4
    assert all(np.isfinite(v) for v in trv.val_loss_history + trv.val_reconst_err_history)
    noise = float((w0 - w1).abs().max())
    diff = float((wv - w0).abs().max())
    print(f"weights after 4 steps: run-to-run {noise:.3e}, with validation {diff:.3e}")
    record_err("trajectory", diff, np.nextafter(noise, np.inf))                      # diff <= noise


# ---- NPPCModelValidator ----------------------------------------------------------------------------------------------------------
def test_validator_end_to_end_on_the_tiny_fixture(tmp_path):
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    z, meta = load("inp_tiny")
    c = meta["config"]
    tr, _, _ = build_trainer(meta, "fp32", tmp_path, z)
    ck = str(tmp_path / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    cfg = V.NPPCModelValidatorConfig(checkpoint_path=ck, save_dir=str(tmp_path / "val"),
                                     model_configuration=tr.config.nppc_model_configuration.model_dump())
    val = V.NPPCModelValidator(cfg)
    assert not val.model.training and not val.model.pretrained_restoration_model.training
    for k, v in tr.nppc_model.state_dict().items():
        assert torch.equal(v.cpu(), val.model.state_dict()[k].cpu()), k
    b1, b2 = held_out(z, 1), held_out(z, 3)
    net = val.model.pretrained_restoration_model.net
    kw = dict(n_mc_samples=8, n_components=c["K"])
    net.dropout_pass = 0
    res = val.validate_dataloader([b1, (*b2, None, None)], save=True, **kw)
    net.dropout_pass = 0
    r1 = val.validate_batch(*b1, **kw)
    r2 = val.validate_batch(*b2, alphas=V.default_alphas(), n_fft=c["nfft"], hop_length=c["hop"], **kw)
    assert not any(m.training for m in val.model.modules())
    items = r1["metrics"] + r2["metrics"]
    assert res["n_items"] == 6 == len(res["per_item"])
    for got, want in zip(res["per_item"], items):
        assert np.abs(scalars(got) - scalars(want)).max() < 2e-6 * scalars(want).max()
        assert np.abs(np.array(got["principal_angles"]) - np.array(want["principal_angles"])).max() < 1e-3
        assert len(got["principal_angles"]) == c["K"] and all(np.isfinite(scalars(got)))
    assert abs(res["mean"]["nppc"]["rmse"] - np.mean([m["nppc"]["rmse"] for m in res["per_item"]])) < 1e-12
    B, K, T = 3, c["K"], c["T"]
    L = VR.natural_length(c["nfft"], c["hop"], T)
    assert r2["audio_variations"].shape == (B, K, 13, L) and r2["clean_audio"].shape == (B, L)
    assert bool(torch.isfinite(r2["audio_variations"]).all()) and "audio_variations" not in r1
    assert r2["pc_directions"].shape == (B, K, 32, T) and r2["mc_dropout"]["scaled_principal_components"].shape == (B, K, 32, T)
    # alpha = 0 is the restored clip itself: the oracle chain on the validator's own tensors
    ref_v, ref_c = VR.pc_variation_chain(r2["clean_spec_mag_norm"].cpu(), r2["pred_spec_mag_norm"].cpu(), r2["pc_directions"].cpu(),
                                         b2[2], V.default_alphas(), r2["mean"].cpu(), r2["std"].cpu(), c["nfft"], c["hop"],
                                         torch.float64)
    assert relmax(r2["audio_variations"].cpu().numpy(), ref_v.numpy()) < 1e-5
    assert relmax(r2["clean_audio"].cpu().numpy(), ref_c.numpy()) < 1e-5
    for i in range(6):
        js = json.load(open(tmp_path / "val" / "validation_metrics" / f"sample_{i}.json"))
        assert set(js) == {"nppc", "mc_dropout", "principal_angles"}
        assert set(js["nppc"]) == set(js["mc_dropout"]) == {"rmse", "residual_error"}
    with pytest.raises(ValueError, match="no batches"):
        val.validate_dataloader([])
    with pytest.raises(ValueError, match="same number of masked"):
        bad = b1[1].clone()
        bad[0, 0] = 0
        val.validate_batch(b1[0], bad, b1[2], **kw)
