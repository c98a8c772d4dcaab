"""GPU: the ragged-gap MC-dropout + PCA baseline (csrc/mc_pca_ragged.hip, csrc/mc_pca.hip through nppc_audio.inpainting.mc_baseline) against
torch's own indexing, the fp64 restatement (tests/mc_ragged_ref.py), its bit-for-bit contract (an item in a batch == the
item alone; two runs agree), the uniform path, and through NPPCModelValidator / NPPCAudioInpaintingTrainer.base_step2 with
`ragged_gaps=True` on a batch of 5-, 6- and 6-frame gaps, which the uniform path refuses."""
import os

import numpy as np
import pytest
import torch

import mc_ragged_ref as R
from oracle import weights as W
from test_mc_ragged_cpu import separated_stack

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 130]                    # around the Gram chunk of 64 elements: 1, 1, 1, 2 and 3 chunks
KN = [(2, 1), (7, 5), (60, 8)]


def masks_8x21():
    """one frame; three frames in two runs; a non-column mask; all but one element"""
    g = torch.Generator().manual_seed(0)
    m = torch.ones(4, 8, 21)
    m[0, :, 4] = 0
    m[1, :, 2:4] = 0
    m[1, :, 17] = 0
    m[2] = (torch.rand(8, 21, generator=g) > 0.3).float()
    m[3] = 0
    m[3, 5, 11] = 1
    return m


def test_index_gather_scatter_equal_torch_indexing():
    from nppc_audio.inpainting import mc_baseline as MB
    B, F, T = 4, 8, 21
    mask = masks_8x21()
    hole = mask.reshape(B, F * T) == 0
    want_counts = hole.sum(1).tolist()
    assert want_counts[0] == 8 and want_counts[1] == 24 and want_counts[3] == F * T - 1
    idx, counts = MB.gap_index(mask.cuda())
    Nmax = max(want_counts)
    assert idx.dtype == torch.int32 and counts.dtype == torch.int32 and idx.shape == (B, Nmax)
    assert counts.tolist() == want_counts
    ref_idx, _ = R.gap_index(mask.numpy())
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    g = torch.Generator().manual_seed(1)
    pred = torch.randn(B, 1, F, T, generator=g)
    stack = MB.gather_gap(pred.cuda(), idx).cpu()
    vals3 = torch.randn(B, 3, Nmax, generator=g)
    full2 = MB.scatter_gap_ragged(stack.cuda(), idx, F, T).cpu()
    full3 = MB.scatter_gap_ragged(vals3.cuda(), idx, F, T).cpu()
    assert full2.shape == (B, F, T) and full3.shape == (B, 3, F, T)
    for b in range(B):
        c = want_counts[b]
        assert torch.equal(idx[b, :c].cpu().long(), torch.nonzero(hole[b])[:, 0]) and bool((idx[b, c:] == -1).all())
        assert torch.equal(stack[b, :c], pred.reshape(B, F * T)[b][hole[b]]) and bool((stack[b, c:] == 0).all())
        want2 = torch.zeros(F * T).masked_scatter_(hole[b], stack[b, :c])
        assert torch.equal(full2[b].reshape(-1), want2)
        want3 = torch.zeros(3, F * T).masked_scatter_(hole[b][None].expand(3, -1), vals3[b, :, :c].contiguous())
        assert torch.equal(full3[b].reshape(3, -1), want3)
    # a frame mask [B, T] expanded over F, as the validator passes it, and more than one 256-element tile per item
    fm = torch.ones(2, 1, 32, 48)
    fm[0, :, :, 7:12] = 0
    fm[1, :, :, 40:46] = 0
    idx, counts = MB.gap_index(fm.cuda())
    assert counts.tolist() == [160, 192]
    for b in range(2):
        want = torch.nonzero(fm[b].reshape(-1) == 0)[:, 0]
        assert torch.equal(idx[b, :len(want)].cpu().long(), want) and bool((idx[b, len(want):] == -1).all())


@pytest.fixture(scope="module")
def ragged_stacks():
    """per (K, n): a padded stack over COUNTS with well-separated singular values, and its fp64 restatement (computed once)"""
    out = {}
    for K, n in KN:
        rng = np.random.default_rng(100 * K + n)
        stack = np.zeros((K, len(COUNTS), max(COUNTS)), dtype=np.float32)
        for b, c in enumerate(COUNTS):
            stack[:, b, :c] = separated_stack(rng, K, c)
        out[(K, n)] = (stack, R.pca_ragged(stack, COUNTS, n))
    return out


@pytest.mark.parametrize("K,n", KN)
def test_ragged_pca_against_fp64_restatement_and_bit_for_bit_contract(K, n, ragged_stacks, record_err):
    """every component of every item against the restatement at compute_pca_batch's own tolerances (5e-6 on components,
    1e-6 relative on singular values).  The one-element item has a single singular pair: its further components have
    singular value 0 and therefore no direction, so for them the singular value and scaled = component x singular value
    are compared (both 0), not the direction."""
    from nppc_audio.inpainting import mc_baseline as MB
    stack, want = ragged_stacks[(K, n)]
    dev = torch.from_numpy(stack).cuda()
    counts = torch.tensor(COUNTS, dtype=torch.int32).cuda()
    got = MB.compute_pca_ragged(dev, counts, n)
    comps, scaled, weights, mean, svals = (t.cpu().numpy().astype(np.float64) for t in got)
    smax = want[4].max()
    for b, c in enumerate(COUNTS):
        m = n if c > 1 else 1
        record_err(f"comps_b{b}", np.abs(comps[b, :m] - want[0][b, :m]).max(), 5e-6)
        record_err(f"scaled_b{b}", np.abs(scaled[b] - want[1][b]).max(), 5e-6 * smax)
        record_err(f"svals_b{b}", np.abs(svals[b] - want[4][b]).max(), 1e-6 * smax)
        record_err(f"weights_b{b}", np.abs(weights[b, :m] - want[2][b, :m]).max(), 1e-6)
        assert np.array_equal(mean[b], want[3][b].astype(np.float64))            # fp64 sum rounded once: the same fp32 number
        assert np.all(comps[b, :, c:] == 0) and np.all(scaled[b, :, c:] == 0) and np.all(mean[b, c:] == 0)
    # contract: two runs agree bit for bit, and item b of the batch is the same call on that item alone
    again = MB.compute_pca_ragged(dev, counts, n)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)
    for b, c in enumerate(COUNTS):
        one = MB.compute_pca_ragged(dev[:, b:b + 1, :c].contiguous(), [c], n)
        assert torch.equal(one[0][0], got[0][b, :, :c]) and torch.equal(one[1][0], got[1][b, :, :c])
        assert torch.equal(one[2][0], got[2][b]) and torch.equal(one[3][0], got[3][b, :c]) and torch.equal(one[4][0], got[4][b])
    # host counts (list / CPU tensor) are the same call
    assert torch.equal(MB.compute_pca_ragged(dev, COUNTS, n)[0], got[0])


@pytest.mark.parametrize("K,n", KN)
def test_ragged_pca_agrees_with_the_uniform_path_on_a_uniform_batch(K, n, record_err):
    """the uniform path sums its Gram with atomics, so agreement is to the tolerances, not bit for bit"""
    from nppc_audio.inpainting import mc_baseline as MB
    rng = np.random.default_rng(7 * K + n)
    B, D = 3, 130
    x = torch.from_numpy(np.stack([separated_stack(rng, K, D) for _ in range(B)], axis=1)).cuda()
    uni = MB.compute_pca_batch(x, n)
    rag = MB.compute_pca_ragged(x, [D] * B, n)
    smax = float(uni[4].max())
    record_err("comps", float((rag[0] - uni[0]).abs().max()), 5e-6)
    record_err("scaled", float((rag[1] - uni[1]).abs().max()), 5e-6 * smax)
    record_err("weights", float((rag[2] - uni[2]).abs().max()), 1e-6)
    assert torch.equal(rag[3], uni[3])                                           # the mean is the same sum in the same order
    record_err("svals", float((rag[4] - uni[4]).abs().max()), 1e-6 * smax)
    with pytest.raises(RuntimeError, match="unsupported"):
        MB.compute_pca_ragged(torch.zeros(61, 1, 8).cuda(), [8], 3)


def _dropout_unet(precision, seed=0):
    from nppc_audio.inpainting.networks.unet import RestorationWrapper, UNet, UNetConfig
    spec = W.unet_spec(1, 1)
    wts = {k: torch.from_numpy(v) for k, v in W.make_weights(spec, 21).items()}
    net = UNet(UNetConfig(in_channels=1, out_channels=1, dropout=0.2, precision=precision))
    net.load_state_dict(wts, strict=True)
    net.dropout_seed = 1234 + seed
    return RestorationWrapper(net).cuda().eval(), wts


GAPS = ((4, 5), (15, 6), (30, 6))                # (first gap frame, frames) per item: 5, 6 and 6 frames


def frame_mask(B, T, gaps=GAPS):
    m = torch.ones(B, T)
    for b, (s, w) in enumerate(gaps):
        m[b, s:s + w] = 0
    return m


def test_calculate_unet_baseline_ragged_end_to_end():
    """shapes, support on each item's own gap, and every item against calculate_unet_baseline on that item's gap alone with
    the same dropout passes.  The keep bits of a pass are a function of the item's rows in the batch, so "alone" keeps the
    item in its slot and gives the other slots the same gap (the uniform path then accepts the batch; in eval mode an
    item's output does not depend on the other items); item 0 is also run literally alone (B = 1).  Tolerances of
    test_calculate_unet_baseline_end_to_end."""
    from nppc_audio.inpainting import mc_baseline as MB
    B, Fq, T, K, n = 3, 32, 48, 6, 5
    model, _ = _dropout_unet("fp32", seed=5)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 1, Fq, T, generator=g).cuda()
    mask = frame_mask(B, T)[:, None, None, :].expand(B, 1, Fq, T).contiguous().cuda()
    with pytest.raises(ValueError, match="same number of masked"):
        MB.calculate_unet_baseline(model, x, mask, n_mc_samples=2, n_components=n)
    net = model.net
    net.dropout_pass = 0
    out = MB.calculate_unet_baseline_ragged(model, x, mask, n_mc_samples=K, n_components=n)
    assert net.dropout_pass == K
    assert out["mean_prediction"].shape == (B, 1, Fq, T) and out["principal_components"].shape == (B, n, Fq, T)
    assert out["scaled_principal_components"].shape == (B, n, Fq, T)
    assert out["singular_vals"].shape == (B, n) and out["importance_weights"].shape == (B, n)
    known = mask.bool().expand(-1, n, -1, -1)
    assert float(out["principal_components"][known].abs().max()) == 0.0
    assert float(out["scaled_principal_components"][known].abs().max()) == 0.0
    assert float(out["mean_prediction"][mask.bool()].abs().max()) == 0.0
    assert float(out["principal_components"][~known].abs().max()) > 0.0
    assert torch.allclose(out["importance_weights"].sum(1), torch.ones(B, device="cuda"), atol=1e-5)
    # the stack of the ragged sampler is the boolean-indexed stack, pass by pass
    net.dropout_pass = 0
    stack, idx, counts = MB.mc_dropout_samples_ragged(model, x, mask, K)
    assert counts.tolist() == [w * Fq for _, w in GAPS] and stack.shape == (K, B, 6 * Fq)
    for b in range(B):
        own = mask[b:b + 1].expand(B, -1, -1, -1).contiguous()                # every slot gets item b's gap
        net.dropout_pass = 0
        preds, hole = MB.mc_dropout_samples(model, x, own, K)
        assert torch.equal(preds[:, b], stack[:, b, :int(counts[b])])
        net.dropout_pass = 0
        alone = MB.calculate_unet_baseline(model, x, own, n_mc_samples=K, n_components=n)
        smax = float(alone["singular_vals"][b].max())
        assert float((out["principal_components"][b] - alone["principal_components"][b]).abs().max()) < 2e-4
        assert float((out["singular_vals"][b] - alone["singular_vals"][b]).abs().max()) < 1e-4 * smax
        assert float((out["mean_prediction"][b] - alone["mean_prediction"][b]).abs().max()) < 1e-5
    net.dropout_pass = 0
    first = MB.calculate_unet_baseline(model, x[:1], mask[:1], n_mc_samples=K, n_components=n)
    assert float((out["principal_components"][0] - first["principal_components"][0]).abs().max()) < 2e-4
    assert float((out["singular_vals"][0] - first["singular_vals"][0]).abs().max()) < 1e-4 * float(first["singular_vals"].max())
    assert float((out["mean_prediction"][0] - first["mean_prediction"][0]).abs().max()) < 1e-5
    # two runs of the same passes agree bit for bit
    net.dropout_pass = 0
    again = MB.calculate_unet_baseline_ragged(model, x, mask, n_mc_samples=K, n_components=n)
    for k in out:
        assert torch.equal(out[k], again[k]), k


# ---- the public surface: validator and base_step2 ----------------------------------------------------------------------
NFFT, HOP, FQ, T48, KDIR = 63, 32, 32, 48, 3


@pytest.fixture(scope="module")
def trainer_and_batches(tmp_path_factory):
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer, NPPCAudioInpaintingTrainerConfig
    tmp = tmp_path_factory.mktemp("mc_ragged")
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(KDIR), 41).items()}
    pre = "pretrained_restoration_model.net."
    ck = os.path.join(str(tmp), "restorer.pt")
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    cfg = NPPCAudioInpaintingTrainerConfig(
        nppc_model_configuration=dict(
            pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
            pretrained_restoration_model_path=ck,
            audio_pc_wrapper_configuration=dict(n_dirs=KDIR, model_configuration=dict(in_channels=2, out_channels=KDIR,
                                                                                      precision="fp32")),
            device="cuda"),
        data_configuration=dict(clean_path=".", stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT)),
        dataloader_configuration=dict(batch_size=3, num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.5, 0.999])), device="cuda")

    class Empty(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, i):
            raise IndexError

    tr = NPPCAudioInpaintingTrainer(cfg, dataset=Empty())
    tr.nppc_model.load_state_dict(wts, strict=True)
    tr.nppc_model.to("cuda")
    g = torch.Generator().manual_seed(11)
    clean = torch.randn(3, 2, FQ, T48, generator=g)

    def batch(gaps):
        m = frame_mask(3, T48, gaps)
        return clean * m[:, None, None, :], m, clean

    return tr, batch(GAPS), batch(((4, 6), (15, 6), (30, 6))), tmp


def scalars(m):
    return np.array([m["nppc"]["rmse"], m["nppc"]["residual_error"], m["mc_dropout"]["rmse"], m["mc_dropout"]["residual_error"]])


def test_validator_with_ragged_gaps(trainer_and_batches):
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    tr, ragged, uniform, tmp = trainer_and_batches
    ck = str(tmp / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    val = V.NPPCModelValidator(V.NPPCModelValidatorConfig(
        checkpoint_path=ck, save_dir=None, model_configuration=tr.config.nppc_model_configuration.model_dump()))
    net = val.model.pretrained_restoration_model.net
    kw = dict(n_mc_samples=6, n_components=KDIR)
    with pytest.raises(ValueError, match="same number of masked"):              # the default is what it was
        val.validate_batch(*ragged, **kw)
    with pytest.raises(ValueError, match="same number of masked"):
        val.validate_batch(*ragged, ragged_gaps=False, **kw)
    with pytest.raises(ValueError, match="same number of masked"):
        val.validate_dataloader([ragged], **kw)
    net.dropout_pass = 0
    out = val.validate_batch(*ragged, ragged_gaps=True, alphas=V.default_alphas(), n_fft=NFFT, hop_length=HOP, **kw)
    net.dropout_pass = 0
    uni = val.validate_batch(*uniform, alphas=V.default_alphas(), n_fft=NFFT, hop_length=HOP, **kw)
    assert not any(m.training for m in val.model.modules())
    assert set(out) == set(uni) and set(out["mc_dropout"]) == set(uni["mc_dropout"])
    for k in ("pc_directions", "pred_spec_mag_norm", "clean_spec_mag_norm", "mask", "audio_variations", "clean_audio"):
        assert out[k].shape == uni[k].shape and bool(torch.isfinite(out[k]).all()), k
    for k, v in out["mc_dropout"].items():
        assert v.shape == uni["mc_dropout"][k].shape and bool(torch.isfinite(v).all()), k
    known = out["mask"].bool()
    assert float(out["mc_dropout"]["scaled_principal_components"][known.expand(-1, KDIR, -1, -1)].abs().max()) == 0.0
    assert float(out["mc_dropout"]["mean_prediction"][known].abs().max()) == 0.0
    assert (out["mask"] == 0).flatten(1).sum(1).tolist() == [w * FQ for _, w in GAPS]
    assert len(out["metrics"]) == 3
    for m in out["metrics"]:
        assert all(np.isfinite(scalars(m))) and len(m["principal_angles"]) == KDIR and m["mc_dropout"]["rmse"] > 0
    # on a uniform batch the keyword changes nothing beyond the summation order of the Gram
    net.dropout_pass = 0
    uni_r = val.validate_batch(*uniform, ragged_gaps=True, **kw)
    smax = float(uni["mc_dropout"]["singular_vals"].max())
    assert float((uni_r["mc_dropout"]["singular_vals"] - uni["mc_dropout"]["singular_vals"]).abs().max()) < 1e-6 * smax
    assert float((uni_r["mc_dropout"]["scaled_principal_components"]
                  - uni["mc_dropout"]["scaled_principal_components"]).abs().max()) < 5e-6 * smax
    assert torch.equal(uni_r["mc_dropout"]["mean_prediction"], uni["mc_dropout"]["mean_prediction"])
    # the loader path: the same items, the same numbers.  The loader's second batch draws the dropout passes that follow
    # the first batch's, so its per-batch counterpart replays from there, not from pass 0
    net.dropout_pass = 0
    res = val.validate_dataloader([ragged, (*uniform, None, None)], ragged_gaps=True, **kw)
    assert res["n_items"] == 6 and net.dropout_pass == 2 * kw["n_mc_samples"]
    net.dropout_pass = kw["n_mc_samples"]
    second = val.validate_batch(*uniform, ragged_gaps=True, **kw)
    for got, want in zip(res["per_item"], out["metrics"] + second["metrics"]):
        assert np.abs(scalars(got) - scalars(want)).max() < 2e-6 * scalars(want).max()
        assert np.abs(np.array(got["principal_angles"]) - np.array(want["principal_angles"])).max() < 1e-3


def test_base_step2_with_ragged_gaps(trainer_and_batches):
    tr, ragged, uniform, _ = trainer_and_batches
    ragged, uniform = (tuple(t.cuda() for t in b) for b in (ragged, uniform))
    tr.step = 500
    with pytest.raises(ValueError, match="same number of masked"):              # the default is what it was
        tr.base_step2(ragged, n_mc_samples=6)
    with pytest.raises(ValueError, match="same number of masked"):
        tr.base_step2(ragged, n_mc_samples=6, ragged_gaps=False)
    net = tr.nppc_model.pretrained_restoration_model.net
    assert not net.training and not any(m.training for m in net.modules())
    _, _, log_u = tr.base_step2(uniform, n_mc_samples=6)
    rec, obj, log = tr.base_step2(ragged, n_mc_samples=6, ragged_gaps=True)
    tr.nppc_model.zero_grad()
    obj.backward()
    torch.cuda.synchronize()
    assert set(log) == set(log_u)
    for k in log:
        assert log[k].shape == log_u[k].shape and bool(torch.isfinite(log[k]).all()), k
    assert torch.isfinite(obj) and float(rec.min()) > -1e-5 and float(rec.max()) < 1 + 1e-5
    grad = tr.nppc_model.pc_wrapper.net.engine().fp.grad
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    assert not net.training and not any(m.training for m in net.modules())
    # the w_mc rows are the scaled components of each item's own gap: non-zero, and zero on the known frames
    assert float(log["w_mc"].flatten(2).norm(dim=2).min()) > 0
    known = ragged[1].bool()[:, None, None, :].expand_as(log["w_mc"])
    assert float(log["w_mc"][known].abs().max()) == 0.0
