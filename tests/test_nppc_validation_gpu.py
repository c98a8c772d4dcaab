"""GPU: held-out validation of the speech-enhancement NPPC step in ragged batches: the ragged forward of the
direction net, the ragged Gram-Schmidt / loss kernels of csrc/nppc_ragged.hip, nppc_base_step(lengths=),
NPPCAudioTrainer.validate and train(val_dataloader=).  Every item of every batch is compared with the same clip run alone;
padding is never read; outputs past an item's end are 0."""
import glob
import json

import numpy as np
import pytest
import torch

import gsloss_ref as GR
from golden_util import load, rel
from nppc_validation_ref import (LENGTHS, ORACLE_FP32_FLOOR, build_model, clips, direction_scores_np, model_config,
                                 oracle_step_alone, padded)
from oracle import nppc_ref as R

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
U24 = 2.0 ** -24
# w_mat against the CPU oracle: tests/test_train_step_gpu.py::test_train_step_matches_oracle (5e-4 in fp32, W_MAT_BF16_TOL there)
W_MAT_ORACLE_LIMIT = {"fp32": 5e-4, "bf16": 1.5e-1}
# w_mat of an item in a batch against the same clip alone: 2 x the worst measured on the MI355X
# (profiles/nppc_validation_parity_errors.json, DESIGN.md §7g: fp32 1.65e-6, bf16 3.49e-3; the factor covers bf16
# roundings that flip with the summation order of the GroupNorm / laplace sums, as in tests/test_ragged_inference_gpu.py)
W_MAT_ALONE_LIMIT = {"fp32": 3.3e-6, "bf16": 7.0e-3}
# loss scalars against the fp64 oracle on the clip alone, fp32: tests/test_train_step_gpu.py::test_train_step_matches_oracle
# (reconst_err) and ::test_long_clip_reference_golden (the other per-item terms)
RECONST_LIMIT_FP32 = 1e-4
LOSS_TERM_LIMIT_FP32 = 5e-4
BF16_LOSS_LIMIT = {"reconst_err": 8.8e-4, "err_norm": 1.4e-4, "err_proj_mag": 2.7e-3, "w_norms": 2.2e-3, "second_moment_mse": 3.6e-3}
CIRM_UNIFORM_LIMIT = 3.1e-7
CIRM_LIMIT = 2e-5          # tests/test_forward_gpu.py::test_cirm_build_decompress_dropband (the kernel alone on given STFT values)


def tiny():
    return load("g0_tiny")[1]["config"]


def frames_of(c, lengths=LENGTHS):
    return [1 + n // c["hop"] for n in lengths]


def bound_ratio(d, bound):
    d, bound = d.double(), bound.double()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------- w_mat
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_w_mat_equals_clips_alone_and_oracle(precision, tmp_path, record_err):
    c = tiny()
    model, wts = build_model(c, precision, tmp_path)          # G_pc = 2: the ragged forward must ignore the drop-band
    waves = [x for x, _ in clips(LENGTHS)]
    Tb = frames_of(c)
    with torch.no_grad():
        w = model(padded(waves).cuda(), lengths=LENGTHS)
    assert w.shape == (len(waves), c["K"], 2, c["F"], 1 + max(LENGTHS) // c["hop"])
    P = {k: v.double() for k, v in wts.items()}
    worst_alone, worst_oracle = 0.0, 0.0
    for b, x in enumerate(waves):
        got = w[b, :, :, :, :Tb[b]].cpu().numpy()
        with torch.no_grad():
            alone = model(x[None].cuda())[0].cpu().numpy()
        assert alone.shape == got.shape
        kw = dict(stft=(c["nfft"], c["hop"], c["nfft"]), g_rest=1, g_pc=1, sb_neighbors=c["sbn"])
        ref = R.nppc_forward(x.double()[None], P, c["K"], **kw)[0][0].numpy()
        # the fixture's precondition (nppc_validation_ref.FIRST_CLIP): fp32 itself resolves this clip
        assert rel(R.nppc_forward(x[None], wts, c["K"], **kw)[0][0].numpy(), ref) < ORACLE_FP32_FLOOR
        ea, eo = rel(got, alone), rel(got, ref)
        print(f"{precision} item {b} (T_b = {Tb[b]}): vs alone {ea:.3e}, vs fp64 oracle {eo:.3e}")
        worst_alone, worst_oracle = max(worst_alone, ea), max(worst_oracle, eo)
        assert bool((w[b, :, :, :, Tb[b]:] == 0).all())
    # two identical calls: bit-identical; NaN / 3e38 padding of the waveform: the same bits (never read)
    with torch.no_grad():
        assert torch.equal(w, model(padded(waves).cuda(), lengths=LENGTHS))
        for fill in (float("nan"), 3e38):
            assert torch.equal(w, model(padded(waves, fill).cuda(), lengths=torch.tensor(LENGTHS)))
    record_err("vs_oracle", worst_oracle, W_MAT_ORACLE_LIMIT[precision])
    record_err("batch_vs_alone", worst_alone, W_MAT_ALONE_LIMIT[precision])


def test_ragged_w_mat_on_a_clip_that_fp32_cannot_resolve(tmp_path, record_err):
    """Clip 172 at 4040 samples (T_b = 127): the laplace norm of its signed real / imag maps makes w_mat noise-limited in
    fp32 -- the ORACLE evaluated in fp32 is 9.8e-4 to 1.7e-3 from its own fp64 evaluation (it moves with the CPU's thread
    count), two to three times the 5e-4 the well-conditioned clips are held to.  The bounds here come from that error, computed in the test: the device (fp32) against the fp64 oracle
    within 2 x the oracle's own fp32 error (two fp32 evaluations with different summation orders, each that far from the
    truth), and the item in a batch against the clip alone -- two fp32 evaluations again -- within 1 x.  Zeros past the
    item and bit-identity on repeat hold as everywhere.  Measured: 8.2e-4 and 1.1e-4."""
    c = tiny()
    model, wts = build_model(c, "fp32", tmp_path)
    waves = [x for x, _ in clips([3970, 4040, 4200], first=171)]              # clip 172 is the middle item
    lengths = [w.numel() for w in waves]
    with torch.no_grad():
        w = model(padded(waves).cuda(), lengths=lengths)
        alone = model(waves[1][None].cuda())[0].cpu().numpy()
        assert torch.equal(w, model(padded(waves, float("nan")).cuda(), lengths=lengths))
    tb = 1 + 4040 // c["hop"]
    got = w[1, ..., :tb].cpu().numpy()
    kw = dict(stft=(c["nfft"], c["hop"], c["nfft"]), g_rest=1, g_pc=1, sb_neighbors=c["sbn"])
    ref = R.nppc_forward(waves[1].double()[None], {k: v.double() for k, v in wts.items()}, c["K"], **kw)[0][0].numpy()
    floor = rel(R.nppc_forward(waves[1][None], wts, c["K"], **kw)[0][0].numpy(), ref)
    assert floor > ORACLE_FP32_FLOOR                       # not one of the clips fp32 resolves
    print(f"clip 172: oracle fp32 vs fp64 {floor:.3e}, device vs fp64 {rel(got, ref):.3e}, batch vs alone {rel(got, alone):.3e}")
    assert bool((w[1, ..., tb:] == 0).all())
    record_err("vs_oracle", rel(got, ref), max(2 * floor, W_MAT_ORACLE_LIMIT["fp32"]))    # never tighter than the other clips' limit
    record_err("batch_vs_alone", rel(got, alone), floor)


def test_equal_lengths_match_the_uniform_forward_without_drop_band(tmp_path, record_err):
    """a uniform batch is a ragged batch of equal lengths: the uniform kernels with the drop-band off give the same w_mat"""
    c = tiny()
    model, _ = build_model(c, "fp32", tmp_path, g_pc=1)
    waves = [x for x, _ in clips([4000] * 4, first=190)]
    x = torch.stack(waves).cuda()
    with torch.no_grad():
        uni = model(x)
        rag = model(x, lengths=[4000] * 4)
    record_err("ragged_vs_uniform", rel(rag.cpu().numpy(), uni.cpu().numpy()), W_MAT_ALONE_LIMIT["fp32"])


# ---------------------------------------------------------------------------------------------------- kernels
def ragged_planes(B, K, F, T, frames, seed, fill):
    g = torch.Generator().manual_seed(seed)
    grid = lambda t: torch.round(t * 4096) / 4096          # gt - pred exact in fp32 (tests/test_gsloss_paths_gpu.py: grid)
    x = torch.randn(B, K, 2, F, T, generator=g) * torch.logspace(-1, 1, K).view(1, K, 1, 1, 1)
    gt, pred = grid(torch.randn(B, 2, F, T, generator=g)), grid(torch.randn(B, 2, F, T, generator=g))
    for b, tb in enumerate(frames):
        x[b, ..., tb:], gt[b, ..., tb:], pred[b, ..., tb:] = fill, fill, fill
    return x, gt, pred


@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_ragged_gram_combine_loss_match_fp64_and_are_batch_independent(K, record_err):
    """Limits of tests/test_gsloss_paths_gpu.py for the same quantities: the Gram of test_gram_matches_fp64
    (4 (2N + 1) u53 S, S = sum |a||b|, no prefill), the combination of test_combine_matches_fp64 (u24 |ref| + 2^-45 sum |c||x|),
    the loss outputs of test_loss_solve_matches_fp64 (4 u24 relative, reconst 2^-22 absolute) on the Gram the device built."""
    from nppc_audio import _hip as h
    from nppc_audio import pc_ops
    F, T = 33, 132
    frames = [125, 10, 127, 126, 132]
    B = len(frames)
    fd = torch.tensor(frames, dtype=torch.int32).cuda()
    x, gt, pred = ragged_planes(B, K, F, T, frames, 40 + K, 0.0)
    xd, gd, pd = x.cuda(), gt.cuda(), pred.cuda()
    Gx = pc_ops.gram_ragged(xd, fd)
    w = pc_ops.gram_schmidt_to_crm_ragged(xd, fd)
    Gl = pc_ops.gram_ragged(w, fd, gd, pd)
    out = pc_ops.nppc_loss_ragged(w, gd, pd, fd, 0.37)
    worst = {}

    def keep(tag, v):
        worst[tag] = max(worst.get(tag, 0.0), v)
    for b, tb in enumerate(frames):
        N = F * tb
        xb = x[b:b + 1, ..., :tb].reshape(1, K, 2, N)
        z = GR.vec_set(xb)
        keep("gram_x", bound_ratio((GR.to_planes(GR.gram(z)) - Gx[b:b + 1].cpu()).abs(),
                                   4 * (2 * N + 1) * U53 * GR.gram_mag(z)[..., None].expand(1, K, K, 2)))
        # the combination with the coefficients the device solved (nppc_gs_solve, unchanged, on the device Gram)
        C = torch.empty(1, K, K, 2, dtype=torch.float64, device="cuda")
        Ch = torch.empty_like(C)
        h.call("nppc_gs_solve", Gx[b:b + 1].contiguous(), C, Ch, 1, K, K, h.stream())
        Cc = GR.from_planes(C.cpu())
        ref = GR.combine(Cc, z)
        mag = torch.einsum("bim,bmt->bit", Cc.abs(), z.abs())
        ref_p = torch.stack([ref.real, ref.imag], dim=2)
        got_w = w[b:b + 1, ..., :tb].reshape(1, K, 2, N).cpu().double()
        keep("combine", bound_ratio((got_w - ref_p).abs(), U24 * ref_p.abs() + 2.0 ** -45 * mag[:, :, None]))
        assert bool((w[b, ..., tb:] == 0).all())
        # the loss Gram of the device's own w (fp32), with e = gt - pred
        zw = GR.vec_set(w[b:b + 1, ..., :tb].reshape(1, K, 2, N).cpu(), gt[b:b + 1, ..., :tb].reshape(1, 2, N),
                        pred[b:b + 1, ..., :tb].reshape(1, 2, N))
        keep("gram_loss", bound_ratio((GR.to_planes(GR.gram(zw)) - Gl[b:b + 1].cpu()).abs(),
                                      4 * (2 * N + 1) * U53 * GR.gram_mag(zw)[..., None].expand(1, K + 1, K + 1, 2)))
        ls = GR.loss_solve(GR.from_planes(Gl[b:b + 1].cpu()), K, 1e-8, 0)
        rec, _, en, pr, pi, pm, wn, sm = (t[b:b + 1].cpu().double() for t in (out[0], out[0], *out[2:]))
        for tag, got, want in (("err_norm", en, ls["err_norm"]), ("proj_re", pr, ls["proj"].real), ("proj_im", pi, ls["proj"].imag),
                               ("proj_mag", pm, ls["proj_mag"]), ("w_norms", wn, ls["w_norms"]), ("sm", sm, ls["sm"])):
            keep(tag, bound_ratio((got - want.reshape(got.shape)).abs(), 4 * U24 * want.reshape(got.shape).abs()))
        keep("reconst", float((rec - ls["reconst"]).abs().max()) / 2.0 ** -22)
    want_obj = out[0].double().mean() + 0.37 * out[7].double().mean()
    assert abs(float(out[1]) - float(want_obj)) < 4 * U24 * (abs(float(out[0].double().mean())) + abs(float(want_obj)))
    for tag, v in worst.items():
        print(f"K = {K} {tag}: {v:.3e} of its bound")
        record_err(tag, v, 1.0)

    # bit identity: run to run, alone against in the batch, clean padding against NaN / 3e38 padding
    def run(xd, gd, pd, fd):
        w_ = pc_ops.gram_schmidt_to_crm_ragged(xd, fd)
        return [pc_ops.gram_ragged(xd, fd), w_, pc_ops.gram_ragged(w_, fd, gd, pd), *pc_ops.nppc_loss_ragged(w_, gd, pd, fd, 0.37)]
    base = run(xd, gd, pd, fd)
    for a, b_ in zip(base, run(xd, gd, pd, fd)):
        assert torch.equal(a, b_)
    for fill in (float("nan"), 3e38):
        x2, gt2, pred2 = ragged_planes(B, K, F, T, frames, 40 + K, fill)
        for a, b_ in zip(base, run(x2.cuda(), gt2.cuda(), pred2.cuda(), fd)):
            assert torch.equal(a, b_), fill
    for b, tb in enumerate(frames):
        one = run(xd[b:b + 1, ..., :tb].contiguous(), gd[b:b + 1, ..., :tb].contiguous(), pd[b:b + 1, ..., :tb].contiguous(),
                  fd[b:b + 1].contiguous())
        for i, (a, o) in enumerate(zip(base, one)):
            if i == 1:
                assert torch.equal(a[b:b + 1, ..., :tb], o), (b, "w")
            elif i == 4:                                                    # the objective is a mean over the batch
                continue
            else:
                assert torch.equal(a[b:b + 1], o), (b, i)


def test_ragged_cirm_matches_fp64_and_is_batch_independent(record_err):
    """the ground-truth cIRM per item: against oracle/nppc_ref.ideal_mask in fp64 on the unpadded item at the limit the uniform
    kernel is held to, bit-identical alone and in the batch, zeros past the item, padding never read.  Against the uniform
    kernel on the item alone it is the same formula compiled in another translation unit (fused multiply-adds fall
    differently): measured 1.5e-7 of the largest value on the MI355X, held at 2 x that."""
    from nppc_audio import _hip as h
    from nppc_audio import ops
    F, T = 33, 132
    frames = [125, 10, 127, 126, 132]
    fd = torch.tensor(frames, dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(5)
    maps = [torch.randn(len(frames), F, T, generator=g) for _ in range(4)]
    base = ops.cirm_build_compress_ragged(*[m.cuda() for m in maps], fd)
    worst, worst_uni = 0.0, 0.0
    for b, tb in enumerate(frames):
        item = [m[b:b + 1, :, :tb].contiguous() for m in maps]
        ref = R.ideal_mask(*[m.double() for m in item]).numpy()
        worst = max(worst, rel(base[b:b + 1, :, :, :tb].cpu().numpy(), ref))
        one = torch.empty(1, 2, F, tb, dtype=torch.float32, device="cuda")       # (the entry point: the wrapper asserts B > groups)
        h.call("nppc_cirm_build_compress", *[m.cuda() for m in item], one, 1, F, tb, 1, ops.EPS32, h.stream())
        worst_uni = max(worst_uni, rel(base[b:b + 1, :, :, :tb].cpu().numpy(), one.cpu().numpy()))
        alone = ops.cirm_build_compress_ragged(*[m.cuda() for m in item], fd[b:b + 1].contiguous())
        assert torch.equal(base[b:b + 1, :, :, :tb], alone)
        assert bool((base[b, :, :, tb:] == 0).all())
    print(f"ragged cIRM: vs fp64 {worst:.3e}, vs the uniform kernel on the item alone {worst_uni:.3e}")
    assert torch.equal(base, ops.cirm_build_compress_ragged(*[m.cuda() for m in maps], fd))
    for fill in (float("nan"), 3e38):
        m2 = [m.clone() for m in maps]
        for m in m2:
            for b, tb in enumerate(frames):
                m[b, :, tb:] = fill
        assert torch.equal(base, ops.cirm_build_compress_ragged(*[m.cuda() for m in m2], fd))
    record_err("vs_fp64", worst, CIRM_LIMIT)
    record_err("vs_uniform_kernel", worst_uni, CIRM_UNIFORM_LIMIT)


# ---------------------------------------------------------------------------------------------------- base step
LOG_KEYS = ("pred_crm", "w_mat", "err_norm", "err_proj", "err_proj_mag", "w_norms", "reconst_err", "second_moment_mse", "objective")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_base_step_matches_the_oracle_on_every_clip_alone(precision, tmp_path, record_err):
    from nppc_audio.data import pad_collate
    from nppc_audio.metrics import nppc_direction_scores
    from nppc_audio.trainer import nppc_base_step
    c = tiny()
    model, wts = build_model(c, precision, tmp_path)
    items = clips(LENGTHS)
    batch = pad_collate(items)
    dev_batch = type(batch)(batch.noisy.cuda(), batch.clean.cuda(), batch.lengths)
    rec, obj, log = nppc_base_step(model, dev_batch, 500, 500, 1.0)
    assert not rec.requires_grad and not obj.requires_grad
    P = {k: v.double() for k, v in wts.items()}
    worst = {}
    Tb = frames_of(c)
    for b, (noisy, clean) in enumerate(items):
        _, ref = oracle_step_alone(noisy.double(), clean.double(), P, c, 500)
        for k in ("reconst_err", "err_norm", "err_proj_mag", "w_norms", "second_moment_mse"):
            e = rel(log[k][b].cpu().numpy(), ref[k][0].numpy())
            print(f"{precision} item {b} {k}: {e:.3e}")
            worst[k] = max(worst.get(k, 0.0), e)
        assert bool((log["pred_crm"][b, ..., Tb[b]:] == 0).all()) and bool((log["w_mat"][b, ..., Tb[b]:] == 0).all())
    # the scores reproduce the loss's own reconst_err: residual of all K directions (the loss's normalisation: per |e|^2)
    sc = nppc_direction_scores(log["err_norm"].cpu(), log["err_proj_mag"].cpu(), log["w_norms"].cpu())
    assert np.abs(sc["residual"][:, -1] - log["reconst_err"].cpu().double().numpy()).max() < 2.0 ** -22
    assert abs(float(obj) - float(log["reconst_err"].mean() + 1.0 * log["second_moment_mse"].mean())) < 1e-6
    # run to run, and NaN / 3e38 in every padded sample of both waveforms: the same bits
    again = nppc_base_step(model, (dev_batch.noisy, dev_batch.clean), 500, 500, 1.0, lengths=LENGTHS)[2]
    for k in LOG_KEYS:
        assert torch.equal(log[k], again[k]), k
    for fill in (float("nan"), 3e38):
        nb = (padded([n for n, _ in items], fill).cuda(), padded([cl for _, cl in items], fill).cuda())
        lg = nppc_base_step(model, nb, 500, 500, 1.0, lengths=LENGTHS)[2]
        for k in LOG_KEYS:
            assert torch.equal(log[k], lg[k]), (k, fill)
    # bf16: the only bf16 limit on record for these scalars (reconst_err 2e-4, test_train_step_matches_oracle) belongs to the
    # full-size fixture g2_k5, whose sums average far more elements.  At the tiny size: 2 x the worst measured on the MI355X
    # (profiles/nppc_validation_parity_errors.json: reconst_err 4.4e-4, err_norm 7.1e-5, err_proj_mag 1.3e-3, w_norms 1.1e-3,
    # second_moment_mse 1.8e-3), the rule the bf16 limits of the train-step test follow.
    if precision == "bf16":
        for k, lim in BF16_LOSS_LIMIT.items():
            record_err(k, worst[k], lim)
    if precision == "fp32":
        record_err("reconst_err", worst["reconst_err"], RECONST_LIMIT_FP32)
        for k in ("err_norm", "err_proj_mag", "w_norms", "second_moment_mse"):
            record_err(k, worst[k], LOSS_TERM_LIMIT_FP32)


# ---------------------------------------------------------------------------------------------------- trainer
class _Mem(torch.utils.data.Dataset):
    def __init__(self, noisy, clean):
        self.noisy, self.clean = noisy, clean

    def __len__(self):
        return self.noisy.shape[0]

    def __getitem__(self, i):
        return self.noisy[i], self.clean[i]


def make_trainer(tmp_path, precision="fp32"):
    from nppc_audio.trainer import NPPCAudioTrainer, NPPCAudioTrainerConfig
    c = tiny()
    mc, wts = model_config(c, precision, tmp_path)
    cfg = NPPCAudioTrainerConfig(
        nppc_model_configuration=mc, data_configuration=dict(data_path=".", dataset=dict(clean_path=".", noisy_path=".")),
        data_loader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=0)),
        device="cuda", log_interval=2)
    tr_clips = clips([c["L"]] * c["B"], first=150)
    tr = NPPCAudioTrainer(cfg, dataset=_Mem(torch.stack([n for n, _ in tr_clips]), torch.stack([cl for _, cl in tr_clips])))
    tr.nppc_model.load_state_dict(wts, strict=True)
    tr.nppc_model.to("cuda")
    return tr, c


def val_loader():
    from nppc_audio.data import pad_collate
    items = clips(LENGTHS + [2000, 2000], first=200)
    uniform = (torch.stack([items[5][0], items[6][0]]), torch.stack([items[5][1], items[6][1]]))
    return [pad_collate(items[:3]), pad_collate(items[3:5]), uniform], items


def state_bits(tr):
    out = {"p." + k: v.detach().clone() for k, v in tr.nppc_model.state_dict().items()}
    for i, (p, st) in enumerate(tr.optimizer.state.items()):
        for k, v in st.items():
            out[f"o.{i}.{k}"] = v.detach().clone() if isinstance(v, torch.Tensor) else torch.tensor(v)
    out["rng.cpu"] = torch.get_rng_state()
    out["rng.cuda"] = torch.cuda.get_rng_state()
    return out


def test_validate_returns_the_direction_scores_and_leaves_the_trainer_untouched(tmp_path):
    from nppc_audio.metrics import nppc_direction_scores
    from nppc_audio.trainer import nppc_base_step
    tr, c = make_trainer(tmp_path)
    loader, items = val_loader()
    batch = next(iter(tr.dataloader))
    batch = tuple(x.cuda() for x in batch)
    tr.step = 500
    tr.train_step(batch)                                  # Adam state exists, an update was applied
    before = state_bits(tr)
    modes = [m.training for m in tr.nppc_model.modules()]
    m = tr.validate(loader)
    after = state_bits(tr)
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert modes == [mm.training for mm in tr.nppc_model.modules()]
    assert tr.val_history == [m] and m["n_clips"] == len(items) and m["step"] == tr.step
    json.dumps(m)
    # every clip alone through the ragged step (a batch of one): the per-item values validate saw, bit for bit
    en, pm, wn, rec, sm = [], [], [], [], []
    for noisy, clean in items:
        lg = nppc_base_step(tr.nppc_model, (noisy[None].cuda(), clean[None].cuda()), tr.step, 500, 1.0, lengths=[noisy.numel()])[2]
        en.append(lg["err_norm"].cpu()), pm.append(lg["err_proj_mag"].cpu()), wn.append(lg["w_norms"].cpu())
        rec.append(lg["reconst_err"].cpu()), sm.append(lg["second_moment_mse"].cpu())
    en, pm, wn, rec, sm = (torch.cat(t).double().numpy() for t in (en, pm, wn, rec, sm))
    # a clip's loss terms in a batch and alone differ by the forward's summation order only: the fp32 limits of
    # tests/test_train_step_gpu.py (reconst_err 1e-4, the other terms 5e-4)
    assert rel(np.asarray(m["per_item"]["reconst_err"]), rec) < RECONST_LIMIT_FP32
    for k, ref in (("err_norm", en), ("err_proj_mag", pm), ("w_norms", wn), ("second_moment_mse", sm)):
        assert rel(np.asarray(m["per_item"][k]), ref) < LOSS_TERM_LIMIT_FP32, k
    # the returned dict IS nppc_direction_scores of the per-item values it carries
    pi = {k: np.asarray(v) for k, v in m["per_item"].items()}
    sc = nppc_direction_scores(pi["err_norm"], pi["err_proj_mag"], pi["w_norms"])
    for k_out, k_sc in (("captured", "captured_mean"), ("residual", "residual_mean"), ("captured_pooled", "captured_pooled"),
                        ("residual_pooled", "residual_pooled"), ("calibration", "calibration")):
        np.testing.assert_allclose(np.asarray(m[k_out]), sc[k_sc], rtol=1e-12, atol=0)
    ref = direction_scores_np(pi["err_norm"], pi["err_proj_mag"], pi["w_norms"])
    np.testing.assert_allclose(np.asarray(m["calibration"]), ref["calibration"], rtol=1e-12)
    assert abs(m["reconst_err"] - pi["reconst_err"].mean()) < 1e-12 and abs(m["residual"][-1] - m["reconst_err"]) < 2.0 ** -22
    assert abs(m["second_moment_mse"] - pi["second_moment_mse"].mean()) < 1e-12


def test_training_with_a_validation_loader_ends_in_the_same_weights(tmp_path, record_err):
    """Four training steps with and without a validation loader.  Around EVERY in-training validation the weights, the
    Adam state and the RNG are bit-identical before and after it: that is what validation can be held to, and it is.

    DEVIATION from the issue, which asks for bit-identical final weights of the two runs: they are two independent training
    runs, and the existing train step cannot promise equal bits from run to run (tests/test_fsn_restorer_trainer_gpu.py::
    test_two_runs_agree states the same for the restorer trainer: existing kernels reduce with atomics whose last bits
    follow the arrival order).  Measured on the MI355X, five runs of these four steps from the same weights: three ended
    bit-identical, two differed from them -- one weight by 1 ulp (3.7e-9) after the second step, before any validation had
    run, at most 1.2e-7 (1 ulp of a weight near 1) in 33641 of the weights after the fourth.  Held instead, as there: the
    share of weights that differ by more than 1e-3 lr plus one fp32 ulp of the weight stays below 1e-3.  Anything
    validation could do to the trajectory -- a stale packed weight, a skipped or doubled update, a disturbed Adam moment --
    moves every weight by about lr per step, a thousand times that threshold."""
    from nppc_audio.nppc_model import NPPCModel
    finals = []
    for use_val in (False, True):
        d = tmp_path / ("val" if use_val else "plain")
        d.mkdir()
        tr, c = make_trainer(d)
        loader, _ = val_loader()
        tr.step = 498
        if use_val:
            inner, seen = tr.validate, []

            def checked(dl):
                tr.flush()
                torch.cuda.synchronize()
                before = state_bits(tr)
                m = inner(dl)
                after = state_bits(tr)
                assert set(before) == set(after)
                for k in before:
                    assert torch.equal(before[k], after[k]), (tr.step, k)
                seen.append(tr.step)
                return m
            object.__setattr__(tr, "validate", checked)
            tr.train(n_steps=4, checkpoint_dir=str(d / "ck"), val_dataloader=loader, validate_every=2)
            assert seen == [500, 502] == [h["step"] for h in tr.val_history]
            hist = glob.glob(str(d / "ck" / "val_history_*.json"))
            assert len(hist) == 1 and json.load(open(hist[0])) == tr.val_history
            best = torch.load(str(d / "ck" / "best_model.pth"), map_location="cpu")
            assert best["reconst_err"] == min(h["reconst_err"] for h in tr.val_history) == tr.best_val_reconst_err
            assert best["step"] in (500, 502)
            NPPCModel(tr.nppc_model.config).load_state_dict(best["model_state_dict"], strict=True)
        else:
            tr.train(n_steps=4, checkpoint_dir=str(d / "ck"))
            assert tr.val_history == [] and not glob.glob(str(d / "ck" / "val_history_*")) and not (d / "ck" / "best_model.pth").exists()
        assert tr.step == 502
        finals.append({k: v.detach().cpu().clone() for k, v in tr.nppc_model.state_dict().items()})
    w0, w1 = (torch.cat([f[k].double().reshape(-1) for k in sorted(f)]) for f in finals)
    d = (w0 - w1).abs()
    over = d > 1e-3 * 1e-4 + 2.0 ** -23 * w0.abs()
    print(f"weights after 4 steps, with vs without validation: max |dw| {float(d.max()):.3e}, {int((d > 0).sum())} of {d.numel()} "
          f"differ, {int(over.sum())} by more than 1e-3 lr + 1 ulp")
    record_err("frac_differing", float(over.double().mean()), 1e-3)


def test_validate_at_the_final_checkpoint_by_default(tmp_path):
    tr, c = make_trainer(tmp_path)
    loader, _ = val_loader()
    tr.train(n_steps=2, checkpoint_dir=str(tmp_path / "ck"), val_dataloader=loader)
    assert [h["step"] for h in tr.val_history] == [2] and (tmp_path / "ck" / "best_model.pth").exists()


# ---------------------------------------------------------------------------------------------------- errors
def test_error_paths(tmp_path):
    from nppc_audio import pc_ops
    from nppc_audio.data import RaggedBatch
    from nppc_audio.trainer import nppc_base_step
    c = tiny()
    model, _ = build_model(c, "fp32", tmp_path)
    x = torch.zeros(2, 4000).cuda()
    with torch.no_grad():
        with pytest.raises(ValueError, match="item 1"):
            model(x, lengths=[4000, 20])                              # L_b <= nfft // 2
        with pytest.raises(ValueError, match="item 1"):
            model(x, lengths=[4000, 100])                             # 4 frames < the TSSE kernel of 10
        with pytest.raises(ValueError, match="item 0"):
            model(x, lengths=[4001, 3000])                            # longer than the padded width
        with pytest.raises(ValueError, match="host"):
            model(x, lengths=torch.tensor([4000, 3000]).cuda())       # would have to be read back
    tr, _ = make_trainer(tmp_path)
    with pytest.raises(ValueError, match="item 1"):
        tr.validate([RaggedBatch(torch.zeros(2, 4000), torch.zeros(2, 4000), torch.tensor([4000, 100]))])
    with pytest.raises(RuntimeError, match="inference only"):
        model(x, lengths=[4000, 4000])                                # autograd on, trainable direction net
    net = model.audio_pc_wrapper.net
    maps = [torch.zeros(2, 1, c["F"], 126).cuda() for _ in range(6)]
    ok = torch.tensor([126, 126], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="inference only"):
        net.engine().forward(maps, train=True, frames=ok)
    for bad in (ok.long(), ok.cpu(), ok[:1]):
        with torch.no_grad(), pytest.raises(ValueError, match="int32"):
            net(*maps, frames=bad)
        with pytest.raises(ValueError, match="int32"):
            pc_ops.gram_ragged(torch.zeros(2, 3, 2, c["F"], 126).cuda(), bad)
    with pytest.raises(RuntimeError, match="forward only"):
        pc_ops.gram_schmidt_to_crm_ragged(torch.zeros(2, 3, 2, c["F"], 126).cuda().requires_grad_(), ok)
    with pytest.raises(RuntimeError, match="forward only"):
        pc_ops.nppc_loss_ragged(torch.zeros(2, 3, 2, c["F"], 126).cuda().requires_grad_(), torch.zeros(2, 2, c["F"], 126).cuda(),
                                torch.zeros(2, 2, c["F"], 126).cuda(), ok, 1.0)
    # the step itself switches autograd off: no error, nothing to differentiate
    rec, obj, _ = nppc_base_step(model, (x + 0.01 * torch.randn_like(x), x), 0, 500, 1.0, lengths=[4000, 3000])
    assert not obj.requires_grad
