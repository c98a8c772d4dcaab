"""GPU: DNS dynamic mixing on the device (nppc_audio/dns_data.py, csrc/dns_mix.hip) -- nppc_rir_convolve against the fp64
direct convolution at edge shapes (limit: twice the error of scipy's fp32 fftconvolve, what the reference runs, on the same
inputs, floored at 2^-23 of the peak), its exactness and batch-independence contracts, nppc_dns_snr_mix and the whole
DeviceReverbMixLoader against the REFERENCE's items (tests/golden/dns_mix.*, limit 3 * e_ref floored the same way), and
two FullSubNetPlusTrainer steps fed by DynamicMixDataset."""
import numpy as np
import pytest
import torch

import dns_mix_ref as M
from fsn_restorer_ref import CONFIGS, weights
from test_dns_data_cpu import dataset, gold, mix_inputs, pools  # noqa: F401  (gold is a fixture)

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23
_REF = {}


def conv_item(L, j):
    """item j at length L: (clean [L] fp32, rir fp32 (full length, may exceed L), fp64 direct convolution, the error of
    scipy's fp32 fftconvolve against it); the tap counts cycle through the edge cases"""
    if (L, j) not in _REF:
        from scipy import signal
        lens = [1000, L, 0, 1, 2, 63, 64, 65, L + 37]
        n = lens[j % len(lens)]
        rng = np.random.Generator(np.random.PCG64(7000 + 31 * j + L))
        clean = (0.1 * rng.standard_normal(L)).astype(np.float32)
        rir = (rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 5.0 + 1.0))).astype(np.float32)
        want = M.rir_convolve(clean, rir[:L])
        err_scipy = M.rel_peak(signal.fftconvolve(clean, rir)[:L], want) if n else 0.0
        _REF[(L, j)] = (clean, rir, want, err_scipy)
    return _REF[(L, j)]


def pack_rirs(rirs, fill=0.0):
    ldr = max(max(len(r) for r in rirs), 1)
    out = np.full((len(rirs), ldr), fill, dtype=np.float32)
    for b, r in enumerate(rirs):
        out[b, :len(r)] = r
    return torch.from_numpy(out), torch.tensor([len(r) for r in rirs], dtype=torch.int32)


def convolve(clean, rirs, fill=0.0):
    from nppc_audio.dns_data import rir_convolve_on_device
    rir, rir_len = pack_rirs(rirs, fill)
    out = rir_convolve_on_device(torch.from_numpy(np.stack(clean)).cuda(), rir.cuda(), rir_len.cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. the convolution against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 255, 4097, 49152])
@pytest.mark.parametrize("B", [1, 3, 18])
def test_rir_convolve_matches_fp64_direct(B, L, record_err):
    items = [conv_item(L, j) for j in range(B)]
    got = convolve([it[0] for it in items], [it[1] for it in items])
    worst = (0.0, 1.0)
    for b, (clean, rir, want, err_scipy) in enumerate(items):
        err, lim = M.rel_peak(got[b], want), max(2.0 * err_scipy, FLOOR)
        print(f"B={B} L={L} item {b}: {len(rir)} taps, err {err:.2e}, scipy fp32 {err_scipy:.2e}, limit {lim:.2e}")
        if len(rir) == 0:
            assert np.array_equal(got[b], clean)
        if err / lim >= worst[0] / worst[1]:
            worst = (err, lim)
    record_err(f"rir_convolve.B{B}.L{L}", worst[0], worst[1])


# ---- 2. exactness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [255, 4097, 49152])
def test_rir_convolve_exact_cases(L):
    rng = np.random.Generator(np.random.PCG64(L))
    x = (0.3 * rng.standard_normal(L)).astype(np.float32)
    d = min(100, L - 1)
    delayed = np.zeros(d + 1, dtype=np.float32)
    delayed[d] = 1.0
    far = np.zeros(L, dtype=np.float32)                  # the impulse on the last tap that can contribute
    far[L - 1] = 1.0
    got = convolve([x, x, x, x], [np.ones(1, dtype=np.float32), delayed, np.zeros(0, dtype=np.float32), far], fill=np.nan)
    assert np.array_equal(got[0], x), "rir = [1] must return the input bit for bit"
    assert np.array_equal(got[1][d:], x[:L - d]) and not got[1][:d].any(), "a delayed unit impulse must shift the input"
    assert np.array_equal(got[2], x), "rir_len = 0 must copy the input"
    assert got[3][L - 1] == x[0] and not got[3][:L - 1].any()


# ---- 3. independence of the batch, of the padding and of the run -------------------------------------------------------------
@pytest.mark.parametrize("L", [4097, 49152])
def test_rir_convolve_item_is_independent_of_its_batch(L):
    from nppc_audio.dns_data import rir_convolve_on_device
    probes = [conv_item(L, j) for j in (0, 5, 8, 1)]             # 1000 taps, 63, L + 37 (longer than the clip), L
    others = [conv_item(L, j) for j in (2, 3, 6)]
    alone = [convolve([p[0]], [p[1]])[0] for p in probes]
    for fill in (3e38, np.nan):
        clean = [p[0] for p in probes] + [o[0] for o in others]
        rirs = [p[1] for p in probes] + [o[1] for o in others]
        rir, rir_len = pack_rirs(rirs, fill)
        rir = torch.cat([rir, torch.full((len(rirs), 77), fill)], dim=1)      # a wider ldr than any item needs
        rir[2, L:] = fill                                                     # taps at or beyond L: never read
        args = (torch.from_numpy(np.stack(clean)).cuda(), rir.cuda(), rir_len.cuda())
        runs = [rir_convolve_on_device(*args).cpu().numpy() for _ in range(2)]
        assert np.array_equal(runs[0], runs[1]), "two runs differ"
        assert np.isfinite(runs[0]).all()
        for b, a in enumerate(alone):
            assert np.array_equal(runs[0][b], a), f"item {b} changes with its batch (padding {fill})"


def test_argument_checks():
    from nppc_audio.dns_data import rir_convolve_on_device, snr_mix_on_device
    x, r = torch.zeros(2, 64).cuda(), torch.zeros(2, 8).cuda()
    n = torch.tensor([8, 3], dtype=torch.int32).cuda()
    rir_convolve_on_device(x, r, n)
    for bad in ((x.cpu(), r, n), (x.double(), r, n), (x, r[:1], n), (x, r, n.long()), (x, r, n[:1]),
                (x, r, torch.tensor([9, 0], dtype=torch.int32).cuda()), (x, r, torch.tensor([-1, 0], dtype=torch.int32).cuda())):
        with pytest.raises(ValueError):
            rir_convolve_on_device(*bad)
    s = torch.zeros(2).cuda()
    snr_mix_on_device(x, x, s, s)
    for bad in ((x, x[:, :5], s, s), (x, x.cpu(), s, s), (x, x, s[:1], s), (x, x, s, s.double()), (x.half(), x, s, s)):
        with pytest.raises(ValueError):
            snr_mix_on_device(*bad)


# ---- 4. the mix and the loader against the reference's items -----------------------------------------------------------------
def test_snr_mix_matches_the_reference(gold, record_err):  # noqa: F811
    from nppc_audio.dns_data import rir_convolve_on_device, snr_mix_on_device
    z, meta = gold
    sides = set()
    for case in meta["mix"]:
        clean, noise, rir = mix_inputs(z, meta, case)
        c = torch.from_numpy(clean)[None].cuda()
        if rir is not None:
            r, n = pack_rirs([rir[:len(clean)]])
            c = rir_convolve_on_device(c, r.cuda(), n.cuda())
            e = M.rel_peak(c[0].cpu().numpy(), M.rir_convolve(clean, rir))
            record_err(f"conv.{case['name']}", e, M.limit(case["e_ref_conv"]))
        noisy, cl = snr_mix_on_device(c, torch.from_numpy(noise)[None].cuda(), torch.tensor([float(case["snr"])]).cuda(),
                                      torch.tensor([float(case["level"])]).cuda(), meta["target_dB_FS"])
        noisy, cl = noisy[0].cpu().numpy(), cl[0].cpu().numpy()
        assert np.isfinite(noisy).all() and np.isfinite(cl).all(), case["name"]
        en, ec = M.rel_peak(noisy, z[f"mix.{case['name']}.noisy"]), M.rel_peak(cl, z[f"mix.{case['name']}.clean"])
        print(f"{case['name']}: noisy {en:.2e} / {M.limit(case['e_ref_noisy']):.2e}, clean {ec:.2e} / {M.limit(case['e_ref_clean']):.2e}")
        record_err(f"noisy.{case['name']}", en, M.limit(case["e_ref_noisy"]))
        record_err(f"clean.{case['name']}", ec, M.limit(case["e_ref_clean"]))
        # the clip rule on the fixture's side: after it the peak is 0.99 - 1e-6, without it the peak stays as it was
        peak = float(np.abs(noisy).max())
        assert (abs(peak - (0.99 - 1e-6)) < 1e-6) == case["clipped"], (case["name"], peak)
        sides.add(case["clipped"])
    assert sides == {True, False}
    # all-zero clean and noise stay finite
    zero = torch.zeros(2, 500).cuda()
    zn, zc = snr_mix_on_device(zero, zero, torch.zeros(2).cuda(), torch.full((2,), -20.0).cuda())
    assert bool(torch.isfinite(zn).all()) and bool(torch.isfinite(zc).all())


@pytest.mark.parametrize("floating", [3, 10])
def test_loader_matches_the_reference_items(gold, floating, record_err):  # noqa: F811
    from nppc_audio.dns_data import DeviceReverbMixLoader, rir_convolve_on_device, snr_mix_on_device
    z, meta = gold
    ds = dataset(z, meta, floating)
    cases = [c for c in meta["items"] if c["floating"] == floating]
    singles, hosts = [], []
    for case in cases:
        ds.rng.seed(case["seed"])
        ds.np_rng.seed(case["seed"])
        loader = DeviceReverbMixLoader(ds, [[case["idx"]]], device="cuda", pin_memory=False)
        (noisy, clean), = list(loader)
        assert noisy.shape == (1, ds.config.crop_length) and noisy.is_cuda
        en = M.rel_peak(noisy[0].cpu().numpy(), z[case["key"] + ".noisy"])
        ec = M.rel_peak(clean[0].cpu().numpy(), z[case["key"] + ".clean"])
        print(f"{case['key']}: rir {case['rir_len']}, noisy {en:.2e} / {M.limit(case['e_ref_noisy']):.2e}, "
              f"clean {ec:.2e} / {M.limit(case['e_ref_clean']):.2e}")
        record_err(f"noisy.{case['key']}", en, M.limit(case["e_ref_noisy"]))
        record_err(f"clean.{case['key']}", ec, M.limit(case["e_ref_clean"]))
        peak = float(noisy.abs().max())
        assert (abs(peak - (0.99 - 1e-6)) < 1e-6) == case["clipped"], (case["key"], peak)
        singles.append((noisy[0].cpu(), clean[0].cpu()))
        ds.rng.seed(case["seed"])
        ds.np_rng.seed(case["seed"])
        hosts.append(loader.gather([case["idx"]]))
    # the same items as ONE batch: bit-identical to each item mixed alone
    ldr = max(h[2].shape[1] for h in hosts)
    rir = torch.cat([torch.nn.functional.pad(h[2], (0, ldr - h[2].shape[1])) for h in hosts])
    clean, noise, rir_len, m = (torch.cat([h[i] for h in hosts]).cuda() for i in (0, 1, 3, 4))
    rev = rir_convolve_on_device(clean, rir.cuda(), rir_len)
    noisy, cl = snr_mix_on_device(rev, noise, m[:, 0].contiguous(), m[:, 1].contiguous(), meta["target_dB_FS"])
    for b, (n1, c1) in enumerate(singles):
        assert torch.equal(noisy[b].cpu(), n1) and torch.equal(cl[b].cpu(), c1), cases[b]["key"]


# ---- 5. the trainer fed by the dynamic mixer ------------------------------------------------------------------------------
def test_trainer_consumes_the_dynamic_mix(gold, record_err):  # noqa: F811
    from nppc_audio.dns_data import DeviceReverbMixLoader, DNSDatasetConfig, DynamicMixDataset
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer, FullSubNetPlusTrainerConfig
    z, meta = gold
    c = CONFIGS["fsr_tiny"]
    clean, noise, rir = pools(z, meta)
    dcfg = DNSDatasetConfig(sub_sample_length=c["L"] / 16000, silence_length=meta["silence_length"])
    assert dcfg.crop_length == c["L"]
    ds, twin = (DynamicMixDataset(dcfg, clean, noise, rir, seed=11) for _ in range(2))
    cfg = FullSubNetPlusTrainerConfig(
        model_configuration=dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                 num_groups_in_drop_band=c["G"], precision="fp32"),
        dataloader_configuration=dict(batch_size=c["B"], num_workers=0, pin_memory=False, shuffle=False),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda")
    tr = FullSubNetPlusTrainer(cfg, dataset=ds)
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights(c).items()}, strict=True)
    assert isinstance(tr.dataloader, DeviceReverbMixLoader)
    assert len(tr.dataloader) == len(ds) // c["B"] == 1, "drop_last: the partial batch must not reach drop-band"
    reverberant = 0
    for step in range(2):
        (batch,) = list(tr.dataloader)                       # one epoch = one full batch
        noisy, cl = batch
        assert noisy.shape == (c["B"], c["L"]) and noisy.is_cuda
        loss, log = tr.train_step(batch)
        assert np.isfinite(loss.item()) and np.isfinite(float(log["grad_norm"]))
        for b in range(c["B"]):
            state = (twin.rng.getstate(), twin.np_rng.get_state())
            it = twin.draw(b)
            twin.rng.setstate(state[0])
            twin.np_rng.set_state(state[1])
            hn, hc = twin[b]                                     # the host item: scipy's fp32 fftconvolve, fp32 snr_mix
            n64, c64 = M.snr_mix(it.clean, it.noise, it.snr, dcfg.target_dB_FS, it.level, rir=it.rir)
            reverberant += it.rir is not None
            # the host item's own distance from the fp64 recipe sets the limit, like e_ref of the fixture
            record_err(f"step{step}.item{b}.noisy", M.rel_peak(noisy[b].cpu().numpy(), hn), M.limit(M.rel_peak(hn, n64)))
            record_err(f"step{step}.item{b}.clean", M.rel_peak(cl[b].cpu().numpy(), hc), M.limit(M.rel_peak(hc, c64)))
    assert reverberant >= 2 and tr.step == 2
