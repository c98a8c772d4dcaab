"""GPU: ragged (variable-length) inference of the FullSubNet+ restorer: padded batches with per-item
lengths through the STFT / iSTFT, the restorer forward, ModelValidator and FullSubNetPlusTrainer.validate_metrics.  Every
item must equal the same clip run alone; padding is never read; outputs past an item's end are 0."""
import json
import os

import numpy as np
import pytest
import torch

import se_metrics_ref as SR
from fsn_restorer_ref import CONFIGS, weights
from golden_util import rel
from oracle import nppc_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = CONFIGS["fsr_tiny"]
# fsr_tiny STFT (nfft 64, hop 32, look-ahead 2): T = 125, 10 (the shortest legal clip: the TSSE kernel of 10), 127, 126,
# 132 frames -> T + la = 127, 12, 129, 128, 134 (the last crosses into a second 128-row tile)
LENGTHS = [3970, 288, 4040, 4001, 4200]
ORACLE_LIMIT = {"fp32": 3e-4, "bf16": 2e-2}       # test_forward_gpu.py::test_restorer_forward_matches_reference
# batch vs alone: <= 2x the worst measured on the MI355X
# (fp32 7.9e-7, bf16 1.9e-3 at fsr_tiny, bf16 5.2e-3 at the train.toml size: bf16 roundings that flip with the summation
# order of the GroupNorm / laplace-norm sums)
ALONE_LIMIT = {"fp32": 1.6e-6, "bf16": 3.8e-3, "bf16_full": 1.1e-2}
ENHANCE_REL = 2e-5                                # test_model_validator_gpu.py (the same fixture comparison)


def clips(lengths, first=70):
    out = []
    for i, n in enumerate(lengths):
        noisy, clean = W.synth_batch(1, n, first_clip=first + i)
        out.append((torch.from_numpy(noisy[0]), torch.from_numpy(clean[0])))
    return out


def padded(xs, fill=0.0):
    L = max(x.numel() for x in xs)
    out = torch.full((len(xs), L), fill, dtype=torch.float32)
    for i, x in enumerate(xs):
        out[i, :x.numel()] = x
    return out


def restorer(c, precision, groups=1):
    from nppc_audio.fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
    net = FullSubNet_Plus(FullSubNetPlusConfig(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                               num_groups_in_drop_band=groups, precision=precision))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights(c).items()}, strict=True)
    return net.cuda().eval()


def ragged_forward(net, waves, c):
    from nppc_audio import ops
    lengths = [w.numel() for w in waves]
    with torch.no_grad():
        mag, re, im = ops.stft(padded(waves).cuda(), c["nfft"], c["hop"], lengths=lengths)
        return net(mag[:, None], re[:, None], im[:, None], frames=ops.stft_frames(lengths, c["hop"]))


def alone_forward(net, wave, c):
    from nppc_audio import ops
    with torch.no_grad():
        mag, re, im = ops.stft(wave[None].cuda(), c["nfft"], c["hop"])
        return net(mag[:, None], re[:, None], im[:, None])


# ---------------------------------------------------------------------------------------------------- STFT / iSTFT
def test_stft_istft_ragged_match_single_clips():
    from nppc_audio import ops
    c = TINY
    waves = [x for x, _ in clips(LENGTHS)]
    lengths = torch.tensor(LENGTHS)
    mag, re, im = ops.stft(padded(waves).cuda(), c["nfft"], c["hop"], lengths=lengths)
    T = re.shape[-1]
    for b, w in enumerate(waves):
        Tb = 1 + LENGTHS[b] // c["hop"]
        m1, r1, i1 = ops.stft(w[None].cuda(), c["nfft"], c["hop"])
        om, orr, oi = R.stft_parts(w.double(), c["nfft"], c["hop"], c["nfft"])
        for got, alone, ref in ((re, r1, orr), (im, i1, oi), (mag, m1, om)):
            assert torch.equal(got[b, :, :Tb], alone[0])          # one kernel body: the same bits
            assert rel(got[b, :, :Tb].cpu().numpy(), ref[0, 0].numpy()) < 2e-6
            assert bool((got[b, :, Tb:] == 0).all()), (b, Tb, T)
    # padding is never read: NaN / 3e38 padding gives the same bits as zero padding
    for fill in (float("nan"), 3e38):
        m2, r2, i2 = ops.stft(padded(waves, fill).cuda(), c["nfft"], c["hop"], lengths=lengths)
        for a, b_ in ((mag, m2), (re, r2), (im, i2)):
            assert torch.equal(a, b_)
    # iSTFT of the ragged spectra: each item equals the clip's own iSTFT, zeros past its length
    out = ops.istft(re, im, c["nfft"], c["hop"], max(LENGTHS), lengths=lengths)
    for b, w in enumerate(waves):
        Tb = 1 + LENGTHS[b] // c["hop"]
        one = ops.istft(re[b:b + 1, :, :Tb], im[b:b + 1, :, :Tb], c["nfft"], c["hop"], LENGTHS[b])
        ref = torch.istft(torch.complex(re[b, :, :Tb].double().cpu(), im[b, :, :Tb].double().cpu()), c["nfft"], c["hop"],
                          c["nfft"], torch.hann_window(c["nfft"], dtype=torch.float64), center=True, length=LENGTHS[b])
        assert torch.equal(out[b, :LENGTHS[b]], one[0])
        assert rel(out[b, :LENGTHS[b]].cpu().numpy(), ref.numpy()) < 2e-6
        assert bool((out[b, LENGTHS[b]:] == 0).all())
    # NaN / huge values in the spectra past an item's frames are not read either
    re2, im2 = re.clone(), im.clone()
    for b in range(len(waves)):
        Tb = 1 + LENGTHS[b] // c["hop"]
        re2[b, :, Tb:] = float("nan")
        im2[b, :, Tb:] = 3e38
    assert torch.equal(out, ops.istft(re2, im2, c["nfft"], c["hop"], max(LENGTHS), lengths=lengths))


# (nfft, hop) -> limits of the error against torch.stft / torch.istft in fp64.  64 / 32: the test above; 512 / 256:
# test_forward_gpu.py (test_stft_matches_reference, test_istft_roundtrip_and_enhanced_waveform).  No test bounded the two
# overlap-8 shapes: twice the worst error, on this test's inputs, of the separate uniform and ragged kernels that the one
# template replaced (128 / 16: 1.155e-7 / 1.029e-7, 512 / 64: 1.301e-7 / 1.339e-7, the same for both)
FFT_SHAPES = {(64, 32): (2e-6, 2e-6), (128, 16): (2 * 1.155e-7, 2 * 1.029e-7), (512, 256): (2e-6, 2e-6),
              (512, 64): (2 * 1.301e-7, 2 * 1.339e-7)}


@pytest.mark.parametrize("short", [True, False])
@pytest.mark.parametrize("nfft,hop", list(FFT_SHAPES))
def test_equal_lengths_ragged_stft_istft_equal_uniform(nfft, hop, short, record_err):
    """a padded batch whose items all have the same length gives the bits of the uniform call: the shortest legal clip, and
    9 frames (a second, partial STFT workgroup; an iSTFT workgroup that straddles the item's end).  hop = nfft / 8 fills
    every frame slot of the iSTFT kernel, 512 / 64 at its largest LDS footprint."""
    from nppc_audio import ops
    B, L = 3, nfft // 2 + 1 if short else 8 * hop + 3
    Tb, pad = 1 + L // hop, 2 * hop + 5
    x = torch.stack([w for w, _ in clips([L] * B, first=130)])
    xp = torch.full((B, L + pad), float("nan"))
    xp[:, :L] = x
    uni = ops.stft(x.cuda(), nfft, hop)
    for wave in (x, xp):                                   # ld == L, and NaN padding past it
        rag = ops.stft(wave.cuda(), nfft, hop, lengths=[L] * B)
        for u, r in zip(uni, rag):
            assert r.shape[-1] == 1 + wave.shape[1] // hop
            assert torch.equal(r[:, :, :Tb], u) and bool((r[:, :, Tb:] == 0).all())
    win = torch.hann_window(nfft, dtype=torch.float64)
    ref = torch.stft(x.double(), nfft, hop, nfft, win, center=True, pad_mode="reflect", return_complex=True)
    lim_stft, lim_istft = FFT_SHAPES[(nfft, hop)]
    mag, re, im = uni
    # every part against the spectrum's largest magnitude: the shortest clip at hop = nfft / 2 is two frames that the
    # reflection makes symmetric, so its imaginary part is zero and has no scale of its own
    err = max(float((got.cpu().double() - want).abs().max()) for got, want in ((re, ref.real), (im, ref.imag), (mag, ref.abs())))
    err /= float(ref.abs().max())
    print(f"stft {nfft}/{hop} L={L}: rel {err:.3e}")
    record_err("stft_vs_fp64", err, lim_stft)
    back = ops.istft(re, im, nfft, hop, L)
    rp, ip = (torch.full((B, nfft // 2 + 1, Tb + 3), fill, device="cuda") for fill in (float("nan"), 3e38))
    rp[:, :, :Tb], ip[:, :, :Tb] = re, im
    for r_, i_, ld in ((re, im, L), (rp, ip, L + pad)):
        rag = ops.istft(r_, i_, nfft, hop, ld, lengths=[L] * B)
        assert torch.equal(rag[:, :L], back) and bool((rag[:, L:] == 0).all())
    ref = torch.istft(torch.complex(re.double().cpu(), im.double().cpu()), nfft, hop, nfft, win, center=True, length=L)
    err = rel(back.cpu().numpy(), ref.numpy())
    print(f"istft {nfft}/{hop} L={L}: rel {err:.3e}")
    record_err("istft_vs_fp64", err, lim_istft)


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_forward_equals_clips_alone_and_oracle(precision, record_err):
    c = TINY
    net = restorer(c, precision)
    waves = [x for x, _ in clips(LENGTHS)]
    out = ragged_forward(net, waves, c)
    F, T = c["F"], 1 + max(LENGTHS) // c["hop"]
    assert out.shape == (len(waves), 2, F, T)
    P = {k: torch.from_numpy(v).double() for k, v in weights(c).items()}
    worst_alone, worst_oracle = 0.0, 0.0
    for b, w in enumerate(waves):
        Tb = 1 + LENGTHS[b] // c["hop"]
        got = out[b, :, :, :Tb].cpu().numpy()
        alone = alone_forward(net, w, c)[0].cpu().numpy()
        assert alone.shape == got.shape
        worst_alone = max(worst_alone, rel(got, alone))
        mag, re, im = R.stft_parts(w.double()[None], c["nfft"], c["hop"], c["nfft"])
        ref = R.restorer_forward(mag, re, im, P, groups=1, sb_neighbors=c["sbn"])[0].numpy()
        worst_oracle = max(worst_oracle, rel(got, ref))
        assert bool((out[b, :, :, Tb:] == 0).all())
    record_err("batch_vs_alone", worst_alone, ALONE_LIMIT[precision])
    record_err("vs_oracle", worst_oracle, ORACLE_LIMIT[precision])
    # two identical calls: bit-identical (no float atomics on the ragged path)
    assert torch.equal(out, ragged_forward(net, waves, c))
    # padding is never read
    from nppc_audio import ops
    with torch.no_grad():
        mag, re, im = ops.stft(padded(waves, float("nan")).cuda(), c["nfft"], c["hop"], lengths=LENGTHS)
        o2 = net(mag[:, None], re[:, None], im[:, None], frames=ops.stft_frames(LENGTHS, c["hop"]))
    assert torch.equal(out, o2)


def test_ragged_forward_ignores_drop_band(record_err):
    c = TINY
    net = restorer(c, "fp32", groups=2)
    waves = [x for x, _ in clips(LENGTHS[:4], first=80)]
    out = ragged_forward(net, waves, c)
    assert out.shape[2] == c["F"]                     # all F bins: a batch of one never drop-bands
    worst = 0.0
    for b, w in enumerate(waves):
        Tb = 1 + w.numel() // c["hop"]
        worst = max(worst, rel(out[b, :, :, :Tb].cpu().numpy(), alone_forward(net, w, c)[0].cpu().numpy()))
    record_err("batch_vs_alone", worst, ALONE_LIMIT["fp32"])


def test_equal_lengths_match_uniform_batched_forward(record_err):
    from nppc_audio import ops
    c = TINY
    net = restorer(c, "fp32")
    waves = [x for x, _ in clips([4000] * 4, first=90)]
    x = torch.stack(waves).cuda()
    with torch.no_grad():
        mag, re, im = ops.stft(x, c["nfft"], c["hop"])
        uni = net(mag[:, None], re[:, None], im[:, None])
    rag = ragged_forward(net, waves, c)
    record_err("ragged_vs_uniform", rel(rag.cpu().numpy(), uni.cpu().numpy()), ALONE_LIMIT["fp32"])


def test_full_size_restorer_items_equal_clips_alone(record_err):
    """train.toml restorer size (F = 257, H = 384, bf16): cooperative / weight-stationary LSTM plans"""
    c = dict(F=257, sbn=15, sbh=384, nfft=512, hop=256, seed=5)
    net = restorer(c, "bf16")
    rng = np.random.default_rng(7)
    lengths = [int(n) for n in rng.integers(16000, 96000, size=8)]
    waves = [x for x, _ in clips(lengths, first=100)]
    out = ragged_forward(net, waves, c)
    worst = 0.0
    for b, w in enumerate(waves):
        Tb = 1 + lengths[b] // c["hop"]
        worst = max(worst, rel(out[b, :, :, :Tb].cpu().numpy(), alone_forward(net, w, c)[0].cpu().numpy()))
        assert bool((out[b, :, :, Tb:] == 0).all())
    record_err("batch_vs_alone", worst, ALONE_LIMIT["bf16_full"])
    assert torch.equal(out, ragged_forward(net, waves, c))


# ---------------------------------------------------------------------------------------------------- validator / trainer
def make_validator(tmp_path, groups=1):
    from nppc_audio.model_validator import ModelValidator, ModelValidatorConfig
    c = TINY
    ck = os.path.join(str(tmp_path), "restorer.tar")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in weights(c).items()}}, ck)
    cfg = ModelValidatorConfig(
        model_path=ck, model_configuration=dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                                num_groups_in_drop_band=groups, precision="fp32"),
        device="cuda", audio_config=dict(sr=16000, stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"],
                                                                            win_length=c["nfft"])))
    return ModelValidator(cfg)


def test_enhance_audio_lengths_matches_reference_one_clip_at_a_time(tmp_path, record_err):
    z = np.load(os.path.join(GOLD, "ragged_enh.npz"))
    meta = json.load(open(os.path.join(GOLD, "ragged_enh.json")))
    assert meta["stft"]["nfft"] == TINY["nfft"] and meta["model_config"]["num_freqs"] == TINY["F"]
    lengths = [int(n) for n in z["lengths"]]
    cut = np.cumsum([0] + lengths)
    noisy = [torch.from_numpy(z["noisy_pcm"][cut[i]:cut[i + 1]].astype(np.float32) / 32768.0) for i in range(len(lengths))]
    mv = make_validator(tmp_path)
    enh = mv.enhance_audio(padded(noisy).cuda(), lengths=lengths).cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lengths):
        worst = max(worst, rel(enh[b, :n], z["enhanced"][cut[b]:cut[b + 1]]))
        assert (enh[b, n:] == 0).all()
    record_err("enhanced_rel", worst, ENHANCE_REL)


def test_validate_dataloader_ragged_is_mean_of_oracle_metrics(tmp_path, record_err):
    from nppc_audio.data import RaggedBatch, pad_collate
    mv = make_validator(tmp_path)
    items = clips([16000, 9000, 12345, 20000, 7000], first=110)
    loader = [pad_collate(items[:3]), pad_collate(items[3:])]
    assert isinstance(loader[0], RaggedBatch)
    got = mv.validate_dataloader(loader)
    stoi, sdr = [], []
    for noisy, clean in items:
        enh = mv.enhance_audio(noisy.cuda())[0].cpu().numpy()
        stoi.append(SR.stoi(clean.numpy(), enh))
        sdr.append(SR.si_sdr_zero_mean(clean.numpy(), enh))
    # the alone enhancement and the ragged one differ by summation order only (ENHANCE_REL): the metrics follow
    record_err("validate_stoi_abs", abs(got["STOI"] - np.mean(stoi)), 1e-8)       # measured 4.0e-9
    record_err("validate_si_sdr_db", abs(got["SI_SDR"] - np.mean(sdr)), 1e-6)     # measured 4.0e-7


def test_validate_metrics_ragged_equals_one_clip_per_batch(tmp_path, record_err):
    from nppc_audio.data import pad_collate
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer, FullSubNetPlusTrainerConfig
    c = TINY
    cfg = FullSubNetPlusTrainerConfig(
        model_configuration=dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"],
                                 num_groups_in_drop_band=2, precision="fp32"),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]),
        dataloader_configuration=dict(batch_size=4, num_workers=0, pin_memory=False, shuffle=False), device="cuda")
    items = clips([16000, 9000, 12345, 20000, 7000], first=120)
    tr = FullSubNetPlusTrainer(cfg, dataset=[(n[:7000], cl[:7000]) for n, cl in items])
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights(c).items()}, strict=True)
    rag = tr.validate_metrics([pad_collate(items[:2]), pad_collate(items[2:])])
    one = tr.validate_metrics([(n[None], cl[None]) for n, cl in items])
    assert set(rag) == set(one)
    # measured: loss 1.3e-8 relative, STOI 1.1e-8, SI-SDR 6.4e-9 dB; the noisy scores see the same samples: 0
    record_err("loss_rel", abs(rag["loss"] - one["loss"]) / abs(one["loss"]), 3e-8)
    record_err("STOI", abs(rag["STOI"] - one["STOI"]), 2.2e-8)
    record_err("SI_SDR", abs(rag["SI_SDR"] - one["SI_SDR"]), 1.3e-8)
    for k in ("STOI_noisy", "SI_SDR_noisy"):
        record_err(k, abs(rag[k] - one[k]), 1e-12)


# ---------------------------------------------------------------------------------------------------- errors
def test_ragged_error_paths(tmp_path):
    from nppc_audio import ops
    c = TINY
    net = restorer(c, "fp32")
    x = torch.zeros(2, 4000).cuda()
    with pytest.raises(ValueError, match="item 1"):
        ops.stft(x, c["nfft"], c["hop"], lengths=[4000, 20])           # L_b <= nfft // 2
    with pytest.raises(ValueError, match="item 0"):
        ops.stft(x, c["nfft"], c["hop"], lengths=[4001, 3000])         # lengths > Lmax
    mv = make_validator(tmp_path)
    with pytest.raises(ValueError, match="item 1"):
        mv.enhance_audio(x, lengths=[4000, 100])                       # 4 frames < the TSSE kernel of 10
    mag, re, im = ops.stft(x, c["nfft"], c["hop"])
    with pytest.raises(RuntimeError, match="inference only"):
        with torch.enable_grad():
            net.requires_grad_(True)
            net(mag[:, None], re[:, None], im[:, None], frames=[126, 126])
    with pytest.raises(RuntimeError, match="inference only"):
        net.engine().forward([m[:, None] for m in (mag, re, im)], train=True,
                             frames=torch.tensor([126, 126], dtype=torch.int32, device="cuda"))
