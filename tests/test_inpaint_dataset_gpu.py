"""GPU: the inpainting dataset on the device (csrc/inpaint_data.hip, nppc_audio/inpainting/{vad,data}.py) against the
fp64 restatement tests/vad_ref.py -- exact equality, which test_inpaint_dataset_cpu.py's 3 dB guard on these very inputs
permits -- its bit-exactness contracts, and both inpainting trainers and the validator running from a wav folder."""
import os

import numpy as np
import pytest
import torch

import vad_ref as R
from oracle import weights as W
from test_inpaint_dataset_cpu import GPU_CASES, GPU_SEED, PINNED_SEED, gpu_case_files

pytestmark = pytest.mark.gpu
SR = 16000


def data_config(L, missing, nfft, hop, **kw):
    from nppc_audio.inpainting.trainer.nppc_trainer import AudioInpaintingConfig
    d = dict(clean_path=".", stft_configuration=dict(nfft=nfft, hop_length=hop, win_length=nfft),
             sub_sample_length_seconds=L / SR, missing_length_seconds=missing / SR, use_vad=True)
    d.update(kw)
    cfg = AudioInpaintingConfig(**d)
    assert int(cfg.sub_sample_length_seconds * SR) == L and int(cfg.missing_length_seconds * SR) == missing
    return cfg


def make_case(name):
    """-> (files fp32, config kwargs): 'six' = the six constructed clips at L = 8000 (15 windows and an ignored tail), then
    the (L, files, seed) of GPU_CASES: 78 windows (more than one wave of windows) and 625 (a sort of several passes)"""
    if name == "six":
        return [x for x, _ in R.six_clips(8000).values()], dict(L=8000, missing=1024, nfft=63, hop=32)
    L, n, seed = GPU_CASES[name]
    return gpu_case_files(L, n, seed), dict(L=L, missing=2048, nfft=255, hop=128)


@pytest.fixture(scope="module", params=["six", 0, 1], ids=["B6_L8000", "B3_L40000", "B2_L320000"])
def case(request):
    from nppc_audio.inpainting.data import AudioInpaintingDataset, InpaintingDeviceLoader
    files, kw = make_case(request.param)
    ds = AudioInpaintingDataset(data_config(**kw), clean_clips=[torch.from_numpy(f) for f in files], seed=GPU_SEED)
    loader = InpaintingDeviceLoader(ds, [list(range(len(files)))])
    want = {e: [R.item(f, float(ds.gain[i]), kw["L"], kw["missing"], GPU_SEED, i, e) for i, f in enumerate(files)]
            for e in (0, 1)}                                     # the reference, once, shared
    return request.param, files, kw, ds, loader, want


def seg_table(items, S):
    t = -np.ones((len(items), S, 2), dtype=np.int32)
    for b, it in enumerate(items):
        for k, s in enumerate(it["segments"]):
            t[b, k] = s
    return t


def test_batch_equals_the_restatement(case):
    name, files, kw, ds, loader, want = case
    idxs = list(range(len(files)))
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        *_, meta = loader.batch(idxs)
        torch.cuda.synchronize()
        w = want[epoch]
        got = {k: v.cpu().numpy() for k, v in meta.items()}
        assert got["n_segments"].tolist() == [len(it["segments"]) for it in w]
        assert np.array_equal(got["segments"], seg_table(w, got["segments"].shape[1]))
        for k in ("gap_start", "gap_end", "used_fallback", "crop_start"):
            assert got[k].tolist() == [it[k] for it in w], (k, epoch)
        assert got["file_index"].tolist() == idxs
        assert np.array_equal(got["clean_audio"], np.stack([it["clean"] for it in w]))
        # every non-fallback gap lies inside one of its item's segments
        for b in range(len(files)):
            if got["used_fallback"][b] == 0:
                segs = got["segments"][b, :got["n_segments"][b]]
                assert any(s <= got["gap_start"][b] and got["gap_end"][b] <= e for s, e in segs), b
            assert 0 <= got["gap_start"][b] and got["gap_end"][b] == got["gap_start"][b] + kw["missing"] <= kw["L"]
    if name == "six":
        assert [it["segments"] for it in want[0]] == [s for _, s in R.six_clips(8000).values()]
        assert [it["used_fallback"] for it in want[0]] == [0, 0, 0, 0, 1, 0]
    else:
        assert sum(len(it["segments"]) > 1 for it in want[0]) >= 1 and any(it["crop_start"] > 0 for it in want[0])


def test_spectra_are_those_of_inpainting_batch_on_device(case):
    from nppc_audio.inpainting.data import inpainting_batch_on_device
    name, files, kw, ds, loader, want = case
    loader.set_epoch(0)
    stft_masked, mask_frames, stft_clean, masked_audio, meta = loader.batch(list(range(len(files))))
    ref = inpainting_batch_on_device(meta["clean_audio"], meta["gap_start"], meta["gap_end"], nfft=kw["nfft"],
                                     hop_length=kw["hop"], normalize=False)
    F, T = kw["nfft"] // 2 + 1, 1 + kw["L"] // kw["hop"]
    assert stft_masked.shape == (len(files), 2, F, T) and masked_audio.shape == (len(files), 1, kw["L"])
    for a, b in zip((stft_masked, mask_frames, stft_clean, masked_audio), ref):
        assert a.shape == b.shape and torch.equal(a, b)
    gap = (mask_frames == 0).sum(1)
    assert int(gap.min()) >= 1 and bool(torch.isfinite(stft_clean).all())


def test_an_item_does_not_depend_on_its_batch(case):
    name, files, kw, ds, loader, want = case
    n = len(files)
    loader.set_epoch(0)
    full = loader.batch(list(range(n)))
    again = loader.batch(list(range(n)))                        # the same seed and epoch: identical batches
    for a, b in zip(full[:4], again[:4]):
        assert torch.equal(a, b)
    for k in full[4]:
        assert torch.equal(full[4][k], again[4][k]), k
    order = list(reversed(range(n)))
    for idxs in ([n - 1], order):
        part = loader.batch(idxs)
        for a, b in zip(full[:4], part[:4]):
            assert torch.equal(a[idxs], b)
        for k in full[4]:
            assert torch.equal(full[4][k][idxs], part[4][k]), k
    one = ds[n - 1]                                              # a batch of one through the same path
    for a, b in zip(full[:4], one):
        assert torch.equal(a[n - 1], b)
    # another epoch changes the gaps when config.seed is unset ...
    loader.set_epoch(1)
    other = loader.batch(list(range(n)))
    assert not torch.equal(other[4]["gap_start"], full[4]["gap_start"])
    loader.set_epoch(0)


def test_config_seed_pins_the_items():
    from nppc_audio.inpainting.data import AudioInpaintingDataset, InpaintingDeviceLoader
    files, kw = make_case(0)
    clips = [torch.from_numpy(f) for f in files] + [torch.zeros(100)]          # index 3 is too short: it maps to file 0
    ds = AudioInpaintingDataset(data_config(seed=PINNED_SEED, **kw), clean_clips=clips, seed=5)
    assert ds.file_of == [0, 1, 2, 0]
    loader = InpaintingDeviceLoader(ds, [[0, 1], [2, 3]])
    batches = list(loader)
    assert len(loader) == 2 and len(batches) == 2 and batches[1][4]["file_index"].tolist() == [2, 0]
    loader.set_epoch(3)
    for a, b in zip(batches, list(loader)):                                    # the epoch is held at 0
        assert torch.equal(a[0], b[0]) and torch.equal(a[4]["gap_start"], b[4]["gap_start"])
    assert torch.equal(batches[0][0][0], batches[1][0][1])                     # item 3 IS item 0, like the reference's recursion
    w = R.item(files[0], float(ds.gain[0]), kw["L"], kw["missing"], PINNED_SEED, 0, 0)
    m = batches[1][4]
    assert (int(m["crop_start"][1]), int(m["gap_start"][1]), int(m["used_fallback"][1])) == \
        (w["crop_start"], w["gap_start"], w["used_fallback"])
    with pytest.raises(IndexError):
        loader.batch([4])


def test_energy_vad_draw_gaps_and_options():
    from nppc_audio import _hip as H
    from nppc_audio.inpainting.data import AudioInpaintingDataset, InpaintingDeviceLoader
    from nppc_audio.inpainting.vad import EnergyVadConfig, draw_gaps, energy_vad
    clips = R.six_clips(8000)
    wave = torch.from_numpy(np.stack([x for x, _ in clips.values()])).cuda()
    segments, n_segments = energy_vad(wave, 1024)
    want = [s for _, s in clips.values()]
    assert n_segments.tolist() == [len(s) for s in want]
    assert [[tuple(p) for p in segments[b, :len(s)].tolist()] for b, s in enumerate(want)] == want
    assert int(segments[4].max()) == -1
    # other constants reach the kernel: without the hangover the 50 ms pause of 'merge' splits
    seg0, n0 = energy_vad(wave[:1], 1024, EnergyVadConfig(min_silence_ms=0.0))
    assert [tuple(p) for p in seg0[0, :int(n0[0])].tolist()] == R.energy_vad(clips["merge"][0], 1024, min_silence_ms=0.0)
    index = torch.tensor([7, 8, 9, 10, 11, 12], dtype=torch.int32)
    for kw in (dict(epoch=0), dict(epoch=2), dict(epoch=0, missing_start=3200)):
        g0, g1, fb = draw_gaps(segments, n_segments, 8000, 1024, 99, index, **kw)
        ref = [R.draw_gap(s, 8000, 1024, 99, int(i), **kw) for s, i in zip(want, index)]
        assert list(zip(g0.tolist(), g1.tolist(), fb.tolist())) == ref
    # use_vad off and a fixed start: always the fallback; the level float scales the crop by the drawn factor
    files, kw = make_case("six")
    tens = [torch.from_numpy(f) for f in files]
    ds = AudioInpaintingDataset(data_config(use_vad=False, missing_start_seconds=0.2, **kw), clean_clips=tens, seed=3)
    m = InpaintingDeviceLoader(ds, None).batch([0, 1, 2, 3, 4, 5])[4]
    assert m["gap_start"].tolist() == [3200] * 6 and m["used_fallback"].tolist() == [1] * 6 and m["n_segments"].tolist() == [0] * 6
    ds = AudioInpaintingDataset(data_config(target_dB_FS_floating_value=10.0, **kw), clean_clips=tens, seed=3)
    m = InpaintingDeviceLoader(ds, None).batch([0, 1, 2, 3, 4, 5])[4]
    w = [R.item(f, float(ds.gain[i]), 8000, 1024, 3, i, 0, dbfs_float=10.0) for i, f in enumerate(files)]
    ref = np.stack([it["clean"] for it in w])
    # the factor's pow may differ in its last fp64 bit: at most one fp32 ulp each on the factor, the gain and the sample
    assert np.all(np.abs(m["clean_audio"].cpu().numpy() - ref) <= 3 * 2.0 ** -23 * np.abs(ref))
    assert m["gap_start"].tolist() == [it["gap_start"] for it in w]
    assert len({round(float(R.level_gain(10.0, 3, i)), 3) for i in range(6)}) == 6
    # host tensors are refused, not handed to a kernel
    with pytest.raises(ValueError, match="device"):
        energy_vad(wave.cpu(), 1024)
    with pytest.raises(ValueError, match="device"):
        draw_gaps(segments.cpu(), n_segments, 8000, 1024, 99, index)
    with pytest.raises(ValueError, match="device"):
        draw_gaps(segments, n_segments.cpu(), 8000, 1024, 99, index)
    # above 2048 windows: the C entry answers unsupported before any launch, the Python layer raises
    z = torch.zeros(1, 2049 * 512, device="cuda")
    with pytest.raises(ValueError, match="windows"):
        energy_vad(z, 2048)
    o = torch.zeros(2, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(2050, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        H.call("nppc_inpaint_vad_batch", z, z.numel(), o, z, 1, i32, i32, 1, z.numel(), 512, 2048, -1, 1, 0, 0, 0, 0.0, 15.0,
               40.0, 5.0, 0.1, 1600, 1024, None, None, i32, i32, i32, i32, i32, H.stream())


# ---- the trainers and the validator from a wav folder -----------------------------------------------------------------------
KDIR, NFFT, HOP, LTR = 3, 63, 32, 8192


@pytest.fixture(scope="module")
def wav_folder(tmp_path_factory):
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("inpaint_wavs")
    for i in range(6):
        x = R.bursts(12000, [(1000 + 300 * i, 5200), (7600, 10500 + 200 * i)], 50 + i)
        wavfile.write(str(d / f"clip{i}.wav"), SR, np.round(x / np.abs(x).max() * 30000).astype(np.int16))
    return d


def trainer_config(folder, tmp, batch_size):
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainerConfig
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(KDIR), 41).items()}
    pre = "pretrained_restoration_model.net."
    ck = os.path.join(str(tmp), "restorer.pt")
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    return NPPCAudioInpaintingTrainerConfig(
        nppc_model_configuration=dict(
            pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
            pretrained_restoration_model_path=ck,
            audio_pc_wrapper_configuration=dict(n_dirs=KDIR, model_configuration=dict(in_channels=2, out_channels=KDIR,
                                                                                      precision="fp32")),
            device="cuda"),
        data_configuration=data_config(LTR, 1024, NFFT, HOP, clean_path=str(folder)).model_dump(),
        dataloader_configuration=dict(batch_size=batch_size, num_workers=0, pin_memory=False, shuffle=True),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.5, 0.999])), device="cuda"), wts


def test_successive_passes_of_the_trainers_loader(wav_folder):
    """without config.seed every pass over the folder cuts other crops and places other gaps, as the reference's unseeded
    __getitem__ does on every visit; config.seed pins every item, pass after pass"""
    from nppc_audio.data import DataLoaderConfig
    from nppc_audio.inpainting.trainer.nppc_trainer import build_device_loader
    from nppc_audio.trainer import LoopLoader
    dl = DataLoaderConfig(batch_size=4, num_workers=0, pin_memory=False, shuffle=False)

    def passes(**kw):
        _, loader = build_device_loader(data_config(LTR, 1024, NFFT, HOP, clean_path=str(wav_folder), **kw), dl, "cuda")
        assert len(loader) == 2
        got = [b[4] for b in LoopLoader(loader, n_epochs=3)]                # the trainers' loop: three passes of two batches
        assert len(got) == 6 and all(g["file_index"].tolist() == got[i % 2]["file_index"].tolist() for i, g in enumerate(got))
        return [{k: torch.cat([got[2 * p][k], got[2 * p + 1][k]]) for k in ("crop_start", "gap_start")} for p in range(3)]

    free = passes()
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(free[a]["crop_start"], free[b]["crop_start"])
        assert not torch.equal(free[a]["gap_start"], free[b]["gap_start"])
    pinned = passes(seed=PINNED_SEED)
    for p in (1, 2):
        assert torch.equal(pinned[0]["crop_start"], pinned[p]["crop_start"])
        assert torch.equal(pinned[0]["gap_start"], pinned[p]["gap_start"])


def test_nppc_trainer_and_validator_from_a_wav_folder(wav_folder, tmp_path):
    """NPPCAudioInpaintingTrainer(config) with no dataset=: two steps, then validate_dataloader over the trainer's own
    loader (n_components = the model's 3 directions, which the validator requires to match)."""
    from nppc_audio.inpainting.data import InpaintingDeviceLoader
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    cfg, wts = trainer_config(wav_folder, tmp_path, 3)
    tr = NPPCAudioInpaintingTrainer(cfg)
    assert isinstance(tr.dataloader, InpaintingDeviceLoader) and len(tr.dataloader) == 2 and len(tr.dataloader.dataset) == 6
    tr.nppc_model.load_state_dict(wts, strict=True)
    tr.nppc_model.to("cuda")
    objs, step = [], tr.train_step

    def recording_step(batch):
        out = step(batch)
        objs.append(float(out[1].detach()))
        return out

    tr.train_step = recording_step
    tr.train(n_steps=2, checkpoint_dir=str(tmp_path / "ck"), save_flag=False)
    assert tr.step == 2 and len(objs) == 2 and all(np.isfinite(objs))
    batch = next(iter(tr.dataloader))
    assert batch[0].shape == (3, 2, NFFT // 2 + 1, 1 + LTR // HOP) and int(batch[4]["n_segments"].min()) >= 1
    ck = str(tmp_path / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    val = V.NPPCModelValidator(V.NPPCModelValidatorConfig(
        checkpoint_path=ck, save_dir=None, model_configuration=tr.config.nppc_model_configuration.model_dump()))
    res = val.validate_dataloader(tr.dataloader, n_mc_samples=4, n_components=KDIR, ragged_gaps=True)
    assert res["n_items"] == 6 and len(res["per_item"]) == 6
    for m in res["per_item"]:
        assert np.isfinite(m["nppc"]["rmse"]) and np.isfinite(m["mc_dropout"]["rmse"])


def test_restoration_trainer_from_a_wav_folder(wav_folder, tmp_path):
    from nppc_audio.inpainting.data import InpaintingDeviceLoader
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainer, InpaintingTrainerConfig
    cfg = InpaintingTrainerConfig(
        model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
        data_configuration=data_config(LTR, 1024, NFFT, HOP, clean_path=str(wav_folder)).model_dump(),
        dataloader_configuration=dict(batch_size=3, num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.5, 0.999])), device="cuda")
    tr = InpaintingTrainer(cfg)
    assert isinstance(tr.dataloader, InpaintingDeviceLoader)
    losses = tr.train(n_steps=2, checkpoint_dir=str(tmp_path / "ck"))
    assert tr.step == 2 and len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses)
