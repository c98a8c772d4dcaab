"""CPU: the specification of the inpainting dataset's energy voice-activity detector and gap draw (tests/vad_ref.py) on
constructed clips, the host side of nppc_audio.inpainting.data.AudioInpaintingDataset (folder scan, index remapping,
errors before any device work), the configuration round trip, and the guard that lets the GPU tests demand equality."""
import numpy as np
import pytest
import torch

import vad_ref as R

SR, MISS = 16000, 1024          # a gap of 64 ms: the constructed clips are half a second long
STFT = dict(nfft=63, hop_length=32, win_length=63)


def data_config(**kw):
    from nppc_audio.inpainting.trainer.nppc_trainer import AudioInpaintingConfig
    d = dict(clean_path=".", stft_configuration=STFT, sub_sample_length_seconds=0.5, missing_length_seconds=0.064, use_vad=True)
    d.update(kw)
    return AudioInpaintingConfig(**d)


# ---- the generator ---------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32-10
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert R.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert R.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_uniform_int_never_exceeds_n():
    for n in (0, 1, 2, 7, 1023, 30656, 2 ** 31 - 2):
        assert R.uniform_int(0, n) == 0 and R.uniform_int(0xFFFFFFFF, n) == n
        for u in (1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE):
            assert 0 <= R.uniform_int(u, n) <= n
    counts = np.bincount([R.uniform_int(R.draw(7, i, 0, R.OFFSET), 4) for i in range(5000)], minlength=5)
    assert counts.min() > 850 and counts.max() < 1150            # 1000 +- 5 sigma
    # the purposes and the epoch are separate streams
    words = {R.draw(7, 3, e, p) for e in (0, 1) for p in (R.CROP, R.SEGMENT, R.OFFSET, R.DBFS)}
    assert len(words) == 8


# ---- the detector on constructed clips ----------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [8000, 8192])
def test_constructed_clips(length):
    clips = R.six_clips(length)
    assert length == 8192 or length % 512                         # 8000: a tail that no window covers
    for name, (x, want) in clips.items():
        assert R.energy_vad(x, MISS) == want, name
        assert R.margin_db(x) >= 3.0, name
    x, _ = clips["merge"]
    assert len(R.energy_vad(x, MISS, min_silence_ms=0.0)) == 2     # without the hangover the 50 ms pause splits
    x, _ = clips["short"]
    assert R.energy_vad(x, 512)[0] == (1024, 1536)                 # a gap of 512 keeps the short burst
    x, _ = clips["flat"]
    assert R.energy_vad(x * 0, MISS) == [] and R.energy_vad(x[:300], 100) == []


def test_hysteresis_and_8khz():
    # a burst that sags to between theta_off and theta_on stays one segment; below theta_off for 300 ms it ends
    x = R.bursts(16384, [(1024, 8192)], 9)
    x[3072:6144] *= 10 ** (-37.5 / 20)                               # -62.5 dB: between -65 and -60
    assert R.margin_db(x) >= 1.0
    assert R.energy_vad(x, MISS) == [(1024, 8192)]
    x[3072:6144] *= 10 ** (-6 / 20)                                  # -68.5 dB: below theta_off
    assert R.energy_vad(x, MISS) == [(1024, 3072), (6144, 8192)]
    y = R.bursts(4096, [(512, 2304)], 10)
    assert R.energy_vad(y, 512, sample_rate=8000) == [(512, 2304)]   # windows of 256, min_silence 800 samples


# ---- gap bounds and the fallback rules ---------------------------------------------------------------------------------
def test_gap_rules():
    L = 8000
    segs = [(512, 4608), (6144, 7680)]
    seen = set()
    for i in range(400):
        g0, g1, fb = R.draw_gap(segs, L, MISS, 11, i)
        assert fb == 0 and g1 - g0 == MISS
        k = [s for s in segs if s[0] <= g0 and g1 <= s[1]]
        assert len(k) == 1
        seen.add(k[0])
        assert R.draw_gap(segs, L, MISS, 11, i) == (g0, g1, fb)    # a function of (seed, item, epoch)
    assert seen == set(segs)
    assert any(R.draw_gap(segs, L, MISS, 11, i, epoch=1) != R.draw_gap(segs, L, MISS, 11, i) for i in range(8))
    for i in range(200):
        # no segment, a segment exactly as long as the gap, use_vad off: the random fallback, inside the clip
        for s, vad in (([], True), ([(1024, 1024 + MISS)], True), (segs, False)):
            g0, g1, fb = R.draw_gap(s, L, MISS, 5, i, use_vad=vad)
            assert fb == 1 and 0 <= g0 and g1 == g0 + MISS <= L
    starts = {R.draw_gap([], L, MISS, 5, i)[0] for i in range(200)}
    assert min(starts) < 700 and max(starts) > L - MISS - 700
    # missing_start_seconds fixes the fallback only: a usable segment still wins with use_vad, never without
    assert R.draw_gap([], L, MISS, 5, 0, missing_start=3200) == (3200, 3200 + MISS, 1)
    assert R.draw_gap(segs, L, MISS, 5, 0, missing_start=3200, use_vad=False) == (3200, 3200 + MISS, 1)
    g0, g1, fb = R.draw_gap(segs, L, MISS, 5, 0, missing_start=3200)
    assert fb == 0 and g0 != 3200
    # a segment one sample longer than the gap has two positions
    assert {R.draw_gap([(100, 101 + MISS)], L, MISS, 3, i)[0] for i in range(64)} == {100, 101}


def test_item_crop_and_level():
    x = R.bursts(20000, [(6000, 14000)], 12)
    it = R.item(x, 1.5, 8000, MISS, 21, 4)
    assert 0 <= it["crop_start"] <= 12000 and it["clean"].dtype == np.float32
    assert np.array_equal(it["clean"], x[it["crop_start"]:it["crop_start"] + 8000] * np.float32(1.5))
    assert R.item(x, 1.5, 8000, MISS, 21, 4, random_crop=False)["crop_start"] == 0
    assert R.item(x[:8000], 1.5, 8000, MISS, 21, 4)["crop_start"] == 0
    gains = [float(R.level_gain(10.0, 21, i)) for i in range(300)]
    assert 10 ** -0.5 <= min(gains) < 0.4 and 2.5 < max(gains) <= 10 ** 0.5 and R.level_gain(0.0, 21, 0) == 1.0


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------
def gpu_case_files(length, n, seed):
    """n files of 1.5 x length samples with bursts at arbitrary (not window-aligned) positions"""
    rng = np.random.Generator(np.random.PCG64(seed))
    files = []
    for i in range(n):
        flen, spans, pos = length + length // 2, [], int(rng.integers(0, length // 4))
        while pos < flen - 2000:
            dur = int(rng.integers(1500, max(length // 3, 3000)))
            spans.append((pos, min(pos + dur, flen)))
            pos += dur + int(rng.integers(500, max(length // 4, 6000)))
        files.append(R.bursts(flen, spans, seed * 100 + i))
    return files


GPU_CASES = [(40000, 3, 30), (320000, 2, 30)]        # (L, files, seed) of tests/test_inpaint_dataset_gpu.py
GPU_SEED = 2024
PINNED_SEED = 77                                     # config.seed of the GPU test that pins its items (first case, epoch 0)


def whole_file_gain(x, target=-25.0):
    t = torch.from_numpy(x)
    return float(10 ** ((target - 20 * torch.log10(t.pow(2).mean().sqrt() + 1e-8)) / 20))


def test_gpu_inputs_keep_3db_from_both_thresholds():
    """what lets the GPU tests demand exact equality: under the restatement every window level of every item they use lies
    at least 3 dB from theta_on and theta_off (and peak - floor at least 3 dB from on_db), so an fp64 rounding of a level
    cannot change a decision"""
    for x, _ in R.six_clips(8000).values():
        assert R.margin_db(x * np.float32(whole_file_gain(x))) >= 3.0
    for L, n, seed in GPU_CASES:
        some_segments = 0
        for i, x in enumerate(gpu_case_files(L, n, seed)):
            for epoch in (0, 1):
                it = R.item(x, whole_file_gain(x), L, 2048, GPU_SEED, i, epoch)
                assert R.margin_db(it["clean"]) >= 3.0, (L, i, epoch)
                some_segments += len(it["segments"])
        assert some_segments >= n
    L, n, seed = GPU_CASES[0]
    for i, x in enumerate(gpu_case_files(L, n, seed)):
        assert R.margin_db(R.item(x, whole_file_gain(x), L, 2048, PINNED_SEED, i, 0)["clean"]) >= 3.0, i


# ---- the host side of the dataset --------------------------------------------------------------------------------------
def test_config_round_trip():
    from nppc_audio.inpainting.vad import EnergyVadConfig
    from nppc_audio.inpainting.trainer.nppc_trainer import AudioInpaintingConfig
    plain = data_config()
    assert plain.vad_configuration is None
    assert AudioInpaintingConfig(**plain.model_dump(mode="json")) == plain
    tuned = data_config(vad_configuration=dict(on_db=12.0, min_silence_ms=60.0))
    assert tuned.vad_configuration == EnergyVadConfig(on_db=12.0, min_silence_ms=60.0)
    assert AudioInpaintingConfig(**tuned.model_dump(mode="json")) == tuned
    d = EnergyVadConfig()
    assert (d.on_db, d.range_db, d.hysteresis_db, d.floor_percentile, d.min_silence_ms) == (15.0, 40.0, 5.0, 0.10, 100.0)
    assert d.min_silence_samples(16000) == 1600
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS
    with pytest.raises(pydantic_error()):
        EnergyVadConfig(floor_percentile=1.5)
    # the trainer configurations carry it and still round-trip
    from test_restoration_cpu import yaml_config
    from nppc_audio.inpainting.trainer.restoration_trainer import InpaintingTrainerConfig
    cfg = yaml_config()
    d = cfg.model_dump(mode="json")
    assert d["data_configuration"]["vad_configuration"] is None and InpaintingTrainerConfig(**d) == cfg
    d["data_configuration"]["vad_configuration"] = dict(range_db=35.0)
    assert InpaintingTrainerConfig(**InpaintingTrainerConfig(**d).model_dump(mode="json")).data_configuration \
        .vad_configuration.range_db == 35.0


def pydantic_error():
    import pydantic
    return pydantic.ValidationError


def test_empty_or_missing_folder_raises_before_the_device(tmp_path):
    from nppc_audio.inpainting.data import AudioInpaintingDataset
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer, NPPCAudioInpaintingTrainerConfig
    with pytest.raises(ValueError, match="dataset="):
        AudioInpaintingDataset(data_config(clean_path=str(tmp_path)))
    with pytest.raises(ValueError, match="dataset="):
        AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "nowhere")))
    (tmp_path / "a.flac").write_bytes(b"fLaC")
    with pytest.raises(ValueError, match="(?s)flac decoder.*dataset="):
        AudioInpaintingDataset(data_config(clean_path=str(tmp_path)))
    cfg = NPPCAudioInpaintingTrainerConfig(
        nppc_model_configuration=dict(
            pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2),
            pretrained_restoration_model_path=str(tmp_path / "no_such_checkpoint.pt"),
            audio_pc_wrapper_configuration=dict(n_dirs=2, model_configuration=dict(in_channels=2, out_channels=2)),
            device="cuda"),
        data_configuration=data_config(clean_path=str(tmp_path / "nowhere")).model_dump(),
        dataloader_configuration=dict(batch_size=2, num_workers=0, pin_memory=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4)), device="cuda")
    with pytest.raises(ValueError, match="dataset="):               # before the model, its checkpoint or the device
        NPPCAudioInpaintingTrainer(cfg)


def test_wav_folder_and_short_file_remapping(tmp_path):
    from scipy.io import wavfile
    from nppc_audio.inpainting.data import AudioInpaintingDataset
    rng = np.random.Generator(np.random.PCG64(3))
    lens = [3000, 9000, 2000, 1000, 8000, 500]                      # L = 8000: files 1 and 4 are usable
    for i, n in enumerate(lens):
        wavfile.write(str(tmp_path / f"clip{i}.wav"), SR, (rng.standard_normal(n) * 3000).astype(np.int16))
    ds = AudioInpaintingDataset(data_config(clean_path=str(tmp_path)))
    assert len(ds) == 6 and [c.numel() for c in ds.clean] == lens
    assert ds.file_of == [1, 1, 4, 4, 4, 1]                         # the next usable file, cyclically
    assert ds.sub_sample_length == 8000 and ds.missing_length == 1024 and not ds.fixed_items
    # the whole-file gain brings every file to -25 dBFS
    for c, g in zip(ds.clean, ds.gain):
        assert abs(20 * np.log10(float((c * g).pow(2).mean().sqrt())) + 25.0) < 1e-3
    # tensor-backed, pinned by config.seed; an entropy seed differs from run to run
    clips = [torch.zeros(n) + 0.01 for n in lens]
    a = AudioInpaintingDataset(data_config(seed=5), clean_clips=clips)
    assert a.fixed_items and a.seed == 5 and a.file_of == ds.file_of
    assert AudioInpaintingDataset(data_config(), clean_clips=clips, seed=9).seed == 9
    assert AudioInpaintingDataset(data_config(), clean_clips=clips).seed != AudioInpaintingDataset(data_config(), clean_clips=clips).seed
    with pytest.raises(ValueError, match="dataset="):
        AudioInpaintingDataset(data_config(), clean_clips=[torch.zeros(100)])
    with pytest.raises(ValueError, match="missing_start_seconds"):
        AudioInpaintingDataset(data_config(missing_start_seconds=0.45), clean_clips=clips)
    with pytest.raises(ValueError, match="windows"):
        AudioInpaintingDataset(data_config(sub_sample_length_seconds=70.0), clean_clips=[torch.zeros(70 * SR)])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):              # the batch path is HIP-only
            ds[0]
