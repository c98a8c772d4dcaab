"""CPU: the DNS dynamic-mixing dataset's host side (nppc_audio/dns_data.py) against items produced by the REFERENCE's own
Dataset.snr_mix / Dataset.__getitem__ (tests/golden/make_goldens_dns_mix.py): the fp64 restatement the GPU tests lean on,
the draws and the host items of DynamicMixDataset, config validation, file-backed construction, and the loud failure of
the device functions without a GPU.  Limits: 3 * e_ref (the reference's own fp32 error against the fp64 restatement, stored
per case by the maker), floored at 2^-23 of the peak."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import dns_mix_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "dns_mix.npz"))
    with open(os.path.join(GOLDEN, "dns_mix.json")) as f:
        meta = json.load(f)
    return z, meta


def pools(z, meta):
    return ([z[f"clean{i}"] for i in range(meta["n_clean"])], [z[f"noise{i}"] for i in range(meta["n_noise"])],
            [z[f"rir{i}"] for i in range(meta["n_rir"])])


def mix_inputs(z, meta, case):
    """the inputs the maker gave Dataset.snr_mix for one `mix` case: (clean [L], noise [L], rir 1-D or None)"""
    L = int(meta["sub_sample_length"] * meta["sr"])

    def fit(a):
        a = a[:L]
        return np.append(a, np.zeros(L - len(a), dtype=np.float32)) if len(a) < L else a
    clean = fit(z[f"clean{case['clean']}"])
    noise = np.zeros(L, dtype=np.float32) if case["noise"] is None else fit(np.tile(z[f"noise{case['noise']}"], 5))
    rir = None
    if case["rir"] is not None:
        rir = z[f"rir{case['rir']}"]
        rir = rir[case["channel"]] if case["channel"] >= 0 else rir
    return clean, noise, rir


def dataset(z, meta, floating, **kw):
    from nppc_audio.dns_data import DNSDatasetConfig, DynamicMixDataset
    clean, noise, rir = pools(z, meta)
    cfg = DNSDatasetConfig(snr_range=tuple(meta["snr_range"]), silence_length=meta["silence_length"],
                           target_dB_FS=meta["target_dB_FS"], target_dB_FS_floating_value=floating,
                           sub_sample_length=meta["sub_sample_length"], sr=meta["sr"], **kw)
    return DynamicMixDataset(cfg, clean_clips=clean, noise_clips=noise, rir_clips=rir)


def test_fixture_covers_the_cases(gold):
    z, meta = gold
    cases = meta["mix"] + meta["items"]
    assert all(abs(c["peak_before_guard"] - 0.999) > 1e-3 for c in cases)
    assert any(c["clipped"] for c in cases) and any(not c["clipped"] for c in cases)
    assert {c["floating"] for c in cases} == {3, 10}
    L = int(meta["sub_sample_length"] * meta["sr"])
    lens = {c["rir_len"] for c in meta["items"]}
    assert 0 in lens and 1 in lens and max(lens) > L
    assert any(c["channel"] >= 0 for c in cases)
    assert any(c["noise"] is None for c in meta["mix"])


def test_restatement_reproduces_the_reference(gold):
    z, meta = gold
    for case in meta["mix"]:
        clean, noise, rir = mix_inputs(z, meta, case)
        info = {}
        n64, c64 = M.snr_mix(clean, noise, case["snr"], meta["target_dB_FS"], case["level"], rir=rir, info=info)
        assert info["clipped"] == case["clipped"], case["name"]
        en, ec = M.rel_peak(z[f"mix.{case['name']}.noisy"], n64), M.rel_peak(z[f"mix.{case['name']}.clean"], c64)
        print(f"{case['name']}: noisy {en:.2e} (e_ref {case['e_ref_noisy']:.2e}), clean {ec:.2e} (e_ref {case['e_ref_clean']:.2e})")
        assert en < M.limit(case["e_ref_noisy"]) and ec < M.limit(case["e_ref_clean"]), case["name"]
        assert np.isfinite(n64).all() and np.isfinite(c64).all()


@pytest.mark.parametrize("floating", [3, 10])
def test_draws_and_items_equal_the_reference_items(gold, floating):
    """both generators in the state of the reference's globals -> the same decisions (exactly) and the same ingredients
    (CRC32 of the arrays the reference handed to snr_mix) -> the reference's (noisy, clean) within the fixture limit"""
    z, meta = gold
    ds = dataset(z, meta, floating)
    L = ds.config.crop_length
    cases = [c for c in meta["items"] if c["floating"] == floating]
    assert len(ds) == meta["n_clean"] and len(cases) >= 2 * len(ds)
    for case in cases:
        ds.rng.seed(case["seed"])
        ds.np_rng.seed(case["seed"])
        it = ds.draw(case["idx"])
        assert it.clean.shape == (L,) and it.noise.shape == (L,) and it.clean.dtype == np.float32
        assert (it.snr, it.level) == (case["snr"], case["level"]), case["key"]
        assert (0 if it.rir is None else len(it.rir)) == case["rir_len"], case["key"]
        assert crc(it.clean) == case["crc_clean"] and crc(it.noise) == case["crc_noise"], case["key"]
        assert (0 if it.rir is None else crc(it.rir)) == case["crc_rir"], case["key"]
        ds.rng.seed(case["seed"])
        ds.np_rng.seed(case["seed"])
        noisy, clean = ds[case["idx"]]
        assert noisy.dtype == np.float32 and clean.dtype == np.float32 and noisy.shape == (L,)
        en, ec = M.rel_peak(noisy, z[case["key"] + ".noisy"]), M.rel_peak(clean, z[case["key"] + ".clean"])
        assert en < M.limit(case["e_ref_noisy"]) and ec < M.limit(case["e_ref_clean"]), (case["key"], en, ec)


def test_seeded_stream_is_reproducible(gold):
    from nppc_audio.dns_data import DNSDatasetConfig, DynamicMixDataset
    z, meta = gold
    clean, noise, rir = pools(z, meta)
    cfg = DNSDatasetConfig(sub_sample_length=meta["sub_sample_length"], silence_length=meta["silence_length"])
    a = DynamicMixDataset(cfg, clean, noise, rir, seed=5)
    b = DynamicMixDataset(cfg, clean, noise, rir, seed=5)
    for i in (0, 3, 2):
        (na, ca), (nb, cb) = a[i], b[i]
        assert np.array_equal(na, nb) and np.array_equal(ca, cb)


def test_config_validation(gold):
    from nppc_audio.dns_data import DNSDatasetConfig, DynamicMixDataset
    z, meta = gold
    cfg = DNSDatasetConfig()                                        # train.toml's values
    assert cfg.snr_range == (-5, 20) and cfg.reverb_proportion == 0.75 and cfg.silence_length == 0.2
    assert (cfg.target_dB_FS, cfg.target_dB_FS_floating_value, cfg.sub_sample_length, cfg.sr) == (-25, 10, 3.072, 16000)
    assert cfg.crop_length == 49152 and cfg.snr_list == list(range(-5, 21))
    assert cfg.clean_dataset_limit is False and cfg.rir_dataset_offset == 0
    DNSDatasetConfig(pre_load_clean_dataset=True, pre_load_noise=True, pre_load_rir=True, num_workers=3)   # accepted
    for bad in (dict(reverb_proportion=1.5), dict(reverb_proportion=-0.1), dict(snr_range=(5, 0)), dict(snr_range=(1, 2, 3)),
                dict(snr_range=(0.5, 3))):
        with pytest.raises(ValueError):
            DNSDatasetConfig(**bad)
    # the reference's np.random.randint(t, t) raises ValueError at the first item; here at construction
    with pytest.raises(ValueError, match="low >= high"):
        np.random.RandomState(0).randint(-25, -25)
    with pytest.raises(ValueError, match="low >= high"):
        dataset(z, meta, 0)
    clean, noise, rir = pools(z, meta)
    with pytest.raises(ValueError, match="RIR"):
        DynamicMixDataset(DNSDatasetConfig(), clean, noise, [])
    DynamicMixDataset(DNSDatasetConfig(reverb_proportion=0), clean, noise, [])
    with pytest.raises(ValueError, match="1D"):
        DynamicMixDataset(DNSDatasetConfig(), [np.zeros((2, 100), dtype=np.float32)], noise, rir)


def test_file_backed_construction_keeps_rir_channels(gold, tmp_path):
    from scipy.io import wavfile
    from nppc_audio.dns_data import DNSDatasetConfig, DynamicMixDataset
    z, meta = gold
    clean, noise, rir = pools(z, meta)
    lists = {}
    for kind, clips in (("clean", clean), ("noise", noise), ("rir", rir)):
        paths = []
        for i, c in enumerate(clips):
            p = tmp_path / f"{kind}{i}.wav"
            wavfile.write(str(p), meta["sr"], np.ascontiguousarray(c.T))       # [n] or [n, C] float32
            paths.append(str(p))
        (tmp_path / f"{kind}.txt").write_text("\n".join(paths) + "\n")
        lists[kind] = str(tmp_path / f"{kind}.txt")
    cfg = DNSDatasetConfig(clean_dataset=lists["clean"], noise_dataset=lists["noise"], rir_dataset=lists["rir"],
                           clean_dataset_offset=1, clean_dataset_limit=3, sub_sample_length=meta["sub_sample_length"],
                           silence_length=meta["silence_length"])
    ds = DynamicMixDataset(cfg, seed=7)
    assert len(ds) == 3 and np.array_equal(ds.clean[0], clean[1]) and len(ds.noise) == len(noise)
    assert [r.shape for r in ds.rir] == [r.shape for r in rir] and np.array_equal(ds.rir[1], rir[1])
    mem = DynamicMixDataset(cfg, clean[1:4], noise, rir, seed=7)
    for i in range(3):
        (na, ca), (nb, cb) = ds[i], mem[i]
        assert np.array_equal(na, nb) and np.array_equal(ca, cb)


def test_loader_gathers_truncated_padded_rirs(gold):
    from nppc_audio.dns_data import DeviceReverbMixLoader
    z, meta = gold
    ds = dataset(z, meta, 10)
    ds.rng.seed(3)
    ds.np_rng.seed(3)
    ld = DeviceReverbMixLoader(ds, [[0, 1, 2, 3, 4, 5, 0, 1]], device="cpu", pin_memory=False)
    clean, noise, rir, rir_len, m = ld.gather([0, 1, 2, 3, 4, 5, 0, 1])
    L = ds.config.crop_length
    assert clean.shape == (8, L) and noise.shape == (8, L) and rir_len.dtype == torch.int32 and m.shape == (8, 2)
    assert rir.shape == (8, max(int(rir_len.max()), 1)) and int(rir_len.max()) <= L
    for b in range(8):
        assert not rir[b, int(rir_len[b]):].any()


def test_device_functions_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nppc_audio.dns_data import rir_convolve_on_device, snr_mix_on_device
    x = torch.zeros(2, 64)
    with pytest.raises(RuntimeError, match="HIP"):
        rir_convolve_on_device(x, torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP"):
        snr_mix_on_device(x, x, torch.zeros(2), torch.zeros(2))
