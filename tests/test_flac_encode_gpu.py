"""GPU: the FLAC encoder kernels (csrc/flac_enc.hip) give byte for byte what the serial host encoder and the restatement
tests/flac_enc_ref.py give, in ragged batches of mono and stereo files, file by file and run after run; the device decoder
reads the streams back; and the places that write audio (encode_waves, save_pc_audio_variations, restore_file) write it.

A call has one sample size, rate and block size, so the shapes of tests/flac_enc_cases.py go in one batch per (block size,
rate): the 4096 / 16000 batch holds the main file (constant, verbatim and partitioned frames), the spike frame, the stereo
file with the four assignments, every short length and the finest partitions; the block-size-16 batch holds the 130- and
2050-frame files.  Every test runs under a time limit of its own: a hang ends the process with a traceback."""
import faulthandler

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import flac_enc_cases as K
import flac_ref as R
from nppc_audio import _hip as H
from nppc_audio import flac

pytestmark = pytest.mark.gpu
LIMIT = 120


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def batches(bps):
    groups = {}
    for c in K.cases(bps):
        groups.setdefault((c.block_size, c.rate), []).append(c)
    return groups


def encode_device(cs, **kw):
    return flac.encode_pcm([torch.from_numpy(c.pcm).cuda() for c in cs], cs[0].bps, cs[0].rate, cs[0].block_size, backend="hip",
                           **kw)


@pytest.fixture(scope="module")
def encoded16():
    """{(block size, rate): (cases, device streams)} at 16 bits, encoded once and shared (read-only)"""
    return {key: (cs, encode_device(cs)) for key, cs in batches(16).items()}


def check_batches(bps, done):
    assert {len(cs) for cs, _ in done.values()} >= {1, 2} and max(len(cs) for cs, _ in done.values()) >= 10
    assert {c.pcm.shape[0] for c in done[(4096, 16000)][0]} == {1, 2}              # mono and stereo in one batch
    for cs, got in done.values():
        host = flac.encode_pcm([torch.from_numpy(c.pcm) for c in cs], bps, cs[0].rate, cs[0].block_size, backend="host")
        for c, g, h in zip(cs, got, host):
            assert g == h, f"{c.name}: device and host differ (first at byte {first_diff(g, h)})"
            assert g == K.reference(bps, c.name)[0], c.name
        assert encode_device(cs) == got                                            # run after run
        for c, g in zip(cs, got):
            assert encode_device([c]) == [g], f"{c.name}: alone it gives other bytes than in the batch"


def first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def test_ragged_batches_equal_host_and_restatement_16_bits(encoded16):
    check_batches(16, encoded16)


def test_ragged_batches_equal_host_and_restatement_24_bits():
    check_batches(24, {key: (cs, encode_device(cs)) for key, cs in batches(24).items()})


def test_the_device_decoder_reads_the_streams_back(encoded16):
    for cs, got in encoded16.values():
        pcm, infos = flac.decode_files(got, out="pcm", backend="hip", verify_md5=True)
        for c, p, i in zip(cs, pcm, infos):
            assert np.array_equal(p.numpy(), c.pcm), c.name
            assert (i.sample_rate, i.channels, i.bits_per_sample, i.min_blocksize) == (c.rate, c.pcm.shape[0], 16, c.block_size)


def test_host_tensors_and_value_checks_on_the_device_path():
    c = {c.name: c for c in K.cases(16)}["main"]
    assert flac.encode_pcm([torch.from_numpy(c.pcm)], 16, backend="hip") == [K.reference(16, "main")[0]]
    with pytest.raises(ValueError):
        flac.encode_pcm([torch.full((1, 9), 32768, dtype=torch.int32).cuda()], 16, backend="hip")
    with pytest.raises(ValueError):
        flac.encode_pcm([torch.zeros(3, 9, dtype=torch.int32).cuda()], 16, backend="hip")


@pytest.mark.parametrize("bits", [16, 24])
def test_encode_waves_equals_encode_pcm_of_the_numpy_quantised_samples(bits):
    rng = np.random.default_rng(5)
    full, eps = 1 << (bits - 1), float(np.spacing(np.float32(1.0)))
    x = (0.3 * rng.standard_normal((5, 6000))).astype(np.float32)
    edge = np.array([1.0, -1.0, 1.0 - eps / 2, -1.0 - eps, 1.0 + eps, (full - 0.5) / full, -(full - 0.5) / full, 0.5 / full,
                     1.5 / full, 2.5 / full, -0.5 / full, -1.5 / full, -2.5 / full, 3.0, -3.0, np.nan, np.inf, -np.inf], np.float32)
    x[1, :edge.size] = edge
    lens = [6000, 4097, 1, 17, 4096]
    q = flac.quantize_waves_host(x, bits)
    assert q[1, :2].tolist() == [full - 1, -full] and q[1, 7:10].tolist() == [0, 2, 2] and q[1, 15] == 0
    got = flac.encode_waves(torch.from_numpy(x).cuda(), lens, 22050, bits, backend="hip")
    want = flac.encode_pcm([torch.from_numpy(q[v:v + 1, :n].copy()) for v, n in enumerate(lens)], bits, 22050, backend="host")
    assert got == want
    assert flac.encode_waves(torch.from_numpy(x), lens, 22050, bits, backend="host") == want
    back, _ = flac.decode_files(got, out="pcm", backend="hip", verify_md5=True)
    assert all(np.array_equal(b.numpy()[0], q[v, :n]) for v, (b, n) in enumerate(zip(back, lens)))


def test_save_pc_audio_variations_writes_the_layout(tmp_path):
    from nppc_audio.inpainting.validator.validator_nppc_model import save_pc_audio_variations
    B, KD, A, L = 2, 2, 3, 2044
    g = torch.Generator().manual_seed(3)
    out = {"audio_variations": (0.4 * torch.randn(B, KD, A, L, generator=g)).cuda(),
           "clean_audio": (0.4 * torch.randn(B, L, generator=g)).cuda(),
           "audio_variations_blind": (0.4 * torch.randn(B, KD, A, L, generator=g)).cuda()}
    alphas = [-1.5, 0.0, 2.0]
    paths = save_pc_audio_variations(out, tmp_path / "v", alphas, first_index=7)
    want = {}
    for b in range(B):
        d = tmp_path / "v" / f"sample_{7 + b}"
        want[d / "clean.flac"] = out["clean_audio"][b]
        for k in range(KD):
            for a, alpha in enumerate(alphas):
                want[d / f"pc_{k + 1}" / f"alpha_{alpha:.1f}.flac"] = out["audio_variations"][b, k, a]
                want[d / f"pc_{k + 1}" / f"alpha_{alpha:.1f}_blind.flac"] = out["audio_variations_blind"][b, k, a]
    assert sorted(map(str, paths)) == sorted(map(str, want)) == sorted(str(p) for p in (tmp_path / "v").rglob("*") if p.is_file())
    assert (tmp_path / "v" / "sample_8" / "pc_2" / "alpha_-1.5_blind.flac").exists()
    names = list(want)
    pcm, infos = flac.decode_files(names, out="pcm", backend="hip", verify_md5=True)
    for p, t, i in zip(names, pcm, infos):
        assert np.array_equal(t.numpy()[0], flac.quantize_waves_host(want[p].cpu().numpy(), 16)), p
        assert (i.sample_rate, i.channels, i.bits_per_sample, i.total_samples) == (16000, 1, 16, L)
    del out["audio_variations_blind"]                                # without the blind set, and as wav: the same samples
    wavs = save_pc_audio_variations(out, tmp_path / "w", alphas, fmt="wav")
    assert len(wavs) == B * (1 + KD * A) and all(str(p).endswith(".wav") for p in wavs)
    sr, w = wavfile.read(str(tmp_path / "w" / "sample_1" / "pc_2" / "alpha_2.0.wav"))
    assert sr == 16000 and np.array_equal(w, flac.quantize_waves_host(out["audio_variations"][1, 1, 2].cpu().numpy(), 16))


from test_restore_gpu import restorer  # noqa: E402,F401  (the module-scoped restorer fixture of the restoration tests)


def test_restore_file_writes_flac_and_the_wav_it_always_wrote(restorer, tmp_path):  # noqa: F811
    from test_restore_gpu import ALPHAS, GAPS, recording
    pcm = np.rint(recording(seed=7).astype(np.float64) * 32768).astype(np.int16)
    for s, e in GAPS:
        pcm[s:e] = 0
    wavfile.write(str(tmp_path / "in.wav"), 16000, pcm)
    out = restorer.restore_file(tmp_path / "in.wav", tmp_path / "out.wav")                     # the default arguments
    # the wav of the default path: the bytes scipy writes for clip(rint(restored 32768)), as before this option existed
    want = np.clip(np.rint(out["restored"].detach().cpu().double().numpy() * 32768.0), -32768, 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "want.wav"), 16000, want)
    assert (tmp_path / "out.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
    restorer.restore_file(tmp_path / "in.wav", tmp_path / "out.flac", out_format="flac")
    restorer.restore_file(tmp_path / "in.wav", tmp_path / "auto.flac", out_format="auto")
    restorer.restore_file(tmp_path / "in.wav", tmp_path / "auto.wav", out_format="auto")
    assert (tmp_path / "auto.wav").read_bytes() == (tmp_path / "out.wav").read_bytes()
    assert (tmp_path / "auto.flac").read_bytes() == (tmp_path / "out.flac").read_bytes()
    (back,), (info,) = flac.decode_files([tmp_path / "out.flac"], out="pcm", backend="hip", verify_md5=True)
    assert np.array_equal(back.numpy()[0], want) and (info.sample_rate, info.channels, info.bits_per_sample) == (16000, 1, 16)
    assert len((tmp_path / "out.flac").read_bytes()) < len((tmp_path / "out.wav").read_bytes())
    with pytest.raises(ValueError):
        restorer.restore_file(tmp_path / "in.wav", tmp_path / "x.ogg", out_format="ogg")
    # save_variations: restored and every spliced variation, from restore's dict
    x = torch.from_numpy(pcm.astype(np.float32) / 32768)
    full = restorer.restore(x, GAPS, alphas=ALPHAS, variations="full")
    paths = restorer.save_variations(full, tmp_path / "var")
    names = ["restored.flac"] + [f"pc_{k + 1}/alpha_{a:.1f}.flac" for k in range(full["variations"].shape[0]) for a in ALPHAS]
    assert [str(p) for p in paths] == [str(tmp_path / "var" / n) for n in names]
    dec, _ = flac.decode_files(paths, out="pcm", backend="hip", verify_md5=True)
    waves = torch.cat([full["restored"][None], full["variations"].reshape(-1, x.numel())]).cpu().numpy()
    assert all(np.array_equal(d.numpy()[0], flac.quantize_waves_host(w, 16)) for d, w in zip(dec, waves))
