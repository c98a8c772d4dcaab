"""GPU: the FLAC encoder's predictor "lpc" on the device (csrc/flac_enc.hip: nppc_flac_enc_plan_lpc, _scan_stride,
_write_lpc) gives byte for byte what the serial host encoder and the restatement tests/flac_lpc_ref.py give, in ragged
batches of mono and stereo files, file by file and run after run; the device decoder reads the streams back, LPC subframes
chosen by the rule included; encode_waves and a saver pass the predictor on.

A call has one sample size, rate, block size and order limit, so the shapes of tests/flac_lpc_cases.py go in one batch per
(block size, rate, order limit).  Every test runs under a time limit of its own: a hang ends the process with a traceback."""
import faulthandler
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flac_lpc_cases as C
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
    for c in C.cases(bps):
        groups.setdefault((c.block_size, c.rate, c.max_order), []).append(c)
    return groups


def encode(cs, backend="hip"):
    pcm = [torch.from_numpy(c.pcm) for c in cs]
    return flac.encode_pcm([p.cuda() for p in pcm] if backend == "hip" else pcm, cs[0].bps, cs[0].rate, cs[0].block_size,
                           backend=backend, predictor="lpc", max_lpc_order=cs[0].max_order)


@pytest.fixture(scope="module")
def encoded16():
    """{(block size, rate, order limit): (cases, device streams)} at 16 bits, encoded once and shared (read-only)"""
    return {key: (cs, encode(cs)) for key, cs in batches(16).items()}


@pytest.fixture(scope="module")
def encoded24():
    return {key: (cs, encode(cs)) for key, cs in batches(24).items()}


def first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def check_batches(bps, done):
    assert {c.pcm.shape[0] for c in done[(4096, 16000, 8)][0]} == {1, 2}           # mono and stereo in one ragged batch
    assert len({c.pcm.shape[1] for c in done[(4096, 16000, 12)][0]}) >= 5
    for cs, got in done.values():
        host = encode(cs, "host")
        for c, g, h in zip(cs, got, host):
            assert g == h, f"{c.name}: device and host differ (first at byte {first_diff(g, h)})"
            assert g == C.reference(bps, c.name)[0], c.name
        assert encode(cs) == got                                                    # run after run
        for c, g in zip(cs, got):
            assert encode([c]) == [g], f"{c.name}: alone it gives other bytes than in the batch"


def test_ragged_batches_equal_host_and_restatement_16_bits(encoded16):
    check_batches(16, encoded16)


def test_ragged_batches_equal_host_and_restatement_24_bits(encoded24):
    check_batches(24, encoded24)


@pytest.mark.parametrize("bps", [16, 24])
def test_the_device_decoder_reads_every_stream_back(bps, encoded16, encoded24):
    orders = set()
    for cs, got in (encoded16 if bps == 16 else encoded24).values():
        pcm, infos = flac.decode_files(got, out="pcm", backend="hip", verify_md5=True)
        for c, g, p, i in zip(cs, got, pcm, infos):
            assert np.array_equal(p.numpy(), c.pcm), c.name
            assert (i.sample_rate, i.channels, i.bits_per_sample, i.min_blocksize) == (c.rate, c.pcm.shape[0], bps, c.block_size)
            assert len(g) <= len(C.fixed_reference(bps, c.name)), c.name
            orders |= {s["order"] for f in C.reference(bps, c.name)[1] for s in f["subframes"] if s["type"] == "lpc"}
    assert max(orders) >= 8 and min(orders) == 1                      # what the LPC decode kernels were given to read
    if bps == 24:                                                     # the side channel at 2^24, block 4608
        assert {c.name for c in encoded24[(4608, 16000, 8)][0]} == {"square", "square_stereo", "sine", "sine_stereo"}


@pytest.mark.parametrize("bits", [16, 24])
def test_encode_waves_equals_encode_pcm_of_the_numpy_quantised_samples(bits):
    full = 1 << (bits - 1)
    x = np.stack([C.voiced(6000, bits, seed, 100 + 9 * seed).astype(np.float32) / np.float32(full) for seed in range(5)])
    x[1, :4] = [1.0, -1.0, np.nan, 3.0]
    lens = [6000, 4097, 1, 17, 4096]
    q = flac.quantize_waves_host(x, bits)
    kw = dict(predictor="lpc", max_lpc_order=10)
    got = flac.encode_waves(torch.from_numpy(x).cuda(), lens, 22050, bits, backend="hip", **kw)
    want = flac.encode_pcm([torch.from_numpy(q[v:v + 1, :n].copy()) for v, n in enumerate(lens)], bits, 22050, backend="host", **kw)
    assert got == want
    assert flac.encode_waves(torch.from_numpy(x), lens, 22050, bits, backend="host", **kw) == want
    fixed = flac.encode_waves(torch.from_numpy(x).cuda(), lens, 22050, bits, backend="hip")
    assert fixed == flac.encode_waves(torch.from_numpy(x).cuda(), lens, 22050, bits, backend="hip", predictor="fixed")
    assert all(len(g) <= len(f) for g, f in zip(got, fixed)) and len(got[0]) < len(fixed[0])
    back, _ = flac.decode_files(got, out="pcm", backend="hip", verify_md5=True)
    assert all(np.array_equal(b.numpy()[0], q[v, :n]) for v, (b, n) in enumerate(zip(back, lens)))


def test_save_variations_writes_lpc_files_of_the_same_samples(tmp_path):
    from nppc_audio.inpainting.restore import RecordingRestorer
    K, A, L = 2, 3, 5000
    waves = torch.from_numpy(np.stack([C.voiced(L, 16, s, 90 + 7 * s) for s in range(1 + K * A)]).astype(np.float32) / 32768)
    out = {"restored": waves[0].cuda(), "variations": waves[1:].reshape(K, A, L).cuda(), "alphas": [-1.0, 0.0, 1.0]}
    me = SimpleNamespace(device="cuda", config=SimpleNamespace(sample_rate=16000))  # all that save_variations reads of self
    fixed = RecordingRestorer.save_variations(me, out, tmp_path / "fixed")
    again = RecordingRestorer.save_variations(me, out, tmp_path / "again", flac_predictor="fixed")
    lpc = RecordingRestorer.save_variations(me, out, tmp_path / "lpc", flac_predictor="lpc")
    assert len(fixed) == len(lpc) == 1 + K * A
    assert [open(p, "rb").read() for p in fixed] == [open(p, "rb").read() for p in again]
    a, _ = flac.decode_files(fixed, out="pcm", backend="hip", verify_md5=True)
    b, _ = flac.decode_files(lpc, out="pcm", backend="hip", verify_md5=True)
    want = flac.quantize_waves_host(waves.numpy(), 16)
    assert all(np.array_equal(x.numpy(), y.numpy()) and np.array_equal(y.numpy()[0], w) for x, y, w in zip(a, b, want))
    assert all(len(open(p, "rb").read()) < len(open(f, "rb").read()) for p, f in zip(lpc, fixed))
    with pytest.raises(ValueError):
        RecordingRestorer.save_variations(me, out, tmp_path / "bad", flac_predictor="tukey")
