"""CPU: the MD5 of decoded FLAC samples on the host (csrc/md5_core.h through nppc_flac_md5_host and nppc_flac_stream_md5;
nppc_audio.flac.pcm_md5, stream_md5, decode_files(verify_md5=True)) and a flac folder through AudioInpaintingDataset.
The oracle is hashlib.md5 over a message built here with numpy; everything is equality."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = [(1, 8), (1, 16), (2, 16), (2, 24), (3, 12), (8, 20), (1, 24)]
# message lengths in bytes around the padding boundaries (a second pad block appears at 56 and at 120)
BOUNDARIES = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128]


def message(pcm, bps):
    """FLAC's MD5 message of int32 pcm [C, n]: interleaved by channel, (bps + 7) // 8 little-endian bytes a sample"""
    nbytes = (bps + 7) // 8
    inter = np.ascontiguousarray(pcm.T.astype("<i4")).reshape(-1)
    return np.ascontiguousarray(inter.view(np.uint8).reshape(-1, 4)[:, :nbytes]).tobytes()


def oracle(pcm, bps):
    return hashlib.md5(message(pcm, bps)).digest()


def sample_counts(channels, bps):
    """per boundary length the sample count whose message is that long, or the nearest one above it that exists, and longer
    ones: 20 blocks, and odd counts that leave the 16-bit paths a ragged tail"""
    step = channels * ((bps + 7) // 8)
    counts = sorted({-(-b // step) for b in BOUNDARIES} | {1, 2, 3, 5, 31, 33, 67, -(-1280 // step), -(-1280 // step) + 1})
    return counts


def random_pcm(channels, bps, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    x = g.integers(lo, hi + 1, (channels, n)).astype(np.int32)
    flat = x.reshape(-1)
    for k, v in enumerate((lo, hi, -1, lo, hi)):                   # both extremes and -1: sign extension into 2 and 3 bytes
        if flat.size >= 5:
            flat[k * (flat.size // 5)] = v
    return x


def md5_cases():
    """[(pcm [C, n] int32, bps)]: every format at every boundary length"""
    out = []
    for channels, bps in FORMATS:
        for n in sample_counts(channels, bps):
            out.append((random_pcm(channels, bps, n, 1000 * channels + 10 * bps + n), bps))
    return out


def test_message_lengths_cover_the_padding_boundaries():
    lengths = {len(message(p, b)) for p, b in md5_cases()}
    assert set(BOUNDARIES) <= lengths                              # (1, 8) reaches every one of them exactly
    for channels, bps in FORMATS:
        mine = {len(message(p, b)) % 64 for p, b in md5_cases() if (p.shape[0], b) == (channels, bps)}
        assert any(r >= 56 for r in mine) and any(0 < r < 56 for r in mine) and 0 in mine, (channels, bps)
    for p, b in md5_cases():
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        assert p.size < 5 or (p.min() == lo and p.max() == hi and (p == -1).any())


def test_pcm_md5_on_host_tensors_equals_hashlib():
    from nppc_audio import flac
    cases = md5_cases()
    got = flac.pcm_md5([torch.from_numpy(p) for p, _ in cases], [b for _, b in cases])
    assert len(got) == len(cases)
    for (p, b), d in zip(cases, got):
        assert isinstance(d, bytes) and d == oracle(p, b), (p.shape, b)
    p, b = cases[40]
    assert flac.pcm_md5(torch.from_numpy(p), b) == [oracle(p, b)]              # one tensor, one int
    assert flac.pcm_md5(torch.zeros(2, 0, dtype=torch.int32), 16, backend="host") == [hashlib.md5(b"").digest()]
    assert flac.pcm_md5([], 16) == []
    with pytest.raises(ValueError, match="int32"):
        flac.pcm_md5(torch.zeros(1, 4), 16)
    with pytest.raises(ValueError, match="bits_per_sample"):
        flac.pcm_md5(torch.zeros(1, 4, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="backend"):
        flac.pcm_md5(torch.zeros(1, 4, dtype=torch.int32), 16, backend="cpu")


def test_host_entry_points_and_argument_errors():
    from nppc_audio import _hip
    d = (ctypes.c_ubyte * 16)()
    x = np.arange(8, dtype=np.int32)
    _hip.call("nppc_flac_md5_host", x.ctypes.data, 8, 1, 16, ctypes.addressof(d))
    assert bytes(d) == hashlib.md5(x.astype("<i2").tobytes()).digest()
    _hip.call("nppc_flac_md5_host", x.ctypes.data, 8, 1, 32, ctypes.addressof(d))       # four bytes a sample
    assert bytes(d) == hashlib.md5(x.astype("<i4").tobytes()).digest()
    _hip.call("nppc_flac_md5_host", 0, 0, 1, 16, ctypes.addressof(d))
    assert bytes(d).hex() == "d41d8cd98f00b204e9800998ecf8427e"
    for n, ch, bps in ((8, 0, 16), (8, 9, 16), (8, 1, 3), (8, 1, 33), (-1, 1, 16)):
        with pytest.raises(RuntimeError, match="bad argument"):
            _hip.call("nppc_flac_md5_host", x.ctypes.data, n, ch, bps, ctypes.addressof(d))
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_flac_md5_host", x.ctypes.data, 8, 1, 16, 0)
    with pytest.raises(RuntimeError, match="bad argument"):               # null pointers are rejected before any launch
        _hip.call("nppc_flac_md5", None, 0, None, 1, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_flac_stream_md5", None, 10, None, None, None)
    from nppc_audio import flac
    assert flac.STATUS[9] and "MD5" in flac.STATUS[9]
    assert flac.FlacInfo._fields == ("sample_rate", "channels", "bits_per_sample", "total_samples", "min_blocksize",
                                     "max_blocksize", "first_frame_offset")


# ---- streams that state an MD5 -----------------------------------------------------------------------------------------
def with_md5(case, digest):
    assert case.data[26:42] == bytes(16)                           # flac_ref's encoder writes "not computed"
    return case.data[:26] + digest + case.data[42:]


STREAMS = ("speech", "ch2_mid_side", "ch3", "bps8_header", "bps12_streaminfo", "bps20_header", "ch2_24bit_mid_side", "bs16",
           "wasted5", "metadata")


def stated_streams():
    """{name: (bytes with the hashlib digest of the case's PCM in STREAMINFO, case)}"""
    return {k: (with_md5(C.cases()[k], oracle(C.cases()[k].pcm, C.cases()[k].bps)), C.cases()[k]) for k in STREAMS}


def flipped(data, bit=77):
    out = bytearray(data)
    out[26 + (bit >> 3)] ^= 0x80 >> (bit & 7)
    return bytes(out)


def other_pcm_digest(case):
    """the digest of other samples of the same shape"""
    other = case.pcm.copy()
    other[-1, -1] ^= 1
    return oracle(other, case.bps)


def test_stream_md5_reads_the_field():
    from nppc_audio import flac
    for k, (data, c) in stated_streams().items():
        assert flac.stream_md5(data) == oracle(c.pcm, c.bps), k
        assert flac.stream_md5(c.data) is None, k
    assert flac.stream_md5(os.path.join(HERE, "golden", "flac_two_frame.flac")) is None
    with pytest.raises(flac.FlacError) as e:
        flac.stream_md5(b"fLaC")
    assert e.value.status == R.TRUNCATED
    with pytest.raises(flac.FlacError):
        flac.stream_md5(b"")


def check_verified_decode(backend):
    """what both backends owe (tests/test_flac_md5_gpu.py runs this with backend="device")"""
    from nppc_audio import flac
    streams = stated_streams()
    datas = [d for d, _ in streams.values()]
    for out in ("pcm", "mono"):
        plain, infos = flac.decode_files(datas, out=out, backend=backend)
        checked, infos2 = flac.decode_files(datas, out=out, backend=backend, verify_md5=True)
        assert infos == infos2 and len(checked) == len(datas)
        assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(plain, checked)), out
    for (k, (data, c)), t in zip(streams.items(), flac.decode_files(datas, out="pcm", backend=backend, verify_md5=True)[0]):
        assert np.array_equal(t.numpy(), c.pcm), k
    first = datas[0]
    for k, (data, c) in streams.items():
        for bad in (flipped(data), flipped(data, 0), flipped(data, 127), with_md5(c, other_pcm_digest(c))):
            with pytest.raises(flac.FlacError) as e:
                flac.decode_files([first, bad], out="mono", backend=backend, verify_md5=True)
            assert e.value.status == 9 and e.value.path == "<bytes>" and isinstance(e.value, ValueError), k
            assert bad[26:42].hex() in str(e.value) and oracle(c.pcm, c.bps).hex() in str(e.value), k
            got, _ = flac.decode_files([first, bad], out="pcm", backend=backend)       # the default: as before
            assert np.array_equal(got[1].numpy(), c.pcm), k
            got, _ = flac.decode_files([first, bad], out="pcm", backend=backend, verify_md5=False)
            assert np.array_equal(got[1].numpy(), c.pcm), k
        # an all-zero digest passes, next to files that state one and alone
        got, _ = flac.decode_files([first, c.data], out="pcm", backend=backend, verify_md5=True)
        assert np.array_equal(got[1].numpy(), c.pcm), k
        got, _ = flac.decode_files([c.data], out="pcm", backend=backend, verify_md5=True)
        assert np.array_equal(got[0].numpy(), c.pcm), k
    # a damaged frame stays what it was: the CRC-16 status, not an MD5 one
    crc = C.corrupt_files()[0][0]
    with pytest.raises(flac.FlacError) as e:
        flac.decode_files([first, crc[:26] + bytes(range(1, 17)) + crc[42:]], backend=backend, verify_md5=True)
    assert e.value.status == R.CRC16


def test_decode_files_verifies_on_the_host(tmp_path):
    from nppc_audio import flac
    check_verified_decode("host")
    data, c = stated_streams()["speech"]
    (tmp_path / "named_clip.flac").write_bytes(flipped(data))
    with pytest.raises(flac.FlacError, match="named_clip.flac.*MD5") as e:
        flac.decode_files([tmp_path / "named_clip.flac"], backend="host", verify_md5=True)
    assert e.value.status == 9 and e.value.path.endswith("named_clip.flac")


# ---- the dataset -------------------------------------------------------------------------------------------------------
def write_folder(tmp_path, wrong=None):
    """four recordings whose STREAMINFO states the MD5 of their PCM (one stereo); `wrong`: the file whose digest has a bit
    flipped"""
    from test_flac_cpu import data_config
    sub = dict(subframes=R.lpc([1638, -819], 12, 10))
    folder = tmp_path / "flac"
    folder.mkdir(exist_ok=True)
    for i, n in enumerate([9000, 8200, 3000, 8500]):
        ch = 2 if i == 1 else 1
        pcm = [C.walk(n, 16, 400 + i + k) // 2 for k in range(ch)]
        sizes = [1152] * (n // 1152) + ([n % 1152] if n % 1152 else [])
        c = C.make(pcm, 16, blocksizes=sizes, frames=sub)
        data = with_md5(c, oracle(c.pcm, 16))
        (folder / f"clip{i}.flac").write_bytes(flipped(data) if i == wrong else data)
    return data_config(clean_path=str(folder))


def test_flac_folder_is_verified_by_default(tmp_path):
    from nppc_audio import flac
    from nppc_audio.inpainting.data import AudioInpaintingDataset
    cfg = write_folder(tmp_path)
    a = AudioInpaintingDataset(cfg)
    b = AudioInpaintingDataset(cfg, verify_flac_md5=False)
    assert len(a) == len(b) == 4 and a.file_of == b.file_of and torch.equal(a.gain, b.gain)
    assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a.clean, b.clean))
    cfg = write_folder(tmp_path, wrong=2)
    with pytest.raises(flac.FlacError, match="clip2.flac") as e:
        AudioInpaintingDataset(cfg)
    assert e.value.status == 9
    c = AudioInpaintingDataset(cfg, verify_flac_md5=False)          # the way out
    assert all(torch.equal(x, y) for x, y in zip(c.clean, a.clean))
