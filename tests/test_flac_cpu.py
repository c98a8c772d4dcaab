"""CPU: the FLAC decoder core through its host entry points (nppc_flac_probe, nppc_flac_decode_host) against the restatement
tests/flac_ref.py on every case of tests/flac_cases.py, the metadata walk, the statuses, a flac folder as an
AudioInpaintingDataset against the same PCM as wav, and the mutation sweep: a damaged file is an error or exactly the
original samples, never silently something else.  No tolerances: everything here is equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def host_pcm(data):
    from nppc_audio import flac
    (pcm,), (info,) = flac.decode_files([data], out="pcm", backend="host")
    return pcm.numpy(), info


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_and_argument_errors():
    from nppc_audio import _hip
    lib = _hip.lib()
    for name in ("nppc_flac_probe", "nppc_flac_decode_host", "nppc_flac_work_elems", "nppc_flac_scan", "nppc_flac_parse",
                 "nppc_flac_chain", "nppc_flac_decode"):
        assert hasattr(lib, name) and name in _hip.SIGS
    n = ctypes.c_long()
    _hip.call("nppc_flac_work_elems", 1000, ctypes.byref(n))
    assert n.value >= 8 + 2 * 1000 + 2048 + (3 * 1000 + 2048) // 2      # the arrays of include/nppc_hip.h fit
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_flac_work_elems", 0, ctypes.byref(n))
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_flac_probe", None, 10, None, None)
    with pytest.raises(RuntimeError, match="bad argument"):               # null pointers are rejected before any launch
        _hip.call("nppc_flac_scan", None, 10, None, 1, None, 8, None)
    info, st = (ctypes.c_long * 8)(), ctypes.c_int()
    buf = np.zeros(8, np.uint8)
    with pytest.raises(RuntimeError, match="unsupported"):                # 2^31 bytes: refused from the length alone
        _hip.call("nppc_flac_probe", buf.ctypes.data, 2 ** 31, ctypes.addressof(info), ctypes.addressof(st))
    # an output that is too small is an argument error, not a write
    c = C.cases()["fixed2"]
    data = np.frombuffer(c.data, np.uint8)
    small = np.zeros(10, np.int32)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_flac_decode_host", data.ctypes.data, data.size, small.ctypes.data, small.size, 0, 0, ctypes.addressof(st))


# ---- the case table ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_decoded():
    return {k: R.decode(c.data) for k, c in C.cases().items()}


def test_reference_decoder_returns_the_source(ref_decoded):
    for k, c in C.cases().items():
        info, pcm = ref_decoded[k]
        assert np.array_equal(np.array(pcm, np.int64), c.pcm), k
        assert (info["bits_per_sample"], info["sample_rate"], info["channels"]) == (c.bps, c.rate, c.pcm.shape[0]), k


def test_host_decoder_equals_source_and_reference(ref_decoded):
    from nppc_audio import flac
    names = list(C.cases())
    pcms, infos = flac.decode_files([C.cases()[k].data for k in names], out="pcm", backend="host")
    monos, _ = flac.decode_files([C.cases()[k].data for k in names], out="mono", backend="host")
    for k, pcm, mono, info in zip(names, pcms, monos, infos):
        c = C.cases()[k]
        rinfo, rpcm = ref_decoded[k]
        assert pcm.dtype == torch.int32 and np.array_equal(pcm.numpy(), c.pcm), k
        assert np.array_equal(pcm.numpy(), np.array(rpcm, np.int64)), k
        assert info == flac.FlacInfo(rinfo["sample_rate"], rinfo["channels"], rinfo["bits_per_sample"], rinfo["total_samples"],
                                     rinfo["min_blocksize"], rinfo["max_blocksize"], rinfo["first_frame"]), k
        x = c.pcm.T.astype(np.float32) / np.float32(1 << (c.bps - 1))           # what _decode_wav does with the same PCM
        want = x.mean(axis=1) if x.shape[1] > 1 else x[:, 0]
        assert mono.dtype == torch.float32 and np.array_equal(mono.numpy(), want), k


def test_mono_equals_decode_wav_of_the_same_pcm(tmp_path):
    from nppc_audio.data import _decode_flac, _decode_wav
    for k in ("bps8_header", "bps12_header", "bps16_header", "bps20_streaminfo", "bps24_header", "ch2_mid_side", "ch3",
              "ch2_24bit_mid_side", "speech"):
        c = C.cases()[k]
        (tmp_path / f"{k}.flac").write_bytes(c.data)
        C.write_wav(tmp_path / f"{k}.wav", c)
        for rate in (c.rate, 8000):                                              # 8000: through the shared resampling branch
            a, b = _decode_flac(tmp_path / f"{k}.flac", rate), _decode_wav(tmp_path / f"{k}.wav", rate)
            assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b), (k, rate)


# ---- metadata, statuses ------------------------------------------------------------------------------------------------
def test_probe_walks_every_metadata_block():
    from nppc_audio import flac
    c = C.cases()["metadata"]
    info = flac.probe(c.data)
    want = 4 + sum(4 + len(b) for _, b in [(0, bytes(34))] + C.METADATA)
    assert info.first_frame_offset == want and info.total_samples == 200 and info.sample_rate == C.RATE
    assert (info.channels, info.bits_per_sample, info.min_blocksize, info.max_blocksize) == (1, 16, 192, 192)
    assert np.array_equal(host_pcm(c.data)[0], c.pcm)              # the SEEKTABLE-typed block holds frame headers: ignored
    plain = C.cases()["fixed2"]
    assert flac.probe(plain.data).first_frame_offset == 42


def status_of(data):
    from nppc_audio import flac
    with pytest.raises(flac.FlacError) as e:
        host_pcm(data)
    assert isinstance(e.value, ValueError) and "<bytes>" in str(e.value)
    return e.value.status


def test_statuses():
    good = C.cases()["fixed2"].data
    si = R.streaminfo
    head = lambda body, typ=0: b"fLaC" + R.metadata_block(typ, body, last=True)
    assert status_of(b"RIFF" + good[4:]) == R.BAD_MARKER
    assert status_of(b"") == R.TRUNCATED and status_of(b"fLaC") == R.TRUNCATED and status_of(good[:30]) == R.TRUNCATED
    assert status_of(b"fLaC" + R.metadata_block(1, bytes(34), last=True)) == R.BAD_STREAMINFO
    assert status_of(head(bytes(34), 127)) == R.BAD_STREAMINFO
    assert status_of(head(si(16, 16, 16000, 1, 32, 100))) == R.UNSUPPORTED
    assert status_of(head(si(16, 16, 16000, 1, 16, 0))) == R.UNSUPPORTED
    assert status_of(b"ID3\x04" + good) == R.UNSUPPORTED and status_of(b"OggS" + good) == R.UNSUPPORTED
    assert status_of(good[:42] + b"\x00" + good[43:]) == R.BAD_HEADER
    for data, st in C.corrupt_files():
        assert status_of(data) == st
        with pytest.raises(R.FlacRefError) as e:
            R.decode(data)
        assert e.value.status == st
    # a 36-bit sample number: truncated to 32 bits it would be the running count, and the frame would be accepted
    x = C.walk(32, 16, 5)
    sub = dict(subframes=R.fixed(1))
    ok = C.make(x, 16, blocksizes=[16, 16], frames=sub, variable=True)
    assert np.array_equal(host_pcm(ok.data)[0], ok.pcm)
    beyond = C.make(x, 16, blocksizes=[16, 16], frames=sub, variable=True, numbers=[0, (1 << 32) + 16])
    assert status_of(beyond.data) == R.COUNT_MISMATCH
    with pytest.raises(R.FlacRefError) as e:
        R.decode(beyond.data)
    assert e.value.status == R.COUNT_MISMATCH
    info = R.probe(beyond.data)
    _, second = R.decode_frame(beyond.data, 42, info, R.parse_header(beyond.data, 42, info))
    assert R.parse_header(beyond.data, second, info)["pos"] == (1 << 32) + 16


# ---- the dataset -------------------------------------------------------------------------------------------------------
def data_config(**kw):
    from nppc_audio.inpainting.trainer.nppc_trainer import AudioInpaintingConfig
    d = dict(clean_path=".", stft_configuration=dict(nfft=63, hop_length=32, win_length=63), sub_sample_length_seconds=0.5,
             missing_length_seconds=0.064, use_vad=True)
    d.update(kw)
    return AudioInpaintingConfig(**d)


def write_folders(tmp_path):
    """six recordings as flac (one of them stereo, one at 8 kHz) and the same PCM as wav"""
    lens = [3000, 9000, 2000, 1000, 8200, 500]
    sub = dict(subframes=R.lpc([1638, -819], 12, 10))
    (tmp_path / "flac" / "deep").mkdir(parents=True)
    (tmp_path / "wav" / "deep").mkdir(parents=True)
    for i, n in enumerate(lens):
        ch = 2 if i == 1 else 1
        rate = 8000 if i == 4 else C.RATE
        n = n // 2 if i == 4 else n
        pcm = [C.walk(n, 16, 200 + i + c) // 2 for c in range(ch)]
        sizes = [1152] * (n // 1152) + ([n % 1152] if n % 1152 else [])
        c = C.make(pcm, 16, rate, blocksizes=sizes, frames=sub)
        where = "deep/" if i == 5 else ""                     # sorts last: rglob finds it
        (tmp_path / "flac" / f"{where}clip{i}.flac").write_bytes(c.data)
        C.write_wav(tmp_path / "wav" / f"{where}clip{i}.wav", c)
    return lens


def test_flac_folder_gives_the_dataset_of_the_same_pcm_as_wav(tmp_path):
    """the test that fails without the decoder: a folder of .flac files trains"""
    from nppc_audio.inpainting.data import AudioInpaintingDataset
    lens = write_folders(tmp_path)
    a = AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "flac")))
    b = AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "wav")))
    assert len(a) == len(b) == 6 and [c.numel() for c in a.clean] == lens
    assert [f.stem for f in a.clean_files] == [f.stem for f in b.clean_files]
    for x, y in zip(a.clean, b.clean):
        assert x.dtype == y.dtype == torch.float32 and torch.equal(x, y)
    assert a.file_of == b.file_of == [1, 1, 4, 4, 4, 1]
    assert torch.equal(a.gain, b.gain)
    # wav files win: flacs next to them stay ignored, as before
    (tmp_path / "wav" / "extra.flac").write_bytes(C.cases()["speech"].data)
    assert len(AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "wav")))) == 6
    # a file the probe rejects is skipped with a warning; the others still load
    (tmp_path / "flac" / "broken.flac").write_bytes(b"fLaC")
    with pytest.warns(UserWarning, match="broken.flac"):
        assert len(AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "flac")))) == 6
    # a file damaged past its metadata is an error that names it
    (tmp_path / "flac" / "clip0.flac").write_bytes(C.corrupt_files()[0][0])
    with pytest.warns(UserWarning), pytest.raises(ValueError, match="clip0.flac.*CRC-16"):
        AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "flac")))


def test_decode_files_arguments():
    from nppc_audio import flac
    with pytest.raises(ValueError, match="out must be"):
        flac.decode_files([], out="stereo")
    with pytest.raises(ValueError, match="backend must be"):
        flac.decode_files([], backend="cpu")
    assert flac.decode_files([], backend="host") == ([], [])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            flac.decode_files([C.cases()["fixed2"].data], backend="device")


# ---- mutations ---------------------------------------------------------------------------------------------------------
def test_golden_stream_is_the_generated_one():
    """tools/check/flac_host_check.cc sweeps tests/golden/flac_two_frame.flac under the sanitizers: the same bytes as here"""
    with open(os.path.join(HERE, "golden", "flac_two_frame.flac"), "rb") as f:
        assert f.read() == C.two_frame_stereo().data


def test_every_truncation_and_bit_flip_is_an_error_or_exact():
    from nppc_audio import _hip
    c = C.two_frame_stereo()
    n_ch, n = c.pcm.shape
    assert len(c.data) >= 600 and R.decode(c.data)[1] == c.pcm.tolist()
    pcm = np.empty((n_ch, n), np.int32)
    st, info = ctypes.c_int(), (ctypes.c_long * 8)()

    def run(buf):
        """-> status, or None when the decode succeeded with the original samples"""
        _hip.call("nppc_flac_probe", buf.ctypes.data or base.ctypes.data, buf.size, ctypes.addressof(info), ctypes.addressof(st))
        if st.value:
            return st.value
        if info[1] * info[3] > pcm.size:                           # a flip made the stream claim more samples than before
            big = np.empty(info[1] * info[3], np.int32) if info[1] * info[3] < 1 << 24 else None
            if big is None:
                return "huge"
            _hip.call("nppc_flac_decode_host", buf.ctypes.data, buf.size, big.ctypes.data, big.size, 0, 0, ctypes.addressof(st))
            assert st.value, "more samples than the stream holds came back"
            return st.value
        pcm.fill(0x5A5A5A5A)
        _hip.call("nppc_flac_decode_host", buf.ctypes.data, buf.size, pcm.ctypes.data, pcm.size, 0, 0, ctypes.addressof(st))
        if st.value:
            return st.value
        assert (info[1], info[3]) == (n_ch, n) and np.array_equal(pcm, c.pcm), "a wrong sample came back silently"
        return None

    base = np.frombuffer(c.data, np.uint8)
    assert run(base.copy()) is None
    for cut in range(len(c.data)):
        assert run(base[:cut].copy()) is not None, cut
    survived = []
    for bit in range(600 * 8):
        buf = base.copy()
        buf[bit >> 3] ^= 0x80 >> (bit & 7)
        if run(buf) is None:
            survived.append(bit >> 3)
    # what a flip may leave intact: STREAMINFO's maximum blocksize when it grows, its frame-size hints and its MD5 (nothing
    # reads them); the frames state their own rate, sample size and channels, so those fields are checked against them
    assert survived and all(10 <= b < 18 or 26 <= b < 42 for b in survived), sorted(set(survived))
    assert R.probe(c.data)["first_frame"] == 42
