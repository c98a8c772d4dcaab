"""GPU: the batched FLAC decoder (nppc_flac_scan / _parse / _chain / _decode through nppc_audio.flac.decode_files) against
the source PCM and the serial host decoder on every case of tests/flac_cases.py, in one ragged batch and each alone, the
scan-specific cases, a batch with corrupt files, and a flac folder against the same PCM as wav through the dataset, the
device loader and RecordingRestorer.restore_file.  Everything is equality; there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as R

pytestmark = pytest.mark.gpu


def device(datas, out="pcm", **kw):
    from nppc_audio import flac
    return flac.decode_files(datas, out=out, backend="device", **kw)[0]


def host(datas, out="pcm"):
    from nppc_audio import flac
    return flac.decode_files(datas, out=out, backend="host")[0]


def wav_mono(case):
    """what data._decode_wav yields for the PCM of a case written as wav"""
    x = case.pcm.T.astype(np.float32) / np.float32(1 << (case.bps - 1))
    return x.mean(axis=1) if x.shape[1] > 1 else x[:, 0]


@pytest.fixture(scope="module")
def table():
    names = list(C.cases())
    datas = [C.cases()[k].data for k in names]
    return names, datas, device(datas, "pcm"), device(datas, "mono")


def test_ragged_batch_equals_source_host_decoder_and_wav(table):
    names, datas, pcm, mono = table
    for k, a, b, m in zip(names, pcm, host(datas), mono):
        c = C.cases()[k]
        assert a.dtype == torch.int32 and not a.is_cuda and np.array_equal(a.numpy(), c.pcm), k
        assert torch.equal(a, b), k
        assert m.dtype == torch.float32 and np.array_equal(m.numpy(), wav_mono(c)), k


def test_item_alone_equals_item_in_batch_and_runs_repeat(table):
    names, datas, pcm, mono = table
    for k, d, a, m in zip(names, datas, pcm, mono):
        assert torch.equal(device([d])[0], a), k
        assert torch.equal(device([d], "mono")[0], m), k
    again = device(datas, "pcm")                                    # two runs: identical bits
    assert all(torch.equal(x, y) for x, y in zip(again, pcm))
    again = device(datas, "mono")
    assert all(torch.equal(x, y) for x, y in zip(again, mono))
    # several batches under a byte budget, one file larger than the budget, and another order: nothing changes
    small = device(datas, "pcm", max_batch_bytes=50000)
    assert all(torch.equal(x, y) for x, y in zip(small, pcm))
    back = device(datas[::-1], "mono")[::-1]
    assert all(torch.equal(x, y) for x, y in zip(back, mono))


def test_wav_written_by_scipy_decodes_to_the_same_mono(tmp_path):
    from nppc_audio.data import _decode_flac, _decode_wav
    for k in ("bps8_header", "bps12_streaminfo", "bps20_header", "bps24_header", "ch2_mid_side", "ch3", "speech"):
        c = C.cases()[k]
        (tmp_path / "a.flac").write_bytes(c.data)
        C.write_wav(tmp_path / "a.wav", c)
        for rate in (c.rate, 8000):
            assert torch.equal(_decode_flac(tmp_path / "a.flac", rate), _decode_wav(tmp_path / "a.wav", rate)), (k, rate)


def test_scan_cases():
    # a header on the last byte of the first scan workgroup's range (256 lanes x 16 bytes) and of a lane's 16 bytes
    for off in (4095, 4096, 4097, 8191, 47 + 16 * 3):
        c = C.header_at(off)
        assert np.array_equal(device([c.data])[0].numpy(), c.pcm), off
    # frames that begin at every byte position relative to the lanes' ranges: the same file behind 0..16 other bytes
    c = C.cases()["frames200"]
    filler = C.cases()["constant"].data
    for shift in range(1, 18):
        pad = C.make(C.walk(16, 16, 3), 16, metadata=[(1, bytes(shift))])
        got = device([pad.data, c.data, filler])
        assert np.array_equal(got[1].numpy(), c.pcm) and np.array_equal(got[0].numpy(), pad.pcm), shift
    # a file that ends inside what looks like a header which the neighbour's first byte would complete
    a, b = C.tail_that_neighbour_completes(), C.cases()["fixed2"]
    assert R.crc8(a.data[-5:]) == b.data[0]
    got = device([a.data, b.data, a.data])
    assert np.array_equal(got[0].numpy(), a.pcm) and np.array_equal(got[1].numpy(), b.pcm) and torch.equal(got[0], got[2])
    # valid headers inside a payload, a one-sample last frame, one frame, two-byte frame numbers: in the table as well
    for k in ("header_in_payload", "last_frame_1", "frames200", "bs_is_order", "metadata"):
        assert np.array_equal(device([C.cases()[k].data])[0].numpy(), C.cases()[k].pcm), k


def test_corrupt_files_keep_to_themselves():
    from nppc_audio import _hip as H
    from nppc_audio import flac
    bad = C.corrupt_files()
    good = [C.cases()[k] for k in ("speech", "ch3", "bs16", "fullscale24_lpc32", "residual_method1")]
    order = [good[0], bad[0], good[1], bad[1], good[2], good[3], bad[2], good[4]]
    datas = [x.data if isinstance(x, C.Case) else x[0] for x in order]
    with pytest.raises(flac.FlacError) as e:
        device(datas)
    assert e.value.status == bad[0][1] and "<bytes>" in str(e.value)        # the first bad file is the one named
    # the statuses of all eight and the outputs of the five, through the entry points themselves
    bufs = [np.frombuffer(d, np.uint8) for d in datas]
    infos = []
    for b in bufs:
        infos.append(flac._probe(b, "x"))
    dev = torch.device("cuda")
    nf = len(bufs)
    begin = np.concatenate([[0], np.cumsum([b.size for b in bufs])])
    n_pcm = [i.channels * i.total_samples for i in infos]
    off = np.concatenate([[0], np.cumsum(n_pcm)])
    meta = np.zeros((nf, 12), np.int64)
    meta[:, 0], meta[:, 1], meta[:, 9], meta[:, 10] = begin[:-1], begin[1:], off[:-1], 0
    for f, i in enumerate(infos):
        meta[f, 2:9] = (i.sample_rate, i.channels, i.bits_per_sample, i.min_blocksize, i.max_blocksize, i.total_samples,
                        i.first_frame_offset)
    d_bytes = torch.from_numpy(np.concatenate(bufs)).to(dev)
    d_meta = torch.from_numpy(meta).to(dev)
    cap = int(begin[-1]) // 4 + 1
    import ctypes
    elems = ctypes.c_long()
    H.call("nppc_flac_work_elems", cap, ctypes.byref(elems))
    work = torch.empty(elems.value, dtype=torch.int64, device=dev)
    pcm = torch.full((int(off[-1]),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    status = torch.empty(nf + 1, dtype=torch.int32, device=dev)
    s = H.stream()
    H.call("nppc_flac_scan", d_bytes, int(begin[-1]), d_meta, nf, work, cap, s)
    H.call("nppc_flac_parse", d_bytes, d_meta, nf, work, cap, s)
    H.call("nppc_flac_chain", d_bytes, d_meta, nf, work, cap, status, s)
    H.call("nppc_flac_decode", d_bytes, d_meta, nf, work, cap, pcm, pcm.numel(), None, 0, s)
    want = [0 if isinstance(x, C.Case) else x[1] for x in order]
    assert status.cpu().tolist() == want + [0]
    assert want.count(0) == 5 and sorted(w for w in want if w) == sorted([R.CRC16, R.TRUNCATED, R.RESERVED])
    host_pcm = pcm.cpu().numpy()
    for f, x in enumerate(order):
        if isinstance(x, C.Case):
            assert np.array_equal(host_pcm[off[f]:off[f + 1]].reshape(x.pcm.shape), x.pcm), f
            assert torch.equal(device([x.data])[0], torch.from_numpy(x.pcm)), f    # as if decoded alone
    # a candidate buffer that is too small is reported, and decode_files runs the batch again with one that always suffices
    c = C.cases()["frames200"]
    H.call("nppc_flac_scan", d_bytes, int(begin[-1]), d_meta, nf, work, 4, s)
    H.call("nppc_flac_parse", d_bytes, d_meta, nf, work, 4, s)
    H.call("nppc_flac_chain", d_bytes, d_meta, nf, work, 4, status, s)
    assert status.cpu().tolist()[nf] == 1
    many = C.many_headers_in_payload()
    info = flac.probe(many.data)
    assert 1536 > 2 * -(-info.total_samples // info.min_blocksize) + len(many.data) // 4096 + 1024
    got = device([c.data, many.data, c.data])
    assert np.array_equal(got[1].numpy(), many.pcm) and np.array_equal(got[0].numpy(), c.pcm) and torch.equal(got[0], got[2])


# ---- the callers -------------------------------------------------------------------------------------------------------
def write_folders(tmp_path, n_files=4, length=12000):
    sub = dict(subframes=R.lpc([1638, -819], 12, 10))
    (tmp_path / "flac").mkdir()
    (tmp_path / "wav").mkdir()
    for i in range(n_files):
        ch = 2 if i == 1 else 1
        n = length + 500 * i if i != 2 else 3000
        pcm = [C.walk(n, 16, 300 + i + c) // 2 for c in range(ch)]
        sizes = [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
        c = C.make(pcm, 16, blocksizes=sizes, frames=sub)
        (tmp_path / "flac" / f"clip{i}.flac").write_bytes(c.data)
        C.write_wav(tmp_path / "wav" / f"clip{i}.wav", c)


def test_flac_folder_trains_like_the_wav_folder(tmp_path):
    from nppc_audio.inpainting.data import AudioInpaintingDataset, InpaintingDeviceLoader
    from test_flac_cpu import data_config
    write_folders(tmp_path)
    a = AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "flac"), seed=11))
    b = AudioInpaintingDataset(data_config(clean_path=str(tmp_path / "wav"), seed=11))
    assert len(a) == 4 and a.file_of == b.file_of and torch.equal(a.gain, b.gain)
    assert all(torch.equal(x, y) for x, y in zip(a.clean, b.clean))
    x = InpaintingDeviceLoader(a, None).batch([0, 1, 2, 3])
    y = InpaintingDeviceLoader(b, None).batch([0, 1, 2, 3])
    for u, v in zip(x[:4], y[:4]):
        assert torch.equal(u, v)
    assert all(torch.equal(x[4][k], y[4][k]) for k in x[4])


from test_restore_gpu import restorer  # noqa: E402,F401  (the module-scoped restorer fixture of the restoration tests)


def test_restore_file_takes_flac(restorer, tmp_path):  # noqa: F811
    from test_restore_gpu import GAPS, recording
    pcm = np.rint(recording(seed=7).astype(np.float64) * 32768).astype(np.int64)
    for s, e in GAPS:
        pcm[s:e] = 0
    n = len(pcm)
    sizes = [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
    c = C.make(pcm, 16, blocksizes=sizes, frames=dict(subframes=R.fixed(2)))
    (tmp_path / "in.flac").write_bytes(c.data)
    C.write_wav(tmp_path / "in.wav", c)
    a = restorer.restore_file(tmp_path / "in.flac", tmp_path / "a.wav")
    b = restorer.restore_file(tmp_path / "in.wav", tmp_path / "b.wav")
    assert [p["gap"] for p in a["windows"]] == GAPS == [p["gap"] for p in b["windows"]]
    assert torch.equal(a["restored"], b["restored"])
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
