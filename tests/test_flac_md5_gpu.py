"""GPU: flac_md5_kernel (nppc_flac_md5 through nppc_audio.flac.pcm_md5 and decode_files(verify_md5=True)) against hashlib
over messages built with numpy (tests/test_flac_md5_cpu.py builds them) and against nppc_flac_md5_host: every format at
the padding boundaries in one launch of 130 files, any order, each file alone, unaligned 16-bit files, and one batch that
mixes a correct file, one without an MD5, one with a wrong MD5 and one with a broken CRC-16.  Every input is well formed
at the memory level; everything is equality."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as R
from test_flac_md5_cpu import check_verified_decode, flipped, md5_cases, oracle, random_pcm, stated_streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    """130 files: the formats and boundary lengths of the CPU test and 26 more 16-bit files of whole and ragged blocks, up to
    20 blocks, n = 0 among them -> (device tensors, bits, hashlib digests)"""
    cases = md5_cases()
    for n in (32, 64, 65, 96, 127, 128, 129, 160, 255, 320, 511, 640, 643):
        cases.append((random_pcm(1, 16, n, 5000 + n), 16))
        cases.append((random_pcm(2, 16, n // 2 + (n & 1), 6000 + n), 16))
    assert len(cases) == 130
    blocks = [p.size * ((b + 7) // 8) // 64 for p, b in cases]
    assert min(blocks) == 0 and 20 <= max(blocks) <= 26
    dev = [torch.from_numpy(p).cuda() for p, _ in cases]
    return dev, [b for _, b in cases], [oracle(p, b) for p, b in cases]


def test_one_launch_of_130_files_equals_hashlib_and_the_host_hash(batch):
    from nppc_audio import flac
    dev, bps, want = batch
    got = flac.pcm_md5(dev, bps)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f, tuple(dev[f].shape), bps[f], g.hex(), w.hex())
    assert flac.pcm_md5([t.cpu() for t in dev], bps) == want                    # nppc_flac_md5_host
    assert flac.pcm_md5([t.cpu() for t in dev[:5]], bps[:5], backend="device") == want[:5]
    assert flac.pcm_md5(dev[:5], bps[:5], backend="host") == want[:5]
    assert flac.pcm_md5(torch.zeros(1, 0, dtype=torch.int32, device="cuda"), 16) == [hashlib.md5(b"").digest()]


def test_order_alone_and_repeat(batch):
    from nppc_audio import flac
    dev, bps, want = batch
    nf = len(dev)
    base = flac._md5_order([t.shape[0] for t in dev], bps, [t.shape[1] for t in dev])
    length = [t.numel() * ((b + 7) // 8) for t, b in zip(dev, bps)]
    assert sorted(base.tolist()) == list(range(nf)) and all(length[a] >= length[b] for a, b in zip(base[:-1], base[1:]))
    shuffled = np.random.Generator(np.random.PCG64(5)).permutation(nf)
    for order in (base, base[::-1], np.arange(nf), shuffled, base):               # the last: a second run of the first
        assert flac._pcm_md5_device(dev, bps, order=np.ascontiguousarray(order, np.int32)) == want
    for f in range(0, nf, 3):
        assert flac.pcm_md5(dev[f], bps[f]) == [want[f]], f


def raw_md5(flat, meta, order, expected=None, status=None):
    """nppc_flac_md5 itself -> (digest [nf, 16] uint8, verdict [nf]) on the host"""
    from nppc_audio import _hip as H
    nf = meta.shape[0]
    digest = torch.full((nf, 16), 0xAA, dtype=torch.uint8, device="cuda")
    verdict = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
    H.call("nppc_flac_md5", flat, flat.numel(), torch.from_numpy(meta).cuda(), nf,
           torch.from_numpy(np.ascontiguousarray(order, np.int32)).cuda(), expected, status, digest, verdict, H.stream())
    return digest.cpu().numpy(), verdict.cpu().tolist()


def test_unaligned_16_bit_files_and_verdicts():
    """16-bit mono and stereo behind 0..3 other samples: every residue of the pcm offset modulo the 16-byte load, and for
    stereo an odd n, so the two channels differ in alignment"""
    pcms, metas, off = [], [], 0
    for k in range(4):
        for ch, n in ((1, 200), (2, 101), (2, 100), (1, 64 + k)):
            p = random_pcm(ch, 16, n, 7000 + 10 * k + ch + n)
            pcms.append(p)
            metas.append((ch, 16, n, off))
            off += p.size
        filler = random_pcm(1, 8, k + 1, 7100 + k)                     # shifts what follows by k + 1 samples
        pcms.append(filler)
        metas.append((1, 8, k + 1, off))
        off += filler.size
    nf = len(pcms)
    assert {m[3] % 4 for m in metas if m[1] == 16} == {0, 1, 2, 3}
    meta = np.zeros((nf, 12), np.int64)
    meta[:, 3], meta[:, 4], meta[:, 7], meta[:, 9] = np.array(metas).T
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pcms])).cuda()
    assert flat.data_ptr() % 16 == 0
    want = [oracle(p, m[1]) for p, m in zip(pcms, metas)]
    digest, verdict = raw_md5(flat, meta, np.arange(nf))
    assert [digest[f].tobytes() for f in range(nf)] == want and verdict == [0] * nf     # expected null: digests only
    # verdicts: match, absent (sixteen zero bytes), mismatch in the last bit, and a file the chain pass rejected
    expected = np.stack([np.frombuffer(w, np.uint8) for w in want]).copy()
    expected[1] = 0
    expected[2, 15] ^= 1
    status = np.zeros(nf, np.int32)
    status[3] = R.CRC16
    digest, verdict = raw_md5(flat, meta, np.arange(nf)[::-1], torch.from_numpy(expected).cuda(), torch.from_numpy(status).cuda())
    assert verdict == [1, 0, 2, 0] + [1] * (nf - 4)
    assert not digest[3].any() and [digest[f].tobytes() for f in range(nf) if f != 3] == [w for f, w in enumerate(want) if f != 3]
    # a file whose samples would lie outside pcm_elems, or whose format cannot be, is skipped, not read
    bad = meta.copy()
    bad[0, 9], bad[1, 3], bad[2, 4], bad[4, 7] = flat.numel() - 10, 9, 33, -1
    digest, verdict = raw_md5(flat, bad, np.arange(nf), torch.from_numpy(expected).cuda())
    assert verdict[:5] == [0, 0, 0, 1, 0] and not digest[[0, 1, 2, 4]].any() and digest[3].tobytes() == want[3]


def test_mixed_batch_one_host_read():
    """a correct file, one without an MD5, one with a wrong MD5, one with a broken CRC-16: the four decode launches and
    the MD5 launch on one status / verdict / digest buffer, read once"""
    from nppc_audio import _hip as H
    from nppc_audio import flac
    streams = stated_streams()
    good, c_good = streams["speech"]
    absent = C.cases()["ch2_mid_side"]
    wrong, c_wrong = streams["ch3"]
    wrong = flipped(wrong)
    crc = C.corrupt_files()[0][0]
    crc = crc[:26] + bytes(range(1, 17)) + crc[42:]                 # it states an MD5, which is never looked at
    datas = [good, absent.data, wrong, crc]
    with pytest.raises(flac.FlacError) as e:
        flac.decode_files(datas, out="mono", backend="device", verify_md5=True)
    assert e.value.status == 9 and wrong[26:42].hex() in str(e.value) and oracle(c_wrong.pcm, 16).hex() in str(e.value)
    with pytest.raises(flac.FlacError) as e:                        # the first bad file by index is the one named
        flac.decode_files([good, crc, wrong], out="mono", backend="device", verify_md5=True)
    assert e.value.status == R.CRC16
    with pytest.raises(flac.FlacError) as e:                        # as before without the check
        flac.decode_files(datas, out="mono", backend="device")
    assert e.value.status == R.CRC16

    bufs = [np.frombuffer(d, np.uint8) for d in datas]
    infos = [flac._probe(b, "x") for b in bufs]
    nf = len(bufs)
    begin = np.concatenate([[0], np.cumsum([b.size for b in bufs])])
    off = np.concatenate([[0], np.cumsum([i.channels * i.total_samples for i in infos])])
    meta = np.zeros((nf, 12), np.int64)
    meta[:, 0], meta[:, 1], meta[:, 9] = begin[:-1], begin[1:], off[:-1]
    for f, i in enumerate(infos):
        meta[f, 2:9] = (i.sample_rate, i.channels, i.bits_per_sample, i.min_blocksize, i.max_blocksize, i.total_samples,
                        i.first_frame_offset)
    dev = torch.device("cuda")
    d_bytes = torch.from_numpy(np.concatenate(bufs)).to(dev)
    d_meta = torch.from_numpy(meta).to(dev)
    d_stated = torch.from_numpy(np.stack([b[26:42] for b in bufs])).to(dev)
    d_order = torch.from_numpy(flac._md5_order(meta[:, 3], meta[:, 4], meta[:, 7])).to(dev)
    cap = int(begin[-1]) // 4 + 1
    elems = ctypes.c_long()
    H.call("nppc_flac_work_elems", cap, ctypes.byref(elems))
    work = torch.empty(elems.value, dtype=torch.int64, device=dev)
    pcm = torch.full((int(off[-1]),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    buf = torch.full((nf + 1 + 5 * nf,), -1, dtype=torch.int32, device=dev)   # status | verdict | digest
    reads = []

    def read(t):
        reads.append(t.numel())
        return t.cpu()

    s = H.stream()
    H.call("nppc_flac_scan", d_bytes, int(begin[-1]), d_meta, nf, work, cap, s)
    H.call("nppc_flac_parse", d_bytes, d_meta, nf, work, cap, s)
    H.call("nppc_flac_chain", d_bytes, d_meta, nf, work, cap, buf, s)
    H.call("nppc_flac_decode", d_bytes, d_meta, nf, work, cap, pcm, pcm.numel(), None, 0, s)
    H.call("nppc_flac_md5", pcm, pcm.numel(), d_meta, nf, d_order, d_stated, buf, buf[2 * nf + 1:], buf[nf + 1:2 * nf + 1], s)
    host = read(buf)
    assert reads == [6 * nf + 1]                                    # one host read holds all of it
    assert host[:nf + 1].tolist() == [0, 0, 0, R.CRC16, 0]
    assert host[nf + 1:2 * nf + 1].tolist() == [1, 0, 2, 0]
    digest = host[2 * nf + 1:].numpy().view(np.uint8).reshape(nf, 16)
    assert digest[0].tobytes() == oracle(c_good.pcm, 16) == good[26:42]
    assert digest[1].tobytes() == oracle(absent.pcm, 16)            # hashed, with nothing to compare it with
    assert digest[2].tobytes() == oracle(c_wrong.pcm, 16) != wrong[26:42]
    assert not digest[3].any()                                      # the CRC-bad file is skipped, not hashed


def test_device_and_host_backends_agree(tmp_path):
    from nppc_audio import flac
    check_verified_decode("device")
    streams = stated_streams()
    datas = [d for d, _ in streams.values()]
    for out in ("mono", "pcm"):
        a, _ = flac.decode_files(datas, out=out, backend="device", verify_md5=True)
        b, _ = flac.decode_files(datas, out=out, backend="host", verify_md5=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), out
    small, _ = flac.decode_files(datas, out="pcm", backend="device", verify_md5=True, max_batch_bytes=20000)   # several batches
    assert all(torch.equal(x, y) for x, y in zip(small, b))
    # the callers pass it through: a stated MD5 that is wrong stops restore_file's and the dataset's decode
    from nppc_audio.data import _decode_flac
    data, c = streams["speech"]
    (tmp_path / "ok.flac").write_bytes(data)
    (tmp_path / "bad.flac").write_bytes(flipped(data))
    good = _decode_flac(tmp_path / "ok.flac", c.rate)
    with pytest.raises(flac.FlacError, match="bad.flac") as e:
        _decode_flac(tmp_path / "bad.flac", c.rate)
    assert e.value.status == 9
    assert torch.equal(_decode_flac(tmp_path / "bad.flac", c.rate, verify_md5=False), good)
