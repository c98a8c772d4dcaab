"""FLAC decoding (csrc/flac_core.h + csrc/flac.hip; specification tests/flac_ref.py) and the MD5 of
the decoded samples (csrc/md5_core.h + csrc/flac_md5.hip).

`decode_files` decodes a list of files in batches: on the HIP device every frame of every file of a batch at once (scan for
frame headers, parse every candidate, chain, decode: five launches and one host read per batch), or with the serial host
decoder on a thread pool when there is no device.  Both run the same decoder core and give the same bits.

STREAMINFO holds the MD5 of the unencoded samples, written by the encoder: `decode_files(..., verify_md5=True)` hashes what
was decoded (on the device one more launch, one lane per file, and still one host read per batch; on the host inside the
worker threads) and raises FlacError(path, 9) when a file that states an MD5 decodes to other samples.  `stream_md5` reads
the field, `pcm_md5` hashes int32 PCM where it lies.

No file written by libFLAC or any other encoder was available when this was built: the format is pinned by
tests/flac_ref.py, written from the published specification; the MD5 of the first LibriSpeech file decides whether libFLAC
reads it the same way.  Not built: 32-bit samples, streams of unknown length, ID3v2 / Ogg wrappers, any encoder.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

from . import _hip as H

STATUS = {1: "bad marker (not a FLAC stream)", 2: "truncated", 3: "no or bad STREAMINFO",
          4: "unsupported (32-bit or odd-sized samples, unknown length, ID3v2 prefix or Ogg container)",
          5: "bad frame header", 6: "reserved subframe or residual type", 7: "CRC-16 mismatch", 8: "sample count mismatch",
          9: "the decoded samples do not match STREAMINFO's MD5"}
META = 12
HOST_THREADS = 16


class FlacError(ValueError):
    """a file the decoder rejects; `.status` is the code of include/nppc_hip.h, `.path` the file"""

    def __init__(self, path, status, detail=None):
        super().__init__(f"{path}: FLAC status {status}: {STATUS.get(status, 'unknown')}" + (f" ({detail})" if detail else ""))
        self.path, self.status = path, status


def _md5_mismatch(name, stated, computed):
    return FlacError(name, 9, f"STREAMINFO states {bytes(stated).hex()}, the decoded samples give {bytes(computed).hex()}")


class FlacInfo(NamedTuple):
    sample_rate: int
    channels: int
    bits_per_sample: int
    total_samples: int
    min_blocksize: int
    max_blocksize: int
    first_frame_offset: int


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(src), dtype=np.uint8), "<bytes>"
    return np.fromfile(str(src), dtype=np.uint8), str(src)


def _probe(buf, name):
    if buf.nbytes >= 2 ** 31:
        raise FlacError(name, 4)
    info = (ctypes.c_long * 8)()
    st = ctypes.c_int()
    data = buf if buf.nbytes else np.zeros(1, np.uint8)
    H.call("nppc_flac_probe", data.ctypes.data, buf.nbytes, ctypes.addressof(info), ctypes.addressof(st))
    if st.value:
        raise FlacError(name, st.value)
    return FlacInfo(*[int(v) for v in info[:7]])


def probe(path_or_bytes) -> FlacInfo:
    """STREAMINFO of one file (host only): walks the metadata blocks, whatever they are, to the first frame"""
    return _probe(*_read(path_or_bytes))


def stream_md5(path_or_bytes):
    """the MD5 of the unencoded samples that STREAMINFO states (host only): 16 bytes, or None when they are all zero, the
    format's "not computed".  A file the probe rejects raises FlacError."""
    buf, name = _read(path_or_bytes)
    if buf.nbytes >= 2 ** 31:
        raise FlacError(name, 4)
    md5 = (ctypes.c_ubyte * 16)()
    present, st = ctypes.c_int(), ctypes.c_int()
    data = buf if buf.nbytes else np.zeros(1, np.uint8)
    H.call("nppc_flac_stream_md5", data.ctypes.data, buf.nbytes, ctypes.addressof(md5), ctypes.addressof(present),
           ctypes.addressof(st))
    if st.value:
        raise FlacError(name, st.value)
    return bytes(md5) if present.value else None


def _md5_host(pcm, n, channels, bps):
    """nppc_flac_md5_host of a C-contiguous int32 array [channels, n]"""
    digest = (ctypes.c_ubyte * 16)()
    H.call("nppc_flac_md5_host", pcm.ctypes.data if n else 0, n, channels, bps, ctypes.addressof(digest))
    return bytes(digest)


def _md5_order(channels, bps, totals):
    """the files by descending message length (stable): lane i of nppc_flac_md5 hashes file order[i]"""
    length = np.asarray(totals, np.int64) * np.asarray(channels, np.int64) * ((np.asarray(bps, np.int64) + 7) // 8)
    return np.argsort(-length, kind="stable").astype(np.int32)


def _pcm_md5_device(tensors, bps, order=None):
    """[C, n] int32 device tensors -> digests, in one launch: the samples are laid back to back in one device buffer (a
    single contiguous tensor is hashed where it is)"""
    nf = len(tensors)
    dev = tensors[0].device
    sizes = np.array([t.numel() for t in tensors], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    flat = tensors[0].contiguous().view(-1) if nf == 1 else torch.cat([t.reshape(-1) for t in tensors])
    meta = np.zeros((nf, META), np.int64)
    meta[:, 3], meta[:, 4], meta[:, 7], meta[:, 9] = [t.shape[0] for t in tensors], bps, [t.shape[1] for t in tensors], off[:-1]
    if order is None:
        order = _md5_order(meta[:, 3], meta[:, 4], meta[:, 7])
    d_meta = torch.from_numpy(meta).to(dev)
    d_order = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev)
    digest = torch.empty(nf, 16, dtype=torch.uint8, device=dev)
    verdict = torch.empty(nf, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("nppc_flac_md5", flat if flat.numel() else None, flat.numel(), d_meta, nf, d_order, None, None, digest, verdict,
               H.stream())
    host = digest.cpu().numpy()
    return [host[f].tobytes() for f in range(nf)]


def pcm_md5(pcm, bits_per_sample, backend="auto"):
    """MD5 of FLAC's message of int32 PCM: one [C, n] tensor or a list of them -> a list of 16-byte digests.  The message is
    the samples interleaved by channel, each a signed little-endian integer of (bits_per_sample + 7) // 8 bytes; n = 0 gives
    the MD5 of the empty message.  bits_per_sample: one int, or one per tensor.  backend "auto" hashes device tensors on
    the device (where they are, one launch for the whole list) and host tensors with the serial host hash; "device" and
    "host" move them first."""
    if backend not in ("auto", "device", "host"):
        raise ValueError(f"backend must be 'auto', 'device' or 'host', got {backend!r}")
    tensors = [pcm] if isinstance(pcm, torch.Tensor) else list(pcm)
    bps = [int(bits_per_sample)] * len(tensors) if np.ndim(bits_per_sample) == 0 else [int(b) for b in bits_per_sample]
    if len(bps) != len(tensors):
        raise ValueError(f"{len(bps)} bits_per_sample for {len(tensors)} tensors")
    for t, b in zip(tensors, bps):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or not 1 <= t.shape[0] <= 8:
            raise ValueError("pcm_md5 takes int32 tensors [C, n] with 1 <= C <= 8")
        if not 4 <= b <= 32:
            raise ValueError(f"bits_per_sample must be 4..32, got {b}")
    if not tensors:
        return []
    if backend == "auto":
        where = {t.is_cuda for t in tensors}
        if len(where) > 1:
            raise ValueError("pcm_md5 with backend='auto' takes tensors that all lie on the device or all on the host")
        backend = "device" if where.pop() else "host"
    if backend == "device":
        H.require_gpu()
        tensors = [t if t.is_cuda else t.cuda() for t in tensors]
        return _pcm_md5_device(tensors, bps)
    out = []
    for t, b in zip(tensors, bps):
        a = np.ascontiguousarray(t.cpu().numpy())
        out.append(_md5_host(a, a.shape[1], a.shape[0], b))
    return out


def _decode_host(buf, name, info, out, verify_md5=False):
    pcm = np.empty((info.channels, info.total_samples), np.int32)
    mono = np.empty(info.total_samples, np.float32) if out == "mono" else None
    st = ctypes.c_int()
    H.call("nppc_flac_decode_host", buf.ctypes.data, buf.nbytes, pcm.ctypes.data, pcm.size,
           mono.ctypes.data if mono is not None else 0, info.total_samples, ctypes.addressof(st))
    if st.value:
        raise FlacError(name, st.value)
    if verify_md5:
        stated = buf[26:42].tobytes()                                 # the probe accepted a STREAMINFO at bytes 8..42
        if any(stated):
            computed = _md5_host(pcm, info.total_samples, info.channels, info.bits_per_sample)
            if computed != stated:
                raise _md5_mismatch(name, stated, computed)
    return torch.from_numpy(mono if mono is not None else pcm)


def _decode_batch_device(bufs, names, infos, out, device, verify_md5=False):
    nf = len(bufs)
    sizes = np.array([b.nbytes for b in bufs], np.int64)
    begin = np.concatenate([[0], np.cumsum(sizes)])
    pcm_n = np.array([i.channels * i.total_samples for i in infos], np.int64)
    mono_n = np.array([i.total_samples for i in infos], np.int64)
    pcm_off = np.concatenate([[0], np.cumsum(pcm_n)])
    mono_off = np.concatenate([[0], np.cumsum(mono_n)])
    meta = np.zeros((nf, META), np.int64)
    meta[:, 0], meta[:, 1] = begin[:-1], begin[1:]
    for f, i in enumerate(infos):
        meta[f, 2:9] = (i.sample_rate, i.channels, i.bits_per_sample, i.min_blocksize, i.max_blocksize, i.total_samples,
                        i.first_frame_offset)
    meta[:, 9], meta[:, 10] = pcm_off[:-1], mono_off[:-1]
    total = int(begin[-1])
    d_bytes = torch.from_numpy(np.concatenate(bufs)).to(device)
    d_meta = torch.from_numpy(meta).to(device)
    d_pcm = torch.empty(int(pcm_off[-1]), dtype=torch.int32, device=device)
    d_mono = torch.empty(int(mono_off[-1]), dtype=torch.float32, device=device) if out == "mono" else None
    stated = np.stack([b[26:42] for b in bufs]) if verify_md5 else None     # every probe accepted a STREAMINFO at 8..42
    verify_md5 = verify_md5 and bool(stated.any())                          # no file states an MD5: nothing to launch
    # status [nf + 1], and with verify_md5 verdict [nf] and digest [nf][16] behind it: one buffer, one host read
    d_status = torch.empty(nf + 1 + (5 * nf if verify_md5 else 0), dtype=torch.int32, device=device)
    if verify_md5:
        d_verdict, d_digest = d_status[nf + 1:2 * nf + 1], d_status[2 * nf + 1:]
        d_stated = torch.from_numpy(stated).to(device)
        d_order = torch.from_numpy(_md5_order(meta[:, 3], meta[:, 4], meta[:, 7])).to(device)
    # twice the frames the STREAMINFOs promise, plus room for chance headers inside payloads; total / 4 + 1 always suffices
    # (two headers lie at least four bytes apart) and is what a batch that overflows is run again with
    cap = min(2 * sum(-(-i.total_samples // i.min_blocksize) for i in infos) + total // 4096 + 1024, total // 4 + 1)
    with torch.cuda.device(d_bytes.device):
        while True:
            elems = ctypes.c_long()
            H.call("nppc_flac_work_elems", cap, ctypes.byref(elems))
            work = torch.empty(elems.value, dtype=torch.int64, device=device)
            s = H.stream()
            H.call("nppc_flac_scan", d_bytes, total, d_meta, nf, work, cap, s)
            H.call("nppc_flac_parse", d_bytes, d_meta, nf, work, cap, s)
            H.call("nppc_flac_chain", d_bytes, d_meta, nf, work, cap, d_status, s)
            H.call("nppc_flac_decode", d_bytes, d_meta, nf, work, cap, d_pcm, d_pcm.numel(), d_mono,
                   d_mono.numel() if d_mono is not None else 0, s)
            if verify_md5:                                            # skips the files the chain pass rejected
                H.call("nppc_flac_md5", d_pcm, d_pcm.numel(), d_meta, nf, d_order, d_stated, d_status, d_digest, d_verdict, s)
            host_status = d_status.cpu()                              # the one host read of the batch
            status = host_status[:2 * nf + 1].tolist()
            if not status[nf] or cap >= total // 4 + 1:
                break
            cap = total // 4 + 1
    for f in range(nf):
        if status[f]:
            raise FlacError(names[f], status[f])
        if verify_md5 and status[nf + 1 + f] == 2:
            computed = host_status[2 * nf + 1:].numpy().view(np.uint8).reshape(nf, 16)[f]
            raise _md5_mismatch(names[f], stated[f].tobytes(), computed.tobytes())
    if out == "mono":
        host = d_mono.cpu()
        return [host[mono_off[f]:mono_off[f + 1]].clone() for f in range(nf)]
    host = d_pcm.cpu()
    return [host[pcm_off[f]:pcm_off[f + 1]].view(infos[f].channels, infos[f].total_samples).clone() for f in range(nf)]


def _use_device(backend):
    if backend not in ("auto", "device", "host"):
        raise ValueError(f"backend must be 'auto', 'device' or 'host', got {backend!r}")
    if backend == "device":
        H.require_gpu()
    return backend == "device" or (backend == "auto" and torch.cuda.is_available())


def decode_files(paths, out="mono", backend="auto", device="cuda", max_batch_bytes=256 << 20, verify_md5=False):
    """paths (or bytes objects) -> (tensors, infos).  out="pcm": int32 [C, n] per file; out="mono": float32 [n] =
    (sum over channels of pcm / 2^(bits-1), left to right in fp32) / C, what data._decode_wav yields for the same PCM.
    backend "auto" takes the device when there is one, else the host decoder.  Files are grouped into batches of at most
    max_batch_bytes (a larger file is a batch of its own).  A file the decoder rejects raises FlacError with its name.
    verify_md5=True hashes the decoded samples of every file whose STREAMINFO states an MD5 (files without one pass) and
    raises FlacError(path, 9), with both digests in its message, when they differ; the tensors returned are the same."""
    if out not in ("mono", "pcm"):
        raise ValueError(f"out must be 'mono' or 'pcm', got {out!r}")
    on_device = _use_device(backend)
    paths = list(paths)
    if not on_device:
        def one(src):
            buf, name = _read(src)
            info = _probe(buf, name)
            return _decode_host(buf, name, info, out, verify_md5), info
        with ThreadPoolExecutor(max_workers=max(1, min(HOST_THREADS, os.cpu_count() or 1, len(paths) or 1))) as ex:
            res = list(ex.map(one, paths))                            # ctypes releases the GIL inside the decoder
        return [t for t, _ in res], [i for _, i in res]
    tensors, infos = [], []
    batch, used = [], 0

    def flush():
        nonlocal batch, used
        if batch:
            bufs, names, binfos = zip(*batch)
            tensors.extend(_decode_batch_device(list(bufs), list(names), list(binfos), out, device, verify_md5))
            infos.extend(binfos)
        batch, used = [], 0

    for src in paths:
        buf, name = _read(src)
        info = _probe(buf, name)                                      # on the host, before any device call
        if batch and used + buf.nbytes > max_batch_bytes:
            flush()
        batch.append((buf, name, info))
        used += buf.nbytes
    flush()
    return tensors, infos
