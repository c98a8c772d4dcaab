"""FLAC decoding (csrc/flac_core.h + csrc/flac.hip; specification tests/flac_ref.py).

`decode_files` decodes a list of files in batches: on the HIP device every frame of every file of a batch at once (scan for
frame headers, parse every candidate, chain, decode: five launches and one host read per batch), or with the serial host
decoder on a thread pool when there is no device.  Both run the same decoder core and give the same bits.

No file written by libFLAC or any other encoder was available when this was built: the format is pinned by
tests/flac_ref.py, written from the published specification.  Not built: MD5 verification (frames are covered by CRC-16),
32-bit samples, streams of unknown length, ID3v2 / Ogg wrappers, any encoder.
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
          5: "bad frame header", 6: "reserved subframe or residual type", 7: "CRC-16 mismatch", 8: "sample count mismatch"}
META = 12
HOST_THREADS = 16


class FlacError(ValueError):
    """a file the decoder rejects; `.status` is the code of include/nppc_hip.h, `.path` the file"""

    def __init__(self, path, status):
        super().__init__(f"{path}: FLAC status {status}: {STATUS.get(status, 'unknown')}")
        self.path, self.status = path, status


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


def _decode_host(buf, name, info, out):
    pcm = np.empty((info.channels, info.total_samples), np.int32)
    mono = np.empty(info.total_samples, np.float32) if out == "mono" else None
    st = ctypes.c_int()
    H.call("nppc_flac_decode_host", buf.ctypes.data, buf.nbytes, pcm.ctypes.data, pcm.size,
           mono.ctypes.data if mono is not None else 0, info.total_samples, ctypes.addressof(st))
    if st.value:
        raise FlacError(name, st.value)
    return torch.from_numpy(mono if mono is not None else pcm)


def _decode_batch_device(bufs, names, infos, out, device):
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
    d_status = torch.empty(nf + 1, dtype=torch.int32, device=device)
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
            status = d_status.cpu().tolist()                          # the one host read of the batch
            if not status[nf] or cap >= total // 4 + 1:
                break
            cap = total // 4 + 1
    for f in range(nf):
        if status[f]:
            raise FlacError(names[f], status[f])
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


def decode_files(paths, out="mono", backend="auto", device="cuda", max_batch_bytes=256 << 20):
    """paths (or bytes objects) -> (tensors, infos).  out="pcm": int32 [C, n] per file; out="mono": float32 [n] =
    (sum over channels of pcm / 2^(bits-1), left to right in fp32) / C, what data._decode_wav yields for the same PCM.
    backend "auto" takes the device when there is one, else the host decoder.  Files are grouped into batches of at most
    max_batch_bytes (a larger file is a batch of its own).  A file the decoder rejects raises FlacError with its name."""
    if out not in ("mono", "pcm"):
        raise ValueError(f"out must be 'mono' or 'pcm', got {out!r}")
    on_device = _use_device(backend)
    paths = list(paths)
    if not on_device:
        def one(src):
            buf, name = _read(src)
            info = _probe(buf, name)
            return _decode_host(buf, name, info, out), info
        with ThreadPoolExecutor(max_workers=max(1, min(HOST_THREADS, os.cpu_count() or 1, len(paths) or 1))) as ex:
            res = list(ex.map(one, paths))                            # ctypes releases the GIL inside the decoder
        return [t for t, _ in res], [i for _, i in res]
    tensors, infos = [], []
    batch, used = [], 0

    def flush():
        nonlocal batch, used
        if batch:
            bufs, names, binfos = zip(*batch)
            tensors.extend(_decode_batch_device(list(bufs), list(names), list(binfos), out, device))
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
