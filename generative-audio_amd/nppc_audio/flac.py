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
reads it the same way.  Not built: 32-bit samples, streams of unknown length, ID3v2 / Ogg wrappers.

Encoding (csrc/flac_enc_core.h + csrc/flac_enc.hip; specification tests/flac_enc_ref.py):
`encode_pcm` turns int32 PCM into FLAC streams, `encode_waves` quantises fp32 waveforms first, `write_files` stores them.
Lossless, fixed predictors with exact Rice-parameter search, one stated decision rule: the bytes are a function of the
samples alone, the same from the serial host encoder and from the device (plan, scan, MD5, write: four launches, one small
host read and one copy of exactly the encoded bytes per batch).  predictor="lpc" (specification
tests/flac_lpc_ref.py) adds LPC subframes of order 1..max_lpc_order to the candidates of every subframe, costed exactly like
the fixed ones, so a stream is never longer than the fixed stream of the same samples; the default stays "fixed".  Not
built: escape partitions, wasted bits, variable block sizes, seek tables and comments, more than two channels on the
device, error feedback in the quantiser, a search over the coefficient precision.
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
    if backend == "hip":                                              # the encoder's name for the device
        backend = "device"
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


# ---- encoding --------------------------------------------------------------------------------------------------------
ENC_BITS = (8, 12, 16, 20, 24)
ENC_MIN_BLOCK, ENC_MAX_BLOCK = 16, 4608
ENC_PREDICTORS = ("fixed", "lpc")
ENC_MAX_LPC_ORDER = 12
PLAN_INTS, PLAN_LPC_INTS = 8, 34                                      # NPPC_FLAC_ENC_PLAN, NPPC_FLAC_ENC_PLAN_LPC


def _enc_args(bits_per_sample, sample_rate, block_size):
    if bits_per_sample not in ENC_BITS:
        raise ValueError(f"bits_per_sample must be one of {ENC_BITS}, got {bits_per_sample!r}")
    if not isinstance(block_size, int) or not ENC_MIN_BLOCK <= block_size <= ENC_MAX_BLOCK:
        raise ValueError(f"block_size must be an int in {ENC_MIN_BLOCK}..{ENC_MAX_BLOCK}, got {block_size!r}")
    if not 1 <= int(sample_rate) < 1 << 20:
        raise ValueError(f"sample_rate must be in 1..{(1 << 20) - 1}, got {sample_rate!r}")


def _enc_predictor(predictor, max_lpc_order):
    """-> the LPC order limit the C entry points take: 0 for the fixed predictors"""
    if predictor not in ENC_PREDICTORS:
        raise ValueError(f"predictor must be one of {ENC_PREDICTORS}, got {predictor!r}")
    if isinstance(max_lpc_order, bool) or not isinstance(max_lpc_order, int) or not 1 <= max_lpc_order <= ENC_MAX_LPC_ORDER:
        raise ValueError(f"max_lpc_order must be an int in 1..{ENC_MAX_LPC_ORDER}, got {max_lpc_order!r}")
    return max_lpc_order if predictor == "lpc" else 0


def _enc_bound(n, channels, bps, block_size):
    nbytes, frames = ctypes.c_long(), ctypes.c_long()
    H.call("nppc_flac_enc_bound", n, channels, bps, block_size, ctypes.byref(nbytes), ctypes.byref(frames))
    return nbytes.value, frames.value


def _encode_host(a, bps, rate, block_size, lpc=0):
    """nppc_flac_encode_host (lpc = 0) or nppc_flac_encode_host_lpc of a C-contiguous int32 array [C, n]"""
    cap, _ = _enc_bound(a.shape[1], a.shape[0], bps, block_size)
    out = np.empty(cap, np.uint8)
    nbytes = ctypes.c_long()
    if lpc:
        H.call("nppc_flac_encode_host_lpc", a.ctypes.data, a.shape[1], a.shape[0], bps, rate, block_size, lpc, out.ctypes.data,
               cap, ctypes.byref(nbytes))
    else:
        H.call("nppc_flac_encode_host", a.ctypes.data, a.shape[1], a.shape[0], bps, rate, block_size, out.ctypes.data, cap,
               ctypes.byref(nbytes))
    return out[:nbytes.value].tobytes()


def _encode_host_pool(arrays, bps, rate, block_size, lpc=0):
    with ThreadPoolExecutor(max_workers=max(1, min(HOST_THREADS, os.cpu_count() or 1, len(arrays) or 1))) as ex:
        return list(ex.map(lambda a: _encode_host(a, bps, rate, block_size, lpc), arrays))   # ctypes releases the GIL


def _encode_device(flat, channels, lengths, bps, rate, block_size, lpc=0):
    """flat: int32 device tensor, the files' planar [C, n] blocks back to back -> list of bytes.  Four launches, one small
    host read (per-file begin / end / min / max frame size, the batch's byte count, the digests), one copy of the bytes.
    lpc: 0 for the fixed predictors, else the LPC order limit (the wider plan record and its three entry points)."""
    dev = flat.device
    nf = len(lengths)
    channels, lengths = np.asarray(channels, np.int64), np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(channels * lengths)])
    frames = -(-lengths // block_size)
    meta = np.zeros((nf, META), np.int64)
    meta[:, 2], meta[:, 3], meta[:, 4], meta[:, 5], meta[:, 6] = rate, channels, bps, block_size, block_size
    meta[:, 7], meta[:, 9] = lengths, off[:-1]
    ftab = np.empty((int(frames.sum()), 2), np.int32)
    ftab[:, 0] = np.repeat(np.arange(nf), frames)
    ftab[:, 1] = np.arange(len(ftab)) - np.repeat(np.cumsum(frames) - frames, frames)
    shapes = {(int(n), int(c)) for n, c in zip(lengths, channels)}   # the shape query, once per distinct file shape
    bound = {k: _enc_bound(k[0], k[1], bps, block_size)[0] for k in shapes}
    cap = sum(bound[(int(n), int(c))] for n, c in zip(lengths, channels))
    nfr = len(ftab)
    d_meta, d_ftab = torch.from_numpy(meta).to(dev), torch.from_numpy(ftab).to(dev)
    d_order = torch.from_numpy(_md5_order(meta[:, 3], meta[:, 4], meta[:, 7])).to(dev)
    small = torch.empty(4 * (nf + 1) + 2 * nf, dtype=torch.int64, device=dev)
    stats, digest = small[:4 * (nf + 1)], small[4 * (nf + 1):].view(torch.uint8)
    verdict = torch.empty(nf, dtype=torch.int32, device=dev)
    plan = torch.empty(nfr * (PLAN_LPC_INTS if lpc else PLAN_INTS), dtype=torch.int32, device=dev)
    goff = torch.empty(nfr, dtype=torch.int64, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = H.stream()
        if lpc:
            H.call("nppc_flac_enc_plan_lpc", flat, flat.numel(), d_meta, nf, d_ftab, nfr, bps, block_size, lpc, plan, s)
            H.call("nppc_flac_enc_scan_stride", plan, PLAN_LPC_INTS, d_ftab, nfr, nf, goff, stats, s)
        else:
            H.call("nppc_flac_enc_plan", flat, flat.numel(), d_meta, nf, d_ftab, nfr, bps, block_size, plan, s)
            H.call("nppc_flac_enc_scan", plan, d_ftab, nfr, nf, goff, stats, s)
        H.call("nppc_flac_md5", flat, flat.numel(), d_meta, nf, d_order, None, None, digest, verdict, s)
        H.call("nppc_flac_enc_write_lpc" if lpc else "nppc_flac_enc_write", flat, flat.numel(), d_meta, nf, d_ftab, nfr, bps, rate,
               block_size, plan, goff, stats, digest, out, cap, s)
        host = small.cpu().numpy()[:4 * (nf + 1)].reshape(nf + 1, 4)  # the small read
        total = int(host[nf, 0])
        data = out[:total].cpu().numpy()                              # exactly the encoded bytes
    return [data[int(host[f, 0]):int(host[f, 1])].tobytes() for f in range(nf)]


def _enc_backend(backend):
    if backend not in ("auto", "hip", "device", "host"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'host', got {backend!r}")
    return _use_device("device" if backend == "hip" else backend)


def encode_pcm(pcm, bits_per_sample, sample_rate=16000, block_size=4096, backend="auto", device="cuda", predictor="fixed",
               max_lpc_order=8):
    """int32 PCM -> FLAC streams: a list of [C, n] tensors (host or device) -> a list of bytes.  One call has one sample
    size, rate and block size; every file has its own length and channel count.  backend "host" runs the serial encoder on
    a pool of 16 threads (1..8 channels), "hip" the device kernels (1 or 2 channels) and "auto" the device when there is
    one; both give the same bytes.  ValueError, before anything is launched, for an empty file, an unsupported
    bits_per_sample or block_size, more than 2 channels on the device, or a sample outside bits_per_sample bits.
    predictor "fixed" (the default) tries the fixed predictors of order 0..4; "lpc" also LPC subframes of order
    1..max_lpc_order (at most 12), each costed exactly, so its streams are never longer.  Any other predictor or order
    limit is a ValueError before anything is launched."""
    _enc_args(bits_per_sample, sample_rate, block_size)
    lpc = _enc_predictor(predictor, max_lpc_order)
    tensors = [pcm] if isinstance(pcm, torch.Tensor) else list(pcm)
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or not 1 <= t.shape[0] <= 8:
            raise ValueError("encode_pcm takes int32 tensors [C, n] with 1 <= C <= 8")
        if t.shape[1] == 0:
            raise ValueError("encode_pcm: a file with no samples")
    on_device = _enc_backend(backend)
    if on_device and any(t.shape[0] > 2 for t in tensors):
        raise ValueError("encode_pcm: the device encoder takes 1 or 2 channels")
    if not tensors:
        return []
    lo, hi = -(1 << (bits_per_sample - 1)), (1 << (bits_per_sample - 1)) - 1
    if not on_device:
        arrays = [np.ascontiguousarray(t.cpu().numpy()) for t in tensors]
        if any(a.min() < lo or a.max() > hi for a in arrays):
            raise ValueError(f"encode_pcm: a sample lies outside {bits_per_sample} bits")
        return _encode_host_pool(arrays, bits_per_sample, int(sample_rate), block_size, lpc)
    tensors = [t if t.is_cuda else t.to(device) for t in tensors]
    flat = tensors[0].contiguous().view(-1) if len(tensors) == 1 else torch.cat([t.reshape(-1) for t in tensors])
    mn, mx = torch.aminmax(flat)
    if int(mn) < lo or int(mx) > hi:
        raise ValueError(f"encode_pcm: a sample lies outside {bits_per_sample} bits")
    return _encode_device(flat, [t.shape[0] for t in tensors], [t.shape[1] for t in tensors], bits_per_sample, int(sample_rate),
                          block_size, lpc)


def quantize_waves_host(waves, bits_per_sample=16):
    """clip(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1) in fp32, halves to even: what nppc_pcm_quantize computes"""
    full = np.float32(1 << (bits_per_sample - 1))
    y = np.rint(np.asarray(waves, np.float32) * full)
    return np.clip(np.nan_to_num(y, nan=0.0, posinf=np.inf, neginf=-np.inf), -full, full - 1).astype(np.int32)


def encode_waves(waves, lengths=None, sample_rate=16000, bits_per_sample=16, block_size=4096, backend="auto", device="cuda",
                 predictor="fixed", max_lpc_order=8):
    """fp32 waveforms [V, L] (or [L]) in [-1, 1) -> V mono FLAC streams of lengths[v] samples each (default L): quantised as
    clip(rint(x 2^(bits-1))) (on the device by nppc_pcm_quantize, straight into the encoder's layout), then encoded.
    predictor, max_lpc_order: as for encode_pcm."""
    _enc_args(bits_per_sample, sample_rate, block_size)
    lpc = _enc_predictor(predictor, max_lpc_order)
    if not isinstance(waves, torch.Tensor) or waves.dtype != torch.float32 or waves.dim() not in (1, 2):
        raise ValueError("encode_waves takes a float32 tensor [V, L] or [L]")
    waves = waves.reshape(-1, waves.shape[-1])
    V, L = waves.shape
    lens = np.full(V, L, np.int64) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), np.int64).reshape(-1)
    if len(lens) != V or (V and (lens.min() < 1 or lens.max() > L)):
        raise ValueError("encode_waves: lengths must be V values in 1..L")
    if not V:
        return []
    if not _enc_backend(backend):
        q = quantize_waves_host(waves.cpu().numpy(), bits_per_sample)
        return _encode_host_pool([np.ascontiguousarray(q[v:v + 1, :lens[v]]) for v in range(V)], bits_per_sample,
                                 int(sample_rate), block_size, lpc)
    waves = (waves if waves.is_cuda else waves.to(device)).contiguous()
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = torch.empty(int(off[-1]), dtype=torch.int32, device=waves.device)
    d_len, d_off = torch.from_numpy(lens).to(waves.device), torch.from_numpy(off[:-1].copy()).to(waves.device)
    for v0 in range(0, V, 65535):                                     # the launch's grid limit
        v1 = min(V, v0 + 65535)
        with torch.cuda.device(waves.device):
            H.call("nppc_pcm_quantize", waves[v0:v1], L, d_len[v0:v1], v1 - v0, bits_per_sample, flat, d_off[v0:v1],
                   flat.numel(), H.stream())
    return _encode_device(flat, np.ones(V, np.int64), lens, bits_per_sample, int(sample_rate), block_size, lpc)


def write_files(paths, streams):
    """streams (what encode_pcm / encode_waves return) -> files; directories are made as needed"""
    paths = [str(p) for p in paths]
    if len(paths) != len(streams):
        raise ValueError(f"{len(paths)} paths for {len(streams)} streams")
    for p, b in zip(paths, streams):
        d = os.path.dirname(p)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(p, "wb") as f:
            f.write(b)


def write_waves(paths, waves, sample_rate=16000, fmt="flac", lengths=None, backend="auto", predictor="fixed", max_lpc_order=8):
    """fp32 waveforms [V, L] -> V 16-bit mono files: fmt "flac" (encode_waves: the whole batch in one device call) or "wav"
    (the same samples, through scipy).  predictor, max_lpc_order: the FLAC encoder's, as for encode_pcm; "wav" ignores them
    once they are checked."""
    if fmt not in ("flac", "wav"):
        raise ValueError(f"fmt must be 'flac' or 'wav', got {fmt!r}")
    _enc_predictor(predictor, max_lpc_order)
    waves = waves.detach().reshape(-1, waves.shape[-1])
    if fmt == "flac":
        write_files(paths, encode_waves(waves.float(), lengths, sample_rate, 16, backend=backend, predictor=predictor,
                                        max_lpc_order=max_lpc_order))
        return
    from scipy.io import wavfile
    paths = [str(p) for p in paths]
    if len(paths) != waves.shape[0]:
        raise ValueError(f"{len(paths)} paths for {waves.shape[0]} waveforms")
    pcm = quantize_waves_host(waves.float().cpu().numpy(), 16).astype(np.int16)
    for v, p in enumerate(paths):
        d = os.path.dirname(p)
        if d:
            os.makedirs(d, exist_ok=True)
        wavfile.write(p, int(sample_rate), pcm[v, :None if lengths is None else int(lengths[v])])
