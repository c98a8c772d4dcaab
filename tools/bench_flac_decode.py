#!/usr/bin/env python3
"""Times the FLAC decoder (nppc_audio/flac.py, csrc/flac.hip, csrc/flac_core.h) on a LibriSpeech-shaped corpus: one 10 s
clip of 16 kHz / 16-bit shaped noise (blocksize 4096, LPC order 8, partition order 3) is encoded once by tests/flac_ref.py
and its bytes are used as 2048 files, 5.7 h of audio.

  (a) nppc_flac_decode_host, the serial decoder, on 1 thread and on a pool of 16 (ctypes releases the GIL)
  (b) the device path of one batch of all the files, phase by phase: upload, scan, parse, chain, decode, download; every
      phase ends in a device synchronise and is timed with the host clock
  (c) flac.decode_files end to end (bytes in host memory -> host tensors), backend "device" and backend "host"

Medians of --runs runs after --warmup warm-ups, with min and max.  The 1-thread pass of (a) decodes --host1-files of the
files (they are all the same bytes) and is scaled to the whole corpus; the json says so.

    python tools/bench_flac_decode.py [--files 2048] [--runs 20] [--warmup 5] [--host1-files 256] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generative-audio_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
COPY_TBS = 6.29          # the device copy rate README.md quotes, TB/s


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def repeat(fn, runs, warmup):
    out = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def corpus_clip(seconds):
    """the one clip whose bytes every file of the corpus holds (tools/bench_flac_md5.py times the same corpus)"""
    import flac_cases as C
    return C.speech(seconds, 1234)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host1-files", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_decode_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio import flac
    clip = corpus_clip(a.seconds)
    data = clip.data
    n, nf = clip.pcm.shape[1], a.files
    buf = np.frombuffer(data, np.uint8)
    info = flac.probe(data)
    res = {"tool": "bench_flac_decode", "files": nf, "clip_seconds": a.seconds, "clip_bytes": len(data), "clip_samples": n,
           "hours": nf * a.seconds / 3600, "compression": len(data) / (2 * n), "runs": a.runs, "warmup": a.warmup,
           "frames_per_file": -(-n // 4096)}
    total_samples, total_bytes = nf * n, nf * len(data)

    # ---- (a) the serial host decoder --------------------------------------------------------------------------------
    def host_one(pcm):
        st = ctypes.c_int()
        H.call("nppc_flac_decode_host", buf.ctypes.data, buf.size, pcm.ctypes.data, pcm.size, 0, 0, ctypes.addressof(st))
        assert st.value == 0

    one = np.empty(n, np.int32)
    host_one(one)
    assert np.array_equal(one, clip.pcm[0])
    n1 = min(a.host1_files, nf)
    t = repeat(lambda: [host_one(one) for _ in range(n1)], a.runs, a.warmup)
    res["host_1_thread_ms"] = stats([x * nf / n1 for x in t])
    res["host_1_thread_files_timed"] = n1
    bufs16 = [np.empty(n, np.int32) for _ in range(16)]

    def pool_run(ex):
        list(ex.map(lambda k: [host_one(bufs16[k]) for _ in range(k, nf, 16)], range(16)))

    with ThreadPoolExecutor(max_workers=16) as ex:
        res["host_16_threads_ms"] = stats(repeat(lambda: pool_run(ex), a.runs, a.warmup))
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()

    datas = [data] * nf
    res["decode_files_host_ms"] = stats(repeat(lambda: flac.decode_files(datas, out="mono", backend="host"), max(3, a.runs // 4), 1))

    if torch.cuda.is_available():
        dev = torch.device("cuda")
        res["device"] = torch.cuda.get_device_name(0)
        # ---- (b) the device path, phase by phase -------------------------------------------------------------------
        host_bytes = torch.from_numpy(np.tile(buf, nf))
        meta = np.zeros((nf, flac.META), np.int64)
        meta[:, 0] = np.arange(nf) * buf.size
        meta[:, 1] = meta[:, 0] + buf.size
        meta[:, 2:9] = (info.sample_rate, info.channels, info.bits_per_sample, info.min_blocksize, info.max_blocksize,
                        info.total_samples, info.first_frame_offset)
        meta[:, 9] = meta[:, 10] = np.arange(nf) * n
        host_meta = torch.from_numpy(meta)
        cap = 2 * nf * -(-n // info.min_blocksize) + total_bytes // 4096 + 1024
        elems = ctypes.c_long()
        H.call("nppc_flac_work_elems", cap, ctypes.byref(elems))
        work = torch.empty(elems.value, dtype=torch.int64, device=dev)
        pcm = torch.empty(total_samples, dtype=torch.int32, device=dev)
        mono = torch.empty(total_samples, dtype=torch.float32, device=dev)
        status = torch.empty(nf + 1, dtype=torch.int32, device=dev)
        phases = {k: [] for k in ("upload", "scan", "parse", "chain", "decode", "download")}
        state = {}

        def phase(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            state["ms"][name] = (time.perf_counter() - t0) * 1e3
            return out

        def one_batch():
            state["ms"] = {}
            s = H.stream()
            d_bytes, d_meta = phase("upload", lambda: (host_bytes.to(dev), host_meta.to(dev)))
            phase("scan", lambda: H.call("nppc_flac_scan", d_bytes, total_bytes, d_meta, nf, work, cap, s))
            phase("parse", lambda: H.call("nppc_flac_parse", d_bytes, d_meta, nf, work, cap, s))
            phase("chain", lambda: H.call("nppc_flac_chain", d_bytes, d_meta, nf, work, cap, status, s))
            phase("decode", lambda: H.call("nppc_flac_decode", d_bytes, d_meta, nf, work, cap, pcm, total_samples, mono,
                                           total_samples, s))
            st, out = phase("download", lambda: (status.cpu(), mono.cpu()))
            assert not st.any()
            return out

        for i in range(a.warmup + a.runs):
            out = one_batch()
            if i >= a.warmup:
                for k in phases:
                    phases[k].append(state["ms"][k])
        want = torch.from_numpy(clip.pcm[0].astype(np.float32) / 32768.0)
        assert torch.equal(out[:n], want) and torch.equal(out[-n:], want)
        res["device_phases_ms"] = {k: stats(v) for k, v in phases.items()}
        on_dev = sum(res["device_phases_ms"][k]["median"] for k in ("scan", "parse", "chain", "decode"))
        res["device_kernels_ms"] = on_dev
        res["device_samples_per_s"] = total_samples / (on_dev * 1e-3)
        res["device_compressed_GBps"] = total_bytes / (on_dev * 1e-3) / 1e9
        res["device_written_GBps"] = total_samples * 8 / (on_dev * 1e-3) / 1e9          # int32 PCM and fp32 mono
        res["device_written_share_of_copy_rate"] = res["device_written_GBps"] / (COPY_TBS * 1e3)
        del host_bytes, pcm, mono, work, out
        # ---- (c) end to end ----------------------------------------------------------------------------------------
        got, _ = flac.decode_files(datas[:3], out="mono", backend="device")
        assert all(torch.equal(g, want) for g in got)
        res["decode_files_device_ms"] = stats(repeat(lambda: flac.decode_files(datas, out="mono", backend="device"),
                                                     a.runs, a.warmup))
        res["decode_files_device_samples_per_s"] = total_samples / (res["decode_files_device_ms"]["median"] * 1e-3)
    res["host_16_threads_samples_per_s"] = total_samples / (res["host_16_threads_ms"]["median"] * 1e-3)
    res["host_1_thread_samples_per_s"] = total_samples / (res["host_1_thread_ms"]["median"] * 1e-3)
    res["decode_files_host_samples_per_s"] = total_samples / (res["decode_files_host_ms"]["median"] * 1e-3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
