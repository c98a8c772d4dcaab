#!/usr/bin/env python3
"""Times the MD5 check of decoded FLAC samples (nppc_audio/flac.py, csrc/flac_md5.hip, csrc/md5_core.h; DESIGN.md section
8i) on the corpus of tools/bench_flac_decode.py: one 10 s clip of 16 kHz / 16-bit shaped noise as 2048 files, 5.7 h of
audio, every file stating the MD5 of its samples.

  (a) the nppc_flac_md5 launch alone on the decoded corpus in device memory (device-synchronised, host clock)
  (b) flac.decode_files(out="mono", backend="device") end to end (bytes in host memory -> host tensors), verify_md5 off and on
      alternated run by run, their paired difference, and HIP events around the launches of one verified call
  (c) what a user could do without it: download the int32 PCM, narrow it to 16 bits and run hashlib.md5 on a pool of 16
      threads (hashlib releases the GIL), and the same pool on nppc_flac_md5_host, which needs no narrowing
  (d) the launch alone on a batch of ONE 35 s file (LibriSpeech's longest): one lane's chain, the floor of this design
  (e) flac.decode_files(backend="host") with verify_md5 off and on (the hash runs inside the worker threads)

Medians of --runs runs after --warmup warm-ups, with min and max.

    python tools/bench_flac_md5.py [--files 2048] [--runs 20] [--warmup 5] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from bench_flac_decode import ROOT, corpus_clip, repeat, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--long-seconds", type=float, default=35.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_md5_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio import flac
    H.require_gpu()
    clip = corpus_clip(a.seconds)
    n, nf = clip.pcm.shape[1], a.files
    want = hashlib.md5(clip.pcm[0].astype("<i2").tobytes()).digest()
    data = clip.data[:26] + want + clip.data[42:]                     # the file states the MD5 of its samples
    assert flac.stream_md5(data) == want
    res = {"tool": "bench_flac_md5", "files": nf, "clip_seconds": a.seconds, "clip_samples": n, "hours": nf * a.seconds / 3600,
           "message_bytes_per_file": 2 * n, "blocks_per_file": 2 * n // 64 + 1, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    dev = torch.device("cuda")

    def launch_alone(pcm, meta, expected):
        nfl = meta.shape[0]
        d_meta = torch.from_numpy(meta).to(dev)
        d_order = torch.from_numpy(flac._md5_order(meta[:, 3], meta[:, 4], meta[:, 7])).to(dev)
        d_exp = torch.from_numpy(expected).to(dev)
        digest = torch.empty(nfl, 16, dtype=torch.uint8, device=dev)
        verdict = torch.empty(nfl, dtype=torch.int32, device=dev)
        s = H.stream()

        def run():
            H.call("nppc_flac_md5", pcm, pcm.numel(), d_meta, nfl, d_order, d_exp, None, digest, verdict, s)
            torch.cuda.synchronize()

        torch.cuda.synchronize()
        t = repeat(run, a.runs, a.warmup)
        assert verdict.cpu().tolist() == [1] * nfl
        return stats(t)

    # ---- (a) the launch alone ---------------------------------------------------------------------------------------
    pcm = torch.from_numpy(clip.pcm[0]).to(dev).repeat(nf)
    meta = np.zeros((nf, flac.META), np.int64)
    meta[:, 3], meta[:, 4], meta[:, 7], meta[:, 9] = 1, 16, n, np.arange(nf) * n
    expected = np.tile(np.frombuffer(want, np.uint8), (nf, 1))
    res["md5_launch_ms"] = stats_a = launch_alone(pcm, meta, expected)
    res["md5_launch_message_GBps"] = nf * 2 * n / (stats_a["median"] * 1e-3) / 1e9
    res["md5_launch_ns_per_block_per_lane"] = stats_a["median"] * 1e6 / (2 * n // 64 + 1)

    # ---- (c) the alternative: download and hash on the host ---------------------------------------------------------
    def hashlib_pool(ex):
        host = pcm.cpu().numpy()                                      # pageable, as decode_files' own download is
        return list(ex.map(lambda f: hashlib.md5(host[f * n:(f + 1) * n].astype("<i2").tobytes()).digest(), range(nf)))

    def core_pool(ex):
        host = pcm.cpu().numpy()
        return list(ex.map(lambda f: flac._md5_host(host[f * n:(f + 1) * n], n, 1, 16), range(nf)))

    with ThreadPoolExecutor(max_workers=16) as ex:
        assert hashlib_pool(ex) == [want] * nf and core_pool(ex) == [want] * nf
        res["download_hashlib_16_threads_ms"] = stats(repeat(lambda: hashlib_pool(ex), a.runs, a.warmup))
        res["download_md5_host_16_threads_ms"] = stats(repeat(lambda: core_pool(ex), a.runs, a.warmup))
        res["download_only_ms"] = stats(repeat(lambda: pcm.cpu(), a.runs, a.warmup))
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    del pcm

    # ---- (d) one long file ------------------------------------------------------------------------------------------
    nl = int(a.long_seconds * 16000)
    g = np.random.Generator(np.random.PCG64(35))
    long_pcm = g.integers(-32768, 32768, nl).astype(np.int32)
    meta1 = np.zeros((1, flac.META), np.int64)
    meta1[0, 3], meta1[0, 4], meta1[0, 7] = 1, 16, nl
    exp1 = np.frombuffer(hashlib.md5(long_pcm.astype("<i2").tobytes()).digest(), np.uint8).reshape(1, 16).copy()
    res["long_file_seconds"] = a.long_seconds
    res["md5_launch_one_long_file_ms"] = launch_alone(torch.from_numpy(long_pcm).to(dev), meta1, exp1)

    # ---- (b), (e) end to end: off and on alternated run by run, because the host-side copies of decode_files (the pageable
    # download, one clone per file) move by more from one run to the next than the check costs
    datas = [data] * nf
    mono = torch.from_numpy(clip.pcm[0].astype(np.float32) / 32768.0)
    for backend, runs, warmup in (("device", a.runs, a.warmup), ("host", max(3, a.runs // 4), 1)):
        t = {False: [], True: []}
        for i in range(warmup + runs):
            for verify in (False, True):
                t0 = time.perf_counter()
                got, _ = flac.decode_files(datas, out="mono", backend=backend, verify_md5=verify)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= warmup:
                    t[verify].append(dt)
                assert torch.equal(got[0], mono) and torch.equal(got[-1], mono)
                del got
        res[f"decode_files_{backend}_verify_off_ms"] = stats(t[False])
        res[f"decode_files_{backend}_verify_on_ms"] = stats(t[True])
        res[f"decode_files_{backend}_on_minus_off_paired_ms"] = stats([y - x for x, y in zip(t[False], t[True])])
    # the launches of one verified decode_files call, by HIP events around each (two batches under the byte budget)
    H.PROFILE = []
    flac.decode_files(datas, out="mono", backend="device", verify_md5=True)
    torch.cuda.synchronize()
    ev = {}
    for name, e0, e1 in H.PROFILE:
        if name not in ("nppc_flac_probe", "nppc_flac_work_elems"):
            ev[name] = ev.get(name, 0.0) + e0.elapsed_time(e1)
    H.PROFILE = None
    res["decode_files_device_launch_events_ms"] = ev
    bad = data[:26] + bytes([want[0] ^ 1]) + want[1:] + data[42:]
    try:
        flac.decode_files([data, bad], out="mono", backend="device", verify_md5=True)
        raise AssertionError("a wrong MD5 passed")
    except flac.FlacError as e:
        assert e.status == 9
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
