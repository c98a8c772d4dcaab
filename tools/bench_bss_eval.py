#!/usr/bin/env python3
"""BSS-eval SDR on the device (nppc_audio.metrics.sdr): the (clean, enhanced) pairs of a validation set in one ragged
batch, the shape tools/bench_metrics.py uses.

Default work: 150 clips of 3 - 10 s at 16 kHz (lengths drawn with a fixed seed, the longest is exactly --seconds), filter
length 512.  Clips are data.synth_clip; the "enhanced" signal is the clean one plus a tenth of the noise.  Prints ONE JSON
line: device-event time of the whole launch sequence (median of --iters after a warm-up), clips/s, the split over the
entry points (device events around every launch of one extra pass: nppc_bss_corr, nppc_bss_solve, nppc_bss_project, the
last with its finishing kernel), and with --cpu-oracle N the host time of the fp64 numpy restatement
(tests/bss_eval_ref.py) on the first N clips, extrapolated to all of them, for orientation only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SR = 16000


def clips(B, L, min_seconds):
    from nppc_audio.data import synth_clip
    rng = np.random.default_rng(0)
    lens = rng.integers(min(int(min_seconds * SR), L), L + 1, size=B)
    lens[0] = L
    clean, enhanced = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for b in range(B):
        n = int(lens[b])
        y, c = synth_clip(b, n)
        clean[b, :n] = c
        enhanced[b, :n] = c + 0.1 * (y - c)
    return clean, enhanced, lens.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--min-seconds", type=float, default=3.0)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-oracle", type=int, default=0, help="also time the fp64 numpy restatement on this many clips")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bss_eval needs a HIP device")
    from nppc_audio import _hip as H
    from nppc_audio import metrics as M
    B, L, P = a.clips, int(round(a.seconds * SR)), a.filter_length
    clean, enhanced, lens = clips(B, L, a.min_seconds)
    c, e, n = torch.from_numpy(clean).cuda(), torch.from_numpy(enhanced).cuda(), torch.from_numpy(lens).cuda()
    for _ in range(a.warmup):
        M.sdr(c, e, lengths=n, filter_length=P)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = M.sdr(c, e, lengths=n, filter_length=P)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    H.PROFILE = []
    M.sdr(c, e, lengths=n, filter_length=P)
    torch.cuda.synchronize()
    split = {name: round(t0.elapsed_time(t1), 3) for name, t0, t1 in H.PROFILE}
    H.PROFILE = None
    ms = float(np.median(times))
    fma = float(np.sum(2.0 * lens * P + (lens + P - 1.0) * P))
    res = {"tool": "bench_bss_eval", "clips": B, "seconds": a.seconds, "min_seconds": a.min_seconds, "filter_length": P,
           "samples": int(lens.sum()), "iters": a.iters, "ms": round(ms, 3), "ms_min": round(min(times), 3),
           "ms_max": round(max(times), 3), "clips_per_s": round(B / (ms / 1e3), 1), "kernel_ms": split,
           "fp64_gfma": round(fma / 1e9, 2), "fp64_tflops": round(2 * fma / (ms / 1e3) / 1e12, 2),
           "mean_sdr_db": float(out.mean()), "finite": bool(torch.isfinite(out).all())}
    if a.cpu_oracle > 0:
        import bss_eval_ref as R
        k = min(a.cpu_oracle, B)
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        want = [R.sdr(clean[b, :lens[b]], enhanced[b, :lens[b]], P) for b in range(k)]
        host = time.perf_counter() - t0
        res["cpu_oracle_clips"] = k
        res["cpu_oracle_ms_per_clip"] = round(1e3 * host / k, 1)
        res["cpu_oracle_ms_all_clips"] = round(1e3 * host / float(lens[:k].sum()) * float(lens.sum()), 0)
        res["cpu_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        res["sdr_abs_diff_vs_oracle_db"] = float(np.abs(got[:k] - np.asarray(want)).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
