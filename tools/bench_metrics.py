#!/usr/bin/env python3
"""Speech-enhancement metrics on the device (nppc_audio.metrics): STOI + both SI-SDRs of the (clean, noisy) and the
(clean, enhanced) pairs of a validation set, the work of one validation epoch's scoring.

Default work: 150 clips x 10 s at 16 kHz (the size of the DNS synthetic no_reverb test set).  Clips are data.synth_clip
with inserted silent stretches; the "enhanced" signal is the clean one plus a little noise (the metrics' cost does not
depend on the model).  Prints ONE JSON line: device-event time of the whole metric launch sequence after a warm-up,
clips/s, and with --cpu-oracle N the host time of the fp64 numpy oracle (tests/se_metrics_ref.py) on N clips.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool, not from here.
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


def clips(B, L):
    from nppc_audio.data import synth_clip
    noisy, clean = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for b in range(B):
        y, c = synth_clip(b, L)
        rng = np.random.default_rng(b)
        for _ in range(3):                                # silent stretches of 0.2 - 0.8 s
            m = int(rng.integers(3200, 12800))
            a = int(rng.integers(0, L - m))
            y[a:a + m] -= c[a:a + m]
            c[a:a + m] = 0.0
        noisy[b], clean[b] = y, c
    enhanced = clean + 0.1 * (noisy - clean)
    return noisy, clean, enhanced.astype(np.float32)


def score(clean, noisy, enhanced):
    from nppc_audio import metrics as M
    return (M.stoi(clean, noisy), M.stoi(clean, enhanced), M.si_sdr_both(clean, noisy), M.si_sdr_both(clean, enhanced))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-oracle", type=int, default=0, help="also time the fp64 numpy oracle on this many clips")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a HIP device")
    B, L = a.clips, int(round(a.seconds * SR))
    noisy, clean, enhanced = clips(B, L)
    c, n, e = (torch.from_numpy(x).cuda() for x in (clean, noisy, enhanced))
    for _ in range(a.warmup):
        score(c, n, e)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = score(c, n, e)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    res = {"tool": "bench_metrics", "clips": B, "seconds": a.seconds, "iters": a.iters,
           "ms": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
           "clips_per_s": round(B / (ms / 1e3), 1),
           "mean_stoi_noisy": float(out[0].mean()), "mean_stoi_enhanced": float(out[1].mean()),
           "mean_si_sdr_noisy": float(out[2][:, 0].mean()), "mean_si_sdr_enhanced": float(out[3][:, 0].mean())}
    if a.cpu_oracle > 0:
        import se_metrics_ref as R
        k = min(a.cpu_oracle, B)
        t0 = time.perf_counter()
        for b in range(k):
            for est in (noisy[b], enhanced[b]):
                R.stoi(clean[b], est)
                R.si_sdr(clean[b], est)
                R.si_sdr_zero_mean(clean[b], est)
        host = time.perf_counter() - t0
        res["cpu_oracle_clips"] = k
        res["cpu_oracle_ms_per_clip"] = round(1e3 * host / k, 2)
        res["gpu_ms_per_clip"] = round(ms / B, 4)
        res["speedup_vs_cpu_oracle"] = round((host / k) / (ms / 1e3 / B), 1)
        res["stoi_enhanced_abs_diff_vs_oracle_clip0"] = abs(float(out[1][0]) - R.stoi(clean[0], enhanced[0]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
