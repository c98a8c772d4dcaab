#!/usr/bin/env python3
"""Sizes and times of the FLAC encoder's predictor "lpc" against "fixed" (nppc_audio/flac.py, csrc/flac_enc.hip,
csrc/flac_enc_core.h), on the two workloads of tools/bench_flac_encode.py

  validator  1056 x 4 s      restore  66 x 60 s      (16 kHz, 16 bits, block 4096, max_lpc_order 8)

each filled twice: with that tool's resonance noise (white noise at full level through [1, -1.6, 0.8]: its entropy is the
floor, LPC has little to find) and with a voiced recipe (tests/flac_lpc_cases.voiced, vectorised: a pulse train plus a
little noise through formant resonators at 600 / 1400 / 2600 Hz; every row its own seed and its own pitch, 80..200 Hz).
Per workload and signal, from the same run:

  size     encoded bytes over raw 16-bit bytes for "fixed" and "lpc" (the device's streams; the host pool's are asserted
           equal, and the first rows are asserted byte-equal to the restatement tests/flac_lpc_ref.py)
  time     flac.encode_waves(backend="hip") for both predictors, HIP-event times per launch of one call of each,
           flac.encode_waves(backend="host") on the pool of 16 threads with "lpc" after the download, the download alone
  window   on the voiced signal, the subframes' exact bits over raw for the Welch window of the rule and for a rectangular
           one, from the restatement on the first --window-rows rows (a flag of this tool, not a mode of the library)

Medians of --runs runs after --warmup warm-ups, with min and max.  No synthetic signal is speech: nothing here was measured
on a recording.

    python tools/bench_flac_lpc.py [--runs 5] [--warmup 2] [--scale 1.0] [--window-rows 4] [--out FILE]
"""
import argparse
import json
import os

import numpy as np
import torch

from bench_flac_decode import ROOT, repeat, stats
from bench_flac_encode import RATE, speech_rows

MAX_ORDER = 8


def voiced_rows(rows, n, seed):
    """[rows, n] fp32 in (-1, 1): tests/flac_lpc_cases.voiced's recipe (peak 0.5), one seed and one pitch per row"""
    from scipy.signal import lfilter
    from flac_lpc_cases import FORMANTS
    g = np.random.default_rng(seed)
    out = np.empty((rows, n), np.float32)
    t = np.arange(n)
    for r0 in range(0, rows, 64):
        r1 = min(rows, r0 + 64)
        period = g.integers(RATE // 200, RATE // 80 + 1, r1 - r0)
        y = (t[None, :] % period[:, None] == 0).astype(np.float64) + 0.01 * g.standard_normal((r1 - r0, n))
        for f, bw in FORMANTS:
            rad = np.exp(-np.pi * bw / RATE)
            y = lfilter([1.0], [1.0, -2.0 * rad * np.cos(2.0 * np.pi * f / RATE), rad * rad], y, axis=1)
        out[r0:r1] = y / np.abs(y).max(1, keepdims=True) * 0.5
    return out


def events(fn):
    from nppc_audio import _hip as H
    H.PROFILE = []
    fn()
    torch.cuda.synchronize()
    ev = {}
    for k, e0, e1 in H.PROFILE:
        ev[k] = ev.get(k, 0.0) + e0.elapsed_time(e1)
    H.PROFILE = None
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the rows of each workload (for a quick look)")
    ap.add_argument("--window-rows", type=int, default=4, help="rows of the voiced signal the restatement plans twice")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_lpc_bench.json"))
    a = ap.parse_args()
    import flac_lpc_ref as L
    from nppc_audio import _hip as H
    from nppc_audio import flac
    H.require_gpu()
    res = {"tool": "bench_flac_lpc", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "host_cpus_used": flac.HOST_THREADS, "sample_rate": RATE, "bits_per_sample": 16, "block_size": 4096,
           "max_lpc_order": MAX_ORDER}
    for name, rows, seconds in (("validator_1056x4s", 1056, 4.0), ("restore_66x60s", 66, 60.0)):
        rows, n = max(1, int(rows * a.scale)), int(seconds * RATE)
        for signal, fill in (("resonance_noise", speech_rows), ("voiced", voiced_rows)):
            host_waves = fill(rows, n, 1234)
            waves = torch.from_numpy(host_waves).cuda()
            torch.cuda.synchronize()
            raw = rows * n * 2
            out = {"rows": rows, "samples_per_row": n, "raw_16bit_MB": raw / 1e6}
            got = {}

            def device(predictor):
                got[predictor] = flac.encode_waves(waves, None, RATE, 16, backend="hip", predictor=predictor, max_lpc_order=MAX_ORDER)

            def host_pool():
                got["host"] = flac.encode_waves(waves.cpu(), None, RATE, 16, backend="host", predictor="lpc", max_lpc_order=MAX_ORDER)

            for p in ("fixed", "lpc"):
                out[f"device_encode_waves_{p}_ms"] = stats(repeat(lambda: device(p), a.runs, a.warmup))
                out[f"device_launch_events_{p}_ms"] = events(lambda: device(p))
                out[f"{p}_over_raw"] = sum(map(len, got[p])) / raw
            assert all(len(x) <= len(y) for x, y in zip(got["lpc"], got["fixed"])), "an LPC stream is longer than the fixed one"
            out["download_fp32_then_host_pool_lpc_ms"] = stats(repeat(host_pool, max(1, a.runs // 2), 1))
            assert got["host"] == got["lpc"], "host and device streams differ"
            out["download_fp32_only_ms"] = stats(repeat(lambda: waves.cpu(), a.runs, a.warmup))
            back, _ = flac.decode_files(got["lpc"][:4], out="pcm", backend="device", verify_md5=True)
            q = flac.quantize_waves_host(host_waves[:4], 16)
            assert all(np.array_equal(b.numpy()[0], q[i]) for i, b in enumerate(back))
            # the restatement on the same rows: the device's bytes are its bytes, or there is a bug
            k = min(rows, 2 if n <= 64000 else 1)
            m = min(n, 4 * 4096 + 100)                                # the restatement is Python: the head of a long row
            head = flac.encode_waves(waves[:k, :m].contiguous(), None, RATE, 16, backend="hip", predictor="lpc", max_lpc_order=MAX_ORDER)
            qh = flac.quantize_waves_host(host_waves[:k, :m], 16)
            assert head == [L.encode(qh[i:i + 1], 16, RATE, 4096, MAX_ORDER) for i in range(k)], "device and restatement differ"
            out["rows_compared_with_restatement"] = k
            if signal == "voiced":
                w = min(rows, a.window_rows)
                qw = flac.quantize_waves_host(host_waves[:w, :min(n, 64000)], 16)
                bits = {key: sum(L.subframe_bits(qw[i:i + 1], 16, 4096, MAX_ORDER, rectangular=rect) for i in range(w))
                        for key, rect in (("welch", False), ("rectangular", True))}
                out["window_rows"] = w
                out["window_subframe_bits_over_raw"] = {key: v / (qw.size * 16) for key, v in bits.items()}
            res[f"{name}/{signal}"] = out
            print(name, signal, json.dumps(out), flush=True)
            del waves
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
