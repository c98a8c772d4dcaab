#!/usr/bin/env python3
"""Times FLAC encoding (nppc_audio/flac.py, csrc/flac_enc.hip, csrc/flac_enc_core.h) from fp32
waveforms in device memory to bytes in host memory, on the two places that produce audio:

  validator  1056 x 4 s   what validate_batch(..., alphas=) synthesises for a batch (tools/bench_inpaint_validator.py)
  restore    66 x 60 s    what RecordingRestorer.restore(..., variations="full") splices (tools/bench_restore_recording.py)

both at 16 kHz, 16 bits, filled with the synthetic speech of the FLAC benchmarks (noise through a two-pole resonance under a
3 Hz envelope, tests/flac_cases.speech's recipe, vectorised; every row its own seed).  Per workload:

  (a) flac.encode_waves(backend="hip"): quantise, plan, scan, MD5, write, one small read, one copy of the encoded bytes
  (b) HIP events around the launches of one such call
  (c) what there was before: download the fp32 waveforms (pageable) and
        - encode them with the serial host encoder on a pool of 16 threads (flac.encode_waves(backend="host")), or
        - quantise them and write 16-bit wav with scipy (into memory: no disk in any of the timings)
  (d) the download alone, and the encoded size over the raw 16-bit size

Medians of --runs runs after --warmup warm-ups, with min and max.

    python tools/bench_flac_encode.py [--runs 5] [--warmup 2] [--out FILE]
"""
import argparse
import io
import json
import os

import numpy as np
import torch

from bench_flac_decode import ROOT, repeat, stats

RATE = 16000


def speech_rows(rows, n, seed):
    """[rows, n] fp32 in (-1, 1): tests/flac_cases.speech's recipe (peak 20000 / 32768), one seed per row"""
    from scipy.signal import lfilter
    g = np.random.default_rng(seed)
    env = (0.2 + np.abs(np.sin(np.arange(n) * 2 * np.pi * 3 / RATE))).astype(np.float32)
    out = np.empty((rows, n), np.float32)
    for r in range(rows):
        x = lfilter([1.0], [1.0, -1.6, 0.8], g.standard_normal(n).astype(np.float32) * env)
        out[r] = x / np.abs(x).max() * (20000.0 / 32768.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the rows of each workload (for a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_encode_bench.json"))
    a = ap.parse_args()
    from scipy.io import wavfile
    from nppc_audio import _hip as H
    from nppc_audio import flac
    H.require_gpu()
    res = {"tool": "bench_flac_encode", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "host_cpus_used": flac.HOST_THREADS, "sample_rate": RATE, "bits_per_sample": 16, "block_size": 4096}
    for name, rows, seconds in (("validator_1056x4s", 1056, 4.0), ("restore_66x60s", 66, 60.0)):
        rows, n = max(1, int(rows * a.scale)), int(seconds * RATE)
        waves = torch.from_numpy(speech_rows(rows, n, 1234)).cuda()
        torch.cuda.synchronize()
        out = {"rows": rows, "samples_per_row": n, "raw_16bit_MB": rows * n * 2 / 1e6, "fp32_MB": rows * n * 4 / 1e6}
        streams = []

        def device():
            streams[:] = flac.encode_waves(waves, None, RATE, 16, backend="hip")

        def host_pool():
            streams[:] = flac.encode_waves(waves.cpu(), None, RATE, 16, backend="host")

        def wav_scipy():
            pcm = flac.quantize_waves_host(waves.cpu().numpy(), 16).astype(np.int16)
            blobs = []
            for r in range(rows):
                b = io.BytesIO()
                wavfile.write(b, RATE, pcm[r])
                blobs.append(b.getvalue())
            return blobs

        def download():
            waves.cpu()

        out["device_encode_waves_ms"] = stats(repeat(device, a.runs, a.warmup))
        dev_streams = list(streams)
        out["flac_MB"] = sum(map(len, dev_streams)) / 1e6
        out["flac_over_raw"] = sum(map(len, dev_streams)) / (rows * n * 2)
        H.PROFILE = []
        device()
        torch.cuda.synchronize()
        ev = {}
        for k, e0, e1 in H.PROFILE:
            ev[k] = ev.get(k, 0.0) + e0.elapsed_time(e1)
        H.PROFILE = None
        out["device_launch_events_ms"] = ev
        out["download_fp32_then_host_pool_ms"] = stats(repeat(host_pool, a.runs, a.warmup))
        assert streams == dev_streams, "host and device streams differ"
        out["download_fp32_then_scipy_wav_ms"] = stats(repeat(wav_scipy, a.runs, a.warmup))
        out["download_fp32_only_ms"] = stats(repeat(download, a.runs, a.warmup))
        back, _ = flac.decode_files(dev_streams[:4], out="pcm", backend="device", verify_md5=True)
        assert all(np.array_equal(b.numpy()[0], flac.quantize_waves_host(waves[i].cpu().numpy(), 16)) for i, b in enumerate(back))
        res[name] = out
        print(name, json.dumps(out), flush=True)
        del waves
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
