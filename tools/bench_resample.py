#!/usr/bin/env python3
"""Times nppc_audio.resample (csrc/resample.hip), the reference's windowed-sinc resampler, on one device:

  recording  60 s of mono audio, 44.1 kHz -> 16 kHz and 16 kHz -> 44.1 kHz
  batch      a ragged batch of 2048 clips of 5 - 15 s, 44.1 kHz -> 16 kHz (--clips to change)

each with three resamplers:
  kernel     nppc_resample_sinc, the compressed table in LDS
  conv1d     the same formula as F.conv1d with the FULL bank on the same device (what torchaudio runs there); the ragged batch
             is padded to its longest clip, as torchaudio would be given it, in chunks of --conv-chunk clips to bound memory
  scipy      scipy.signal.resample_poly (fp64) on --threads host threads, including the download of the input and the upload
             of the result; on the batch it runs on the first --scipy-clips clips only and the figure is scaled to the batch

Medians of --rounds timed runs after --warmup, host clock around a device synchronise.  GB/s = (samples read + samples
written) x 4 bytes / time, against the 6.29 TB/s copy rate of tools/bench_inpaint_data.py.  Then, with --restore, one
RecordingRestorer.restore(..., sample_rate=44100) of the 60 s / 8-gap recording of tools/bench_restore_recording.py next to the
16 kHz call on the downsampled recording: the difference is the price of restoring at the recording's own rate.

    python tools/bench_resample.py [--rounds 10] [--warmup 3] [--restore] [--out FILE]
"""
import argparse
import concurrent.futures as cf
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generative-audio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
COPY_RATE = 6.29e12


def timed(fn, warmup, rounds):
    out, ms = None, []
    for i in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": [round(t, 4) for t in ms]}, out


def conv1d_resample(x, table, bank, chunk):
    """x [B, L] (device, zero past each item) -> [B, ceil(new L / orig)]: pad, conv1d with stride orig, transpose, cut"""
    outs = []
    target = -(-table.new * x.shape[1] // table.orig)
    for b0 in range(0, x.shape[0], chunk):
        xp = torch.nn.functional.pad(x[b0:b0 + chunk, None], (table.width, table.width + table.orig))
        y = torch.nn.functional.conv1d(xp, bank, stride=table.orig)
        outs.append(y.transpose(1, 2).reshape(y.shape[0], -1)[:, :target])
    return torch.cat(outs) if len(outs) > 1 else outs[0].contiguous()


def scipy_resample(x_dev, lens, orig, new, threads):
    from scipy.signal import resample_poly
    xh = x_dev.cpu().numpy()
    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        ys = list(ex.map(lambda b: resample_poly(xh[b, :lens[b]].astype(np.float64), new, orig).astype(np.float32),
                         range(len(lens))))
    out = torch.zeros(len(lens), max(y.size for y in ys))
    for b, y in enumerate(ys):
        out[b, :y.size] = torch.from_numpy(y)
    return out.cuda()


def case(name, x, lens, orig_freq, new_freq, a, scipy_items=None):
    from nppc_audio import resample as RS
    t = RS.sinc_table(orig_freq, new_freq)
    bank = RS._host_bank(t).cuda()
    B = x.shape[0]
    outs = [RS.out_length(n, orig_freq, new_freq) for n in lens]
    res = {"case": name, "orig_freq": orig_freq, "new_freq": new_freq, "items": B, "samples_in": int(sum(lens)),
           "samples_out": int(sum(outs)), "tile": t.tile, "lds_bytes": t.lds_bytes, "table_bytes": t.new * t.stride * 4,
           "full_bank_bytes": t.new * t.klen * 4}
    ragged = None if B == 1 else lens
    run = (lambda: RS.resample(x, orig_freq, new_freq, lengths=ragged, backend="hip"))
    res["kernel_ms"], yk = timed(run, a.warmup, a.rounds)
    yk = yk[0] if ragged is not None else yk
    moved = 4 * (sum(lens) + B * max(outs))                                 # read once, every column of y written
    res["kernel_gbps"] = moved / res["kernel_ms"]["median"] / 1e6
    res["kernel_share_of_copy_rate"] = res["kernel_gbps"] * 1e9 / COPY_RATE
    res["conv1d_ms"], yc = timed(lambda: conv1d_resample(x, t, bank, a.conv_chunk), min(a.warmup, 2), max(a.rounds // 2, 3))
    res["conv1d_gbps"] = moved / res["conv1d_ms"]["median"] / 1e6
    res["conv1d_over_kernel"] = res["conv1d_ms"]["median"] / res["kernel_ms"]["median"]
    worst = 0.0
    for b in range(0, B, max(B // 16, 1)):                                  # the two agree up to fp32 summation order
        worst = max(worst, float((yk[b, :outs[b]] - yc[b, :outs[b]]).abs().max()))
    res["kernel_vs_conv1d_max_abs_diff"] = worst
    n_sc = B if scipy_items is None else min(scipy_items, B)
    res["scipy_items"] = n_sc
    res["scipy_ms"], _ = timed(lambda: scipy_resample(x[:n_sc], lens[:n_sc], t.orig, t.new, a.threads), 1, 3)
    res["scipy_threads"] = a.threads
    if n_sc < B:
        res["scipy_ms_scaled_to_batch"] = res["scipy_ms"]["median"] * sum(lens) / sum(lens[:n_sc])
    return res


def restore_case(a):
    spec = importlib.util.spec_from_file_location("bench_restore_recording", os.path.join(ROOT, "tools", "bench_restore_recording.py"))
    BR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(BR)
    from nppc_audio import resample as RS
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas
    r = BR.build("bf16")
    rate = 44100
    n = rate * BR.SECONDS
    tt = np.arange(n) / rate
    rng = np.random.default_rng(0)
    x = 0.05 * (np.sin(2 * np.pi * 220 * tt) + 0.5 * np.sin(2 * np.pi * 330 * tt + 1)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * tt))
    x = (x + 0.005 * rng.standard_normal(n)).astype(np.float32)
    glen = BR.GAP * 441 // 160
    gaps = [(int((i + 0.5) * n / BR.N_GAPS), int((i + 0.5) * n / BR.N_GAPS) + glen) for i in range(BR.N_GAPS)]
    for s, e in gaps:
        x[s:e] = 0.0
    xd = torch.from_numpy(x).cuda()
    alphas = default_alphas("cuda")
    down = RS.sinc_table(rate, 16000)
    low = RS.resample(xd, rate, 16000)
    mapped = [RS.map_gap(s, e, down, out_len=low.numel()) for s, e in gaps]
    res = {"case": "restore", "seconds": BR.SECONDS, "gaps": BR.N_GAPS, "gap_samples_native": glen,
           "gap_samples_model_rate": [b - c for c, b in mapped], "alphas": int(alphas.numel())}
    runs = {"native_44100": lambda: r.restore(xd, gaps, alphas=alphas, sample_rate=rate),
            "model_rate_16000": lambda: r.restore(low, mapped, alphas=alphas)}
    times = {k: [] for k in runs}
    for rnd in range(a.warmup + a.rounds):
        for k, fn in runs.items():                                          # alternated: one of each per round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if k == "native_44100":
                keep = out["restored"]
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(t, 3) for t in v]}
    res["price_of_native_rate_ms"] = res["native_44100_ms"]["median"] - res["model_rate_16000_ms"]["median"]
    region = torch.zeros(n, dtype=torch.bool)
    for s, e in gaps:                                                       # far apart: none of them merge
        region[max(s - 177, 0):e + 177] = True
    res["known_samples_bit_equal"] = bool(torch.equal(keep.cpu()[~region], torch.from_numpy(x)[~region]))
    res["restored_finite"] = bool(torch.isfinite(keep).all())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--conv-chunk", type=int, default=256)
    ap.add_argument("--scipy-clips", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs a HIP device")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"tool": "bench_resample", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
           "copy_rate_quoted": COPY_RATE, "cases": []}
    rec = 0.1 * torch.randn(1, 44100 * 60, device="cuda", generator=g)
    res["cases"].append(case("recording_down", rec, [rec.shape[1]], 44100, 16000, a))
    rec16 = 0.1 * torch.randn(1, 16000 * 60, device="cuda", generator=g)
    res["cases"].append(case("recording_up", rec16, [rec16.shape[1]], 16000, 44100, a))
    rng = np.random.default_rng(1)
    lens = [int(v) for v in rng.integers(5 * 44100, 15 * 44100 + 1, a.clips)]
    x = 0.1 * torch.randn(a.clips, max(lens), device="cuda", generator=g)
    x *= (torch.arange(max(lens), device="cuda")[None] < torch.tensor(lens, device="cuda")[:, None])
    res["cases"].append(case("ragged_batch_down", x, lens, 44100, 16000, a, scipy_items=a.scipy_clips))
    del x
    if a.restore:
        res["cases"].append(restore_case(a))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
