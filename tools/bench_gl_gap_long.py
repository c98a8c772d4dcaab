#!/usr/bin/env python3
"""Times the tiled long-span path of gap-constrained Griffin-Lim (griffin_lim_gap(..., long_spans=...), csrc/gl_gap_long.hip,
DESIGN.md section 8g) on the validator's workload: 16 items x 66 variations, T = 256 frames at n_fft 255 / hop 128, 32
iterations.

  (a) a 33-frame gap (the reference yaml's 0.256 s), which only the tiled path takes, against the same loop written with
      torch.stft / torch.istft on the device over whole clips (tools/bench_gl_gap.py's baseline);
  (b) the 17-frame gap of tools/bench_gl_gap.py through the tiled path ("always") against the resident kernel (the default
      call): what long_spans costs when nothing is long.

All runs of a part share one process and are alternated round by round; a round is timed with the host clock around a
device synchronise; medians of --rounds rounds after --warmup warm-up rounds.

    python tools/bench_gl_gap_long.py [--rounds 20] [--warmup 5] [--momentum 0.0] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generative-audio_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_gl_gap import torch_loop  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def inputs(B, V, T, gap, n_fft, hop):
    F, L = n_fft // 2 + 1, hop * (T - 1) + 1
    g = torch.Generator().manual_seed(0)
    wave = torch.randn(B, L, generator=g) * 0.1
    S = torch.stft(wave, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft), center=True,
                   pad_mode="reflect", return_complex=True)
    mask = torch.ones(B, T)
    for b in range(B):
        s = 20 + 11 * b
        mask[b, s:s + gap] = 0
    known = (torch.stack([S.real, S.imag], 1) * mask[:, None, None, :]).cuda()
    tm = (S.abs()[:, None] * (1 + 0.2 * (2 * torch.rand(B, V, F, T, generator=g) - 1))).cuda().contiguous()
    ph = ((2 * torch.rand(B, V, F, T, generator=g) - 1) * math.pi).cuda().contiguous()
    return tm, known, mask.cuda(), ph, L


def alternate(runs, rounds, warmup):
    times, outs = {k: [] for k in runs}, {}
    for rnd in range(warmup + rounds):
        for k, fn in runs.items():                                       # alternated: one of each per round
            ms, outs[k] = timed(fn)
            if rnd >= warmup:
                times[k].append(ms)
    stats = {k + "_ms": {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 4) for x in v]}
             for k, v in times.items()}
    return stats, outs


def rel_l2(a, b):
    return float(torch.linalg.norm(a.double() - b.double()) / torch.linalg.norm(b.double()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--variations", type=int, default=66)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--long-gap", type=int, default=33)
    ap.add_argument("--short-gap", type=int, default=17)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="kernels only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gl_gap_long needs a HIP device")
    from nppc_audio.inpainting import phase as PH
    n_fft, hop = 255, 128
    B, V, T = a.items, a.variations, a.frames
    r = -(-n_fft // hop) - 1
    res = {"tool": "bench_gl_gap_long", "items": B, "variations": V, "frames": T, "iterations": a.iters, "momentum": a.momentum,
           "n_fft": n_fft, "hop": hop, "rounds": a.rounds, "warmup": a.warmup, "timer": "host clock around a device synchronise",
           "device": torch.cuda.get_device_name(0)}
    gl = lambda z, **kw: PH.griffin_lim_gap(z[0], z[1], z[2], a.iters, a.momentum, z[3], **kw)

    # (a) the 33-frame gap
    z = inputs(B, V, T, a.long_gap, n_fft, hop)
    span = a.long_gap + 2 * r
    _, info = gl(z)
    assert info["status"].cpu().tolist() == [1] * B, "the long gap is meant to be over the resident cap"
    runs = {"tiled_sized_by_clip": lambda: gl(z, long_spans=True)[0],
            "tiled_long_max_span": lambda: gl(z, long_spans=True, long_max_span=span)[0]}
    if not a.skip_torch:
        runs["torch_stft_istft_loop"] = lambda: torch_loop(z[0], z[1], z[2], z[3], a.iters, a.momentum, n_fft, hop, z[4])
    stats, outs = alternate(runs, a.rounds, a.warmup)
    part = {"gap_frames": a.long_gap, "long_max_span": span, **stats,
            "work_bytes_sized_by_clip": PH.gl_gap_shape(B, V, n_fft // 2 + 1, T, n_iter=a.iters, momentum=a.momentum,
                                                        long_spans=True)["work_bytes"],
            "work_bytes_long_max_span": PH.gl_gap_shape(B, V, n_fft // 2 + 1, T, n_iter=a.iters, momentum=a.momentum,
                                                        long_spans=True, long_max_span=span)["work_bytes"],
            "tiled_runs_bit_equal": bool(torch.equal(outs["tiled_sized_by_clip"], outs["tiled_long_max_span"]))}
    if "torch_stft_istft_loop" in outs:
        for k in ("tiled_sized_by_clip", "tiled_long_max_span"):
            part[k + "_rel_l2_vs_torch_loop"] = rel_l2(outs[k], outs["torch_stft_istft_loop"])
            part["speedup_" + k] = stats["torch_stft_istft_loop_ms"]["median"] / stats[k + "_ms"]["median"]
    res["a_long_gap_vs_torch_loop"] = part
    del outs

    # (b) the 17-frame gap: tiled against resident
    z = inputs(B, V, T, a.short_gap, n_fft, hop)
    span = a.short_gap + 2 * r
    runs = {"resident_default_cap": lambda: gl(z)[0],
            "resident_max_span": lambda: gl(z, max_span=span)[0],
            "routed_nothing_long": lambda: gl(z, long_spans=True)[0],
            "tiled_always_sized_by_clip": lambda: gl(z, long_spans="always")[0],
            "tiled_always_long_max_span": lambda: gl(z, long_spans="always", long_max_span=span)[0]}
    stats, outs = alternate(runs, a.rounds, a.warmup)
    part = {"gap_frames": a.short_gap, "max_span": span, **stats,
            "all_bit_equal": all(bool(torch.equal(outs["resident_default_cap"], o)) for o in outs.values())}
    for k in ("routed_nothing_long", "tiled_always_sized_by_clip", "tiled_always_long_max_span"):
        part[k + "_over_resident_default_cap"] = stats[k + "_ms"]["median"] / stats["resident_default_cap_ms"]["median"]
        part[k + "_over_resident_max_span"] = stats[k + "_ms"]["median"] / stats["resident_max_span_ms"]["median"]
    res["b_tiled_vs_resident"] = part

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
