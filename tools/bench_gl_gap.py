#!/usr/bin/env python3
"""Times gap-constrained Griffin-Lim (nppc_audio.inpainting.phase.griffin_lim_gap, csrc/gl_gap.hip) on the workload of the
inpainting validator: 16 items x 66 variations, T = 256 frames at n_fft 255 / hop 128, a 17-frame gap, 32 iterations.

Nothing in the project did this job before, so the comparison is what a user could write without the kernel: the same loop
with torch.stft / torch.istft on the device over whole clips.  Both run in the same process, alternated round by round after
a warm-up; every round is timed with device events around the whole call; the medians and the spread are reported.

    python tools/bench_gl_gap.py [--rounds 7] [--warmup 2] [--momentum 0.0] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generative-audio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_loop(tm, known, mask, phase, n_iter, mu, n_fft, hop, L):
    """the restatement of tests/gl_gap_ref.py batched on the device in fp32, whole clips"""
    B, V, F, T = tm.shape
    w = torch.hann_window(n_fft, periodic=True, device=tm.device)
    gap = (mask == 0)[:, None, None, :]
    Kn = torch.complex(known[:, 0], known[:, 1])[:, None].expand(B, V, F, T)
    M = torch.where(gap, tm, torch.zeros((), device=tm.device))
    C = torch.where(gap, torch.polar(M, torch.where(gap, phase, torch.zeros((), device=tm.device))), Kn)
    prev = torch.zeros_like(C)
    ist = lambda c: torch.istft(c.reshape(B * V, F, T), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=L)
    for _ in range(n_iter):
        x = ist(C)
        R = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                       return_complex=True).reshape(B, V, F, T)
        A = R - (mu / (1.0 + mu)) * prev
        A = A / (A.abs() + 1e-16)
        prev = R
        C = torch.where(gap, M * A, Kn)
    return ist(C).reshape(B, V, L)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--variations", type=int, default=66)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--gap", type=int, default=17)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-torch", action="store_true", help="kernel only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gl_gap needs a HIP device")
    from nppc_audio.inpainting import phase as PH
    n_fft, hop = 255, 128
    B, V, T, F = a.items, a.variations, a.frames, n_fft // 2 + 1
    L = hop * (T - 1) + 1
    g = torch.Generator().manual_seed(0)
    wave = torch.randn(B, L, generator=g) * 0.1
    S = torch.stft(wave, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft), center=True,
                   pad_mode="reflect", return_complex=True)
    mask = torch.ones(B, T)
    for b in range(B):
        s = 20 + 11 * b
        mask[b, s:s + a.gap] = 0
    known = (torch.stack([S.real, S.imag], 1) * mask[:, None, None, :]).cuda()
    tm = (S.abs()[:, None] * (1 + 0.2 * (2 * torch.rand(B, V, F, T, generator=g) - 1))).cuda().contiguous()
    ph = ((2 * torch.rand(B, V, F, T, generator=g) - 1) * math.pi).cuda().contiguous()
    mask = mask.cuda()
    span = a.gap + 2 * (-(-n_fft // hop) - 1)
    runs = {"kernel_default_cap": lambda: PH.griffin_lim_gap(tm, known, mask, a.iters, a.momentum, ph)[0],
            "kernel_max_span": lambda: PH.griffin_lim_gap(tm, known, mask, a.iters, a.momentum, ph, max_span=span)[0]}
    if not a.skip_torch:
        runs["torch_stft_istft_loop"] = lambda: torch_loop(tm, known, mask, ph, a.iters, a.momentum, n_fft, hop, L)
    times = {k: [] for k in runs}
    outs = {}
    for rnd in range(a.warmup + a.rounds):
        for k, fn in runs.items():                                       # alternated: one of each per round
            ms, outs[k] = timed(fn)
            if rnd >= a.warmup:
                times[k].append(ms)
    res = {"tool": "bench_gl_gap", "items": B, "variations": V, "frames": T, "gap_frames": a.gap, "iterations": a.iters,
           "momentum": a.momentum, "n_fft": n_fft, "hop": hop, "rounds": a.rounds, "warmup": a.warmup, "max_span": span,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 4) for x in v]}
    if "torch_stft_istft_loop" in outs:
        ref = outs["torch_stft_istft_loop"].double()
        for k in ("kernel_default_cap", "kernel_max_span"):
            res[k + "_rel_l2_vs_torch_loop"] = float(torch.linalg.norm(outs[k].double() - ref) / torch.linalg.norm(ref))
        res["speedup_max_span"] = res["torch_stft_istft_loop_ms"]["median"] / res["kernel_max_span_ms"]["median"]
        res["speedup_default_cap"] = res["torch_stft_istft_loop_ms"]["median"] / res["kernel_default_cap_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
