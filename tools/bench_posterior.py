#!/usr/bin/env python3
"""Times posterior sampling (nppc_audio/posterior.py, csrc/posterior.hip) at B = 8 clips of 4 s,
K = 5 directions, n_fft 512 / hop 256 (F = 257, T = 251), S in {16, 64, 256} samples per clip, from the model's outputs in
device memory to waveforms (or their statistics) in device memory:

  (fused)       posterior.sample_waveforms(samples=True): one launch
  (fused_stats) posterior.sample_waveforms(samples=False, stats=True, spec_stats=True): the launch and its two finishing
                launches; no sample is written
  (composed)    the existing ops: the B S masks by torch (broadcast multiply-adds in the rule's order), then
                ops.cirm_decompress_apply and ops.istft on [B S, F, T] planes
The composed and the fused call alternate, run by run.  Medians of --runs runs after --warmup warm-ups, with min and max; the
peak of torch.cuda.max_memory_allocated over one call of each, above what the inputs hold; the output bytes per second of
the sample-writing variants against the device copy rate README.md quotes.

    python tools/bench_posterior.py [--runs 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import time

import torch

from bench_flac_decode import COPY_TBS, ROOT, stats

B, K, NFFT, HOP, L = 8, 5, 512, 256, 64000
SAMPLES = (16, 64, 256)


def composed(pred, w, re, im, z, S):
    from nppc_audio import ops
    F, T = re.shape[1:]
    mr, mi = pred[:, None, 0].repeat(1, S, 1, 1), pred[:, None, 1].repeat(1, S, 1, 1)
    for k in range(K):
        zr, zi = z[:, :, k, 0, None, None], z[:, :, k, 1, None, None]
        a, c = w[:, None, k, 0], w[:, None, k, 1]
        mr = mr + (zr * a - zi * c)
        mi = mi + (zr * c + zi * a)
    n_re = re[:, None].expand(B, S, F, T).reshape(B * S, F, T)
    n_im = im[:, None].expand(B, S, F, T).reshape(B * S, F, T)
    _, xr, xi = ops.cirm_decompress_apply(torch.stack((mr, mi), dim=2).reshape(B * S, 2, F, T), n_re, n_im)
    return ops.istft(xr, xi, NFFT, HOP, L).view(B, S, L)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio import posterior as P
    H.require_gpu()
    F, T = NFFT // 2 + 1, 1 + L // HOP
    g = torch.Generator(device="cuda").manual_seed(3)
    pred = torch.rand(B, 2, F, T, generator=g, device="cuda") * 6 - 3
    w = torch.randn(B, K, 2, F, T, generator=g, device="cuda") * 0.5
    re, im = torch.randn(B, F, T, generator=g, device="cuda"), torch.randn(B, F, T, generator=g, device="cuda")
    res = {"tool": "bench_posterior", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "shape": dict(B=B, K=K, nfft=NFFT, hop=HOP, F=F, T=T, L=L), "copy_TBs": COPY_TBS, "S": {}}
    for S in SAMPLES:
        z = P.draw_coefficients(B, S, K, seed=S)
        fused = lambda: P.sample_waveforms(pred, w, re, im, z, L, NFFT, HOP)["samples"]
        fstat = lambda: P.sample_waveforms(pred, w, re, im, z, L, NFFT, HOP, samples=False, stats=True, spec_stats=True)
        base = lambda: composed(pred, w, re, im, z, S)
        same = bool(torch.equal(fused(), base()))
        t = {"composed": [], "fused": [], "fused_stats": []}
        for i in range(a.warmup + a.runs):
            row = (timed(base), timed(fused), timed(fstat))       # the baseline and the fused call alternate
            if i >= a.warmup:
                for k, v in zip(t, row):
                    t[k].append(v)
        out_bytes = B * S * L * 4
        r = {"ms": {k: stats(v) for k, v in t.items()}, "bit_equal_to_composed": same, "output_MB": out_bytes / 1e6,
             "plane_MB": B * S * F * T * 4 / 1e6,
             "peak_MB": {"composed": peak_mb(base), "fused": peak_mb(fused), "fused_stats": peak_mb(fstat)},
             "tiling": dict(zip(("tiles", "samples_per_tile", "work_bytes"), P.sample_tiling(B, S, K, T, NFFT, HOP, L, 3)))}
        for k in ("composed", "fused"):
            tbs = out_bytes / (r["ms"][k]["median"] * 1e-3) / 1e12
            r[f"{k}_output_TBs"] = tbs
            r[f"{k}_output_share_of_copy_rate"] = tbs / COPY_TBS
        r["composed_over_fused"] = r["ms"]["composed"]["median"] / r["ms"]["fused"]["median"]
        res["S"][str(S)] = r
        print(json.dumps({str(S): r}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
