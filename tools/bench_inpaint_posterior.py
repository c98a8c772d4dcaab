#!/usr/bin/env python3
"""Times posterior sampling of inpainted gaps (nppc_audio/inpainting/posterior.py, csrc/inpaint_posterior.hip and the third
magnitude source of csrc/gl_gap_common.h) at the validator's shape: B = 16 clips of 4 s at n_fft 255 /
hop 128 (F = 128, T = 501, L = 64001), K = 5 directions, a 17-frame gap, S in {16, 64, 256} samples per clip, from the
model's outputs in device memory to waveforms in device memory.

Clean phase
  (fused)          posterior.sample_waveforms: one launch, the K + 1 planes and the unit phasors of a workgroup staged in LDS
  (fused_no_stage) the same launch with the staging switched off (no_stage=True): planes re-read, phasor recomputed per sample
  (fused_stats)    samples=False, stats=True, spec_stats=True: nothing of size S is written
  (composed)       what existed before: the [B, S, F, T] magnitudes and the phasor by torch operators (fp32), then
                   ops.istft_any on [B S, F, T] planes
Blind (32 iterations of gap-constrained Griffin-Lim)
  (gl_post)        posterior.sample_waveforms_blind: the magnitudes formed where the iteration starts
  (gl_stack)       phase.griffin_lim_gap fed a [B, S + 1, F, T] magnitude stack formed by torch
The candidates of a group alternate, run by run.  Medians of --runs runs after --warmup warm-ups, with min and max; the peak
of torch.cuda.max_memory_allocated over one call of each, above what the inputs hold; output bytes per second against the
device copy rate README.md quotes.

    python tools/bench_inpaint_posterior.py [--runs 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os

import torch

from bench_flac_decode import COPY_TBS, ROOT, stats
from bench_posterior import peak_mb, timed

B, K, NFFT, HOP, T, GAP = 16, 5, 255, 128, 501, 17
F, L = NFFT // 2 + 1, HOP * (T - 1) + 1
SAMPLES = (16, 64, 256)


def magnitudes(pred, pc, z, mean, std):
    """[B, S, F, T] by torch, fp32, k ascending"""
    x = pred.expand(B, z.shape[1], F, T).clone()
    for k in range(K):
        x = x + z[:, :, k, None, None] * pc[:, k, None]
    return torch.exp(x * std + mean)


def composed(pred, pc, clean, z, mean, std):
    from nppc_audio import ops
    S = z.shape[1]
    mag = magnitudes(pred, pc, z, mean, std)
    h = torch.sqrt(clean[:, 0] ** 2 + clean[:, 1] ** 2)
    ur = torch.where(h > 0, clean[:, 0] / h, torch.ones_like(h))
    ui = torch.where(h > 0, clean[:, 1] / h, torch.zeros_like(h))
    re, im = (mag * ur[:, None]).reshape(B * S, F, T), (mag * ui[:, None]).reshape(B * S, F, T)
    return ops.istft_any(re, im, NFFT, HOP).view(B, S, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_posterior_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import phase as PH
    from nppc_audio.inpainting import posterior as P
    H.require_gpu()
    g = torch.Generator(device="cuda").manual_seed(3)
    mask = torch.ones(B, T, device="cuda")
    for b in range(B):
        mask[b, 100 + 20 * b:100 + 20 * b + GAP] = 0
    pred = torch.rand(B, 1, F, T, generator=g, device="cuda") * 4 - 2
    pc = (torch.rand(B, K, F, T, generator=g, device="cuda") * 1.2 - 0.6) * (1 - mask)[:, None, None, :]
    clean = torch.randn(B, 2, F, T, generator=g, device="cuda")
    known = clean * mask[:, None, None, :]
    mean, std = torch.tensor(-1.0, device="cuda"), torch.tensor(2.5, device="cuda")
    ph0 = PH.phase_advance_init(known, mask, NFFT, HOP)
    res = {"tool": "bench_inpaint_posterior", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "shape": dict(B=B, K=K, nfft=NFFT, hop=HOP, F=F, T=T, L=L, gap_frames=GAP, gl_iters=32), "copy_TBs": COPY_TBS, "S": {}}
    for S in SAMPLES:
        z = P.draw_coefficients(B, S, K, seed=S) / K
        clean_calls = {
            "composed": lambda: composed(pred, pc, clean, z, mean, std),
            "fused": lambda: P.sample_waveforms(pred, pc, clean, z, mean, std)["samples"],
            "fused_no_stage": lambda: P.sample_waveforms(pred, pc, clean, z, mean, std, no_stage=True)["samples"],
            "fused_stats": lambda: P.sample_waveforms(pred, pc, clean, z, mean, std, samples=False, stats=True, spec_stats=True),
        }
        zz = torch.cat([z, torch.zeros(B, 1, K, device="cuda")], 1)
        blind_calls = {
            "gl_stack": lambda: PH.griffin_lim_gap(magnitudes(pred, pc, zz, mean, std), known, mask, n_iter=32, init_phase=ph0)[0],
            "gl_post": lambda: P.sample_waveforms_blind(pred, pc, known, mask, z, mean, std, n_iter=32, init_phase=ph0)[0],
        }
        ref, got = clean_calls["composed"](), clean_calls["fused"]()
        r = {"fused_bit_equal_to_no_stage": bool(torch.equal(got, clean_calls["fused_no_stage"]())),
             "fused_vs_composed_max_rel": float((got - ref).abs().max() / ref.abs().max()),
             "shape_query": P.sample_shape(B, S, K, T), "shape_query_stats": P.sample_shape(B, S, K, T, stats=3),
             "output_MB": B * S * L * 4 / 1e6, "magnitude_stack_MB": B * S * F * T * 4 / 1e6, "ms": {}, "peak_MB": {}}
        del ref, got
        for calls in (clean_calls, blind_calls):
            t = {k: [] for k in calls}
            for i in range(a.warmup + a.runs):
                row = [timed(fn) for fn in calls.values()]          # the candidates alternate
                if i >= a.warmup:
                    for k, v in zip(t, row):
                        t[k].append(v)
            r["ms"].update({k: stats(v) for k, v in t.items()})
            r["peak_MB"].update({k: peak_mb(fn) for k, fn in calls.items()})
        for k in ("composed", "fused", "fused_no_stage", "gl_stack", "gl_post"):
            tbs = B * S * L * 4 / (r["ms"][k]["median"] * 1e-3) / 1e12
            r[f"{k}_output_TBs"] = tbs
            r[f"{k}_output_share_of_copy_rate"] = tbs / COPY_TBS
        med = lambda k: r["ms"][k]["median"]
        r["composed_over_fused"] = med("composed") / med("fused")
        r["no_stage_over_fused"] = med("fused_no_stage") / med("fused")
        r["gl_stack_over_gl_post"] = med("gl_stack") / med("gl_post")
        res["S"][str(S)] = r
        print(json.dumps({str(S): r}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
