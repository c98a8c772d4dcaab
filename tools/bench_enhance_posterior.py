#!/usr/bin/env python3
"""Times posterior sampling of whole recordings (enhance.sample_chunks, csrc/enhance_post.hip): a 60 s
and a 10 min recording at 16 kHz, K = 5 directions, chunks of 65536 at n_fft 512 / hop 256 (F = 257, T = 257), S = 16 and 64
samples, from the planes of the chunks and the alignment tables in device memory to recordings (or their statistics) in
device memory:

  (fused)       sample_chunks(samples=True): one launch
  (fused_stats) sample_chunks(samples=False, stats=True): the launch and its finishing launch; no sample is written
  (composed)    what was there before: w_mat gathered to slot order with torch, posterior.sample_waveforms on the chunks (an
                [n, S, C] intermediate), then one enhance.splice launch per sample row
The composed and the fused call alternate, run by run.  Medians of --runs runs after --warmup warm-ups, with min and max, and
the peak of torch.cuda.max_memory_allocated over one call of each, above what the inputs hold, and the composed path once
more stage by stage (composed_parts_ms: medians of 5, a synchronize after every stage).  The planes are random (the
nets are not part of the measurement) and the tables a random signed permutation per chunk.

    python tools/bench_enhance_posterior.py [--runs 20] [--warmup 5] [--seconds 60 600] [--out FILE]
"""
import argparse
import json
import os

import torch

from bench_flac_decode import ROOT, stats
from bench_posterior import peak_mb, timed

K, NFFT, HOP, C, RATE = 5, 512, 256, 65536, 16000
SAMPLES = (16, 64)


def composed(en, P, pred, w, re, im, z, perm, sign, last):
    n, S = pred.shape[0], z.shape[0]
    slot = w[torch.arange(n, device=w.device)[:, None], perm.long()] * sign.float()[:, :, None, None, None]
    y = P.sample_waveforms(pred, slot, re, im, z[None].expand(n, *z.shape), C, NFFT, HOP, lengths=[C] * (n - 1) + [last])["samples"]
    return torch.stack([en.splice(y[:, s], None, last, None, None, None)[0] for s in range(S)])


def composed_parts(en, P, pred, w, re, im, z, perm, sign, last, runs):
    """the composed path stage by stage (each ended by a synchronize): medians over `runs` runs, ms"""
    n, S = pred.shape[0], z.shape[0]
    t = {"gather": [], "sample_waveforms": [], "splices": [], "stack": []}
    for _ in range(runs):
        box = {}
        t["gather"].append(timed(lambda: box.update(slot=w[torch.arange(n, device=w.device)[:, None], perm.long()]
                                                    * sign.float()[:, :, None, None, None])))
        t["sample_waveforms"].append(timed(lambda: box.update(y=P.sample_waveforms(
            pred, box["slot"], re, im, z[None].expand(n, *z.shape), C, NFFT, HOP, lengths=[C] * (n - 1) + [last])["samples"])))
        t["splices"].append(timed(lambda: box.update(rows=[en.splice(box["y"][:, s], None, last, None, None, None)[0]
                                                           for s in range(S)])))
        t["stack"].append(timed(lambda: box.update(out=torch.stack(box["rows"]))))
    return {k: stats(v)["median"] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance_posterior_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio import enhance as en
    from nppc_audio import posterior as P
    H.require_gpu()
    F, T, Hh = NFFT // 2 + 1, 1 + C // HOP, C // 2
    res = {"tool": "bench_enhance_posterior", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "shape": dict(K=K, nfft=NFFT, hop=HOP, F=F, T=T, chunk_samples=C, rate=RATE), "recordings": {}}
    for sec in a.seconds:
        L = sec * RATE
        n = -(-(L - C) // Hh) + 1
        last = L - (n - 1) * Hh
        g = torch.Generator(device="cuda").manual_seed(sec)
        pred = torch.rand(n, 2, F, T, generator=g, device="cuda") * 6 - 3
        w = torch.randn(n, K, 2, F, T, generator=g, device="cuda") * 0.5
        re, im = torch.randn(n, F, T, generator=g, device="cuda"), torch.randn(n, F, T, generator=g, device="cuda")
        perm = torch.stack([torch.randperm(K, generator=g, device="cuda") for _ in range(n)]).int()
        sign = (torch.randint(0, 2, (n, K), generator=g, device="cuda") * 2 - 1).int()
        rec = {"L": L, "chunks": n, "last_chunk": last, "plane_MB": (2 * K + 4) * F * T * 4 * n / 1e6, "S": {}}
        for S in SAMPLES:
            z = P.draw_coefficients(1, S, K, seed=S)[0]
            fused = lambda: en.sample_chunks(pred, w, re, im, None, z, perm, sign, last, C, NFFT, HOP)["samples"]      # noqa: E731
            fstat = lambda: en.sample_chunks(pred, w, re, im, None, z, perm, sign, last, C, NFFT, HOP, samples=False, stats=True)  # noqa: E731
            base = lambda: composed(en, P, pred, w, re, im, z, perm, sign, last)                                      # noqa: E731
            same = bool(torch.equal(fused(), base()))
            t = {"composed": [], "fused": [], "fused_stats": []}
            for i in range(a.warmup + a.runs):
                row = (timed(base), timed(fused), timed(fstat))     # the baseline and the fused call alternate
                if i >= a.warmup:
                    for k, v in zip(t, row):
                        t[k].append(v)
            r = {"ms": {k: stats(v) for k, v in t.items()}, "bit_equal_to_composed": same, "output_MB": S * L * 4 / 1e6,
                 "intermediate_MB_composed": n * S * C * 4 / 1e6,
                 "peak_MB": {"composed": peak_mb(base), "fused": peak_mb(fused), "fused_stats": peak_mb(fstat)},
                 "tiling": dict(zip(("tiles", "samples_per_tile", "work_bytes"), en.enh_post_shape(n, S, K, C, L, T, NFFT, HOP, True)))}
            r["composed_parts_ms"] = composed_parts(en, P, pred, w, re, im, z, perm, sign, last, 5)
            r["composed_over_fused"] = r["ms"]["composed"]["median"] / r["ms"]["fused"]["median"]
            rec["S"][str(S)] = r
            print(json.dumps({f"{sec}s_S{S}": r}), flush=True)
        res["recordings"][f"{sec}s"] = rec
        del pred, w, re, im
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
