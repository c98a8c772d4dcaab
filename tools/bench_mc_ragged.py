#!/usr/bin/env python3
"""Times the MC-dropout + PCA baseline of the inpainting validator on ragged-gap batches (csrc/mc_pca_ragged.hip, csrc/mc_pca.hip,
mc_baseline.calculate_unet_baseline_ragged) against the uniform path (mc_baseline.calculate_unet_baseline) at the C3 shape
(F = 128, T = 256: a 32704-sample clip at STFT 255/128), B = 16, 50 passes, n = 5 components:

  * uniform batch (an 18-frame gap in every item): uniform path and ragged path, alternating;
  * mixed batch (17- and 18-frame gaps, as AudioInpaintingDataset's random starts give): ragged path (the uniform path
    raises ValueError for it);
  * host synchronisations per batch of each path, counted by torch's sync debug mode (warnings raised by synchronising
    torch calls; the HIP entry points of this project never synchronise);
  * the PCA alone (compute_pca_batch / compute_pca_ragged) on the sampled stack, device events.

Wall times end in a device synchronise.  Prints one JSON line.

    python tools/bench_mc_ragged.py [--batch 16] [--mc-samples 50] [--reps 5] [--precision fp32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, ROOT)
F, T, HOP, WIN, GAP, LEN = 128, 256, 128, 255, 2048, 32704


def gap_frame_range(start):
    """frames whose 255-sample window touches [start, start + 2048) (tests/mc_ragged_ref.py gap_frames)"""
    lo = max(0, -(-(start - WIN // 2) // HOP))
    hi = min(T - 1, (start + GAP - 1 + WIN // 2) // HOP)
    return lo, hi + 1


def frame_masks(starts):
    m = torch.ones(len(starts), T)
    for b, s in enumerate(starts):
        lo, hi = gap_frame_range(s)
        m[b, lo:hi] = 0
    return m


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def count_syncs(fn):
    """synchronising torch calls of one fn(); None where the sync debug mode is not available"""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(w.message).lower() for w in rec)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--mc-samples", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mc_ragged needs a HIP device")
    from nppc_audio.inpainting import mc_baseline as MB
    from nppc_audio.inpainting.networks.unet import RestorationWrapper, UNet, UNetConfig
    torch.manual_seed(0)
    B, K, n = a.batch, a.mc_samples, 5
    model = RestorationWrapper(UNet(UNetConfig(in_channels=1, out_channels=1, dropout=0.2, precision=a.precision))).cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 1, F, T, generator=g).cuda()
    # starts with (s - 127) % 128 in {1, 2} give 17 frames, the others 18
    uni_starts = [4000 + 128 * 7 * b + 64 for b in range(B)]
    mix_starts = [s if b % 4 else 127 + 128 * (30 + 5 * b) + 1 + b % 2 for b, s in enumerate(uni_starts)]
    masks = {}
    for name, starts in (("uniform", uni_starts), ("mixed", mix_starts)):
        m = frame_masks(starts)
        masks[name] = m[:, None, None, :].expand(B, 1, F, T).contiguous().cuda()
    frames = {k: sorted(set((v[:, 0, 0] == 0).sum(1).tolist())) for k, v in masks.items()}
    assert frames["uniform"] == [18] and frames["mixed"] == [17, 18], frames
    uniform = lambda: MB.calculate_unet_baseline(model, x, masks["uniform"], K, n)
    ragged_u = lambda: MB.calculate_unet_baseline_ragged(model, x, masks["uniform"], K, n)
    ragged_m = lambda: MB.calculate_unet_baseline_ragged(model, x, masks["mixed"], K, n)
    with torch.no_grad():
        for fn in (uniform, ragged_u, ragged_m):                              # warm-up of every shape
            fn()
        tu, tr, tm = [], [], []
        for _ in range(a.reps):                                               # alternating, same process
            tu += wall(uniform, 1)
            tr += wall(ragged_u, 1)
            tm += wall(ragged_m, 1)
        syncs = {"uniform_path": count_syncs(uniform), "ragged_path": count_syncs(ragged_m)}
        model.net.dropout_pass = 0
        stack, idx, counts = MB.mc_dropout_samples_ragged(model, x, masks["uniform"], K)
        pca_u = device_ms(lambda: MB.compute_pca_batch(stack, n), 20)
        pca_r = device_ms(lambda: MB._pca_ragged(stack, counts, n), 20)
        index_ms = device_ms(lambda: MB.gap_index(masks["mixed"]), 20)
        gather_ms = device_ms(lambda: MB.gather_gap(x, idx, out=stack[0]), 50)
        hole = masks["uniform"].reshape(B, F * T) == 0
        bool_ms = device_ms(lambda: x.reshape(B, F * T)[hole], 50)
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "bench_mc_ragged", "B": B, "F": F, "T": T, "mc_samples": K, "n_components": n, "precision": a.precision,
           "reps": a.reps, "gap_frames": frames,
           "uniform_batch_uniform_path_ms": {"median": med(tu), "min": min(tu), "max": max(tu)},
           "uniform_batch_ragged_path_ms": {"median": med(tr), "min": min(tr), "max": max(tr)},
           "mixed_batch_ragged_path_ms": {"median": med(tm), "min": min(tm), "max": max(tm)},
           "host_syncs_per_batch": syncs,
           "pca_only_device_ms": {"compute_pca_batch": pca_u, "compute_pca_ragged": pca_r},
           "gap_index_ms_incl_host_read": index_ms,
           "gather_one_pass_device_ms": {"kernel_through_idx": gather_ms, "boolean_indexing": bool_ms}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
