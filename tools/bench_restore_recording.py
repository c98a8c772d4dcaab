#!/usr/bin/env python3
"""Times RecordingRestorer.restore (nppc_audio/inpainting/restore.py, csrc/restore_rec.hip) on a whole recording: 60 s of
synthetic 16 kHz audio with 8 gaps of 2048 samples, alphas = default_alphas() (K = 5 directions x 13 alphas + the
prediction = 66 waveforms per window), windows of 32704 samples, 32 Griffin-Lim iterations.

Beside it runs the same pipeline with the gain, the gather and the splice written with torch indexing on the device (what a
user could write without the three kernels); everything between them (frame mask, STFT, preprocess_data, the nets,
pc_audio_variations_blind) is the same code in both.  The two are alternated round by round after a warm-up; each round is
timed with the host clock around a device synchronise.  A further pass with device events around the launches of the three
new kernels gives their share of the call.  Weights are the oracle's seeded draw: the timing does not depend on them.

    python tools/bench_restore_recording.py [--rounds 20] [--warmup 5] [--variations windows|full] [--out FILE]
"""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generative-audio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
SR, SECONDS, N_GAPS, GAP, K_DIRS = 16000, 60, 8, 2048, 5
NEW_KERNELS = ("nppc_rec_gain", "nppc_rec_windows", "nppc_rec_splice")


def build(precision, **cfg):
    from nppc_audio.inpainting import restore as RS
    from oracle import weights as W
    tmp = tempfile.mkdtemp(prefix="nppc_bench_restore_")
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(K_DIRS), 41).items()}
    pre = "pretrained_restoration_model.net."
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, os.path.join(tmp, "r.pt"))
    torch.save({"model_state_dict": wts}, os.path.join(tmp, "nppc.pt"))
    mc = dict(pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision=precision),
              pretrained_restoration_model_path=os.path.join(tmp, "r.pt"),
              audio_pc_wrapper_configuration=dict(n_dirs=K_DIRS, model_configuration=dict(in_channels=2, out_channels=K_DIRS,
                                                                                          precision=precision)),
              device="cuda")
    with contextlib.redirect_stdout(sys.stderr):
        return RS.RecordingRestorer(RS.RecordingRestorerConfig(checkpoint_path=os.path.join(tmp, "nppc.pt"),
                                                               model_configuration=mc, **cfg))


def recording():
    n = SR * SECONDS
    t = np.arange(n) / SR
    rng = np.random.default_rng(0)
    x = 0.05 * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 330 * t + 1)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x = (x + 0.005 * rng.standard_normal(n)).astype(np.float32)
    gaps = [(int((i + 0.5) * n / N_GAPS), int((i + 0.5) * n / N_GAPS) + GAP) for i in range(N_GAPS)]
    for s, e in gaps:
        x[s:e] = 0.0
    return torch.from_numpy(x), gaps


def torch_restore(r, x, plan, alphas, variations):
    """restore() with torch indexing on the device in place of nppc_rec_gain / nppc_rec_windows / nppc_rec_splice"""
    from nppc_audio import _hip as H
    from nppc_audio.inpainting import phase as PH
    from nppc_audio.inpainting.data import time_to_spec_mask
    from nppc_audio.inpainting.utils import preprocess_data
    c = r.config
    dev, L, Lw, xf = x.device, x.numel(), c.window_samples, c.crossfade_samples
    W, F, T = len(plan), c.n_fft // 2 + 1, 1 + c.window_samples // c.hop_length
    host = torch.tensor([[p["gap"][0], p["gap"][1], p["start"]] for p in plan], dtype=torch.int64).to(dev)
    s, e, ws = host[:, 0], host[:, 1], host[:, 2]
    with torch.no_grad():
        n = torch.arange(L, device=dev)
        known = torch.ones(L, dtype=torch.bool, device=dev)
        known[((n[None] >= s[:, None]) & (n[None] < e[:, None])).any(0)] = False
        xd = x.double()
        rms = ((xd * xd * known).sum() / known.sum()).sqrt()
        gain = 10.0 ** ((c.target_dB_FS - 20.0 * torch.log10(rms + 1e-8)) / 20.0)
        idx = ws[:, None] + torch.arange(Lw, device=dev)[None]
        mt = known[idx].float()
        xw = ((xd[idx] * gain).float()) * mt
        mf = time_to_spec_mask(mt, T, Lw, c.n_fft, c.hop_length, True)
        spec, masked = torch.empty(W, 2, F, T, device=dev), torch.empty(W, 2, F, T, device=dev)
        H.call("nppc_stft_pair", xw, mf, spec, masked, W, Lw, c.n_fft, c.hop_length, H.stream())
        _, mask4, mn, mean, std = preprocess_data(masked, masked, mf, plot_mean_std=True)
        mask4 = mask4.contiguous()
        pc = r.model(mn, mask4)
        pred = r.model.get_pred_spec_mag_norm(mn, mask4)
        var, rest, info = PH.pc_audio_variations_blind(pred, pc, masked, mf, alphas, mean, std, n_iter=c.gl_iters,
                                                       momentum=c.momentum, n_fft=c.n_fft, hop_length=c.hop_length, length=Lw)
        K, A = var.shape[1], var.shape[2]
        # splice: the ramp weights of one gap, then index assignment gap by gap
        ramp = 0.5 - 0.5 * torch.cos(math.pi * (torch.arange(xf, device=dev, dtype=torch.float64) + 1) / (xf + 1))
        c_gap = torch.cat([ramp, torch.ones(GAP, device=dev, dtype=torch.float64), ramp.flip(0)])
        stack = torch.cat([var.reshape(W, K * A, Lw), rest[:, None]], 1) if variations == "full" else rest[:, None]
        out = x[None].repeat(stack.shape[1], 1)
        for i, p in enumerate(plan):
            a, b = p["gap"][0] - xf, p["gap"][1] + xf
            y = stack[i, :, a - p["start"]:b - p["start"]].double() / gain
            out[:, a:b] = (xd[a:b] + c_gap * (y - xd[a:b])).float()
        res = {"restored": out[-1]}
        if variations == "full":
            res["variations"] = out[:-1].view(K, A, L)
        else:
            res["variation_windows"] = var / gain.float()
    assert not bool(info["status"].any())
    return res


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variations", choices=("windows", "full"), default="windows")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_recording_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore_recording needs a HIP device")
    from nppc_audio import _hip as H
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas
    r = build(a.precision)
    wave, gaps = recording()
    x = wave.cuda()
    alphas = default_alphas("cuda")
    plan = r.plan(x.numel(), gaps)
    runs = {"restore": lambda: r.restore(x, gaps, alphas=alphas, variations=a.variations),
            "torch_indexing": lambda: torch_restore(r, x, plan, alphas, a.variations)}
    times, outs = {k: [] for k in runs}, {}
    for rnd in range(a.warmup + a.rounds):
        for k, fn in runs.items():                                          # alternated: one of each per round
            ms, outs[k] = timed(fn)
            if rnd >= a.warmup:
                times[k].append(ms)
    # the three new kernels' share: device events around every launch of one more call
    H.PROFILE = []
    try:
        total_ms, _ = timed(runs["restore"])
        torch.cuda.synchronize()
        per = {}
        for name, e0, e1 in H.PROFILE:
            per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
    finally:
        H.PROFILE = None
    new_ms = sum(per.get(k, 0.0) for k in NEW_KERNELS)
    res = {"tool": "bench_restore_recording", "seconds": SECONDS, "sample_rate": SR, "gaps": N_GAPS, "gap_samples": GAP,
           "windows": len(plan), "window_samples": r.config.window_samples, "directions": K_DIRS, "alphas": int(alphas.numel()),
           "gl_iters": r.config.gl_iters, "variations": a.variations, "precision": a.precision, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(t, 3) for t in v]}
    res["torch_over_restore"] = res["torch_indexing_ms"]["median"] / res["restore_ms"]["median"]
    res["profiled_call_ms"] = total_ms
    res["new_kernels_ms"] = {k: per.get(k, 0.0) for k in NEW_KERNELS}
    res["new_kernels_share_of_call"] = new_ms / res["restore_ms"]["median"]
    res["entry_points_ms"] = {k: round(v, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    d = (outs["restore"]["restored"].double() - outs["torch_indexing"]["restored"].double()).abs().max()
    res["restored_max_abs_diff_vs_torch"] = float(d)
    res["restored_peak"] = float(outs["restore"]["restored"].abs().max())
    res["restored_finite"] = bool(torch.isfinite(outs["restore"]["restored"]).all())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
