#!/usr/bin/env python3
"""Times RecordingEnhancer.enhance (nppc_audio/enhance.py, csrc/enhance_rec.hip) on whole recordings of the benchmarks'
synthetic noisy speech: 60 s and 10 min at 16 kHz, K = 5 directions, alphas = default_alphas() (13), chunks of 65536 samples
in batches of 32, the BASELINE network sizes.

Beside it runs the same result from the pieces that existed before: per chunk ops.pc_direction_waveforms (K A + 1 inverse
STFTs, alpha applied before the transform), then the alignment (Gram, cosines, greedy chain) and the weighted overlap-add
written with torch operators on the device, with no host read.  The chunking and the nets are the same code in both.  The two
are alternated round by round after a warm-up; a round is timed with the host clock around a device synchronise.  The three
new kernels are then timed on their own with device events on the chunk waveforms of the last call, and the splice's bytes
(4 L (2 (K + 1) + 1 + K A)) are set against the measured 6.29 TB/s copy rate.  Weights are a seeded draw: the timing does not
depend on them.

    python tools/bench_enhance_recording.py [--seconds 60 600] [--rounds 20] [--warmup 5] [--precision bf16] [--out FILE]
"""
import argparse
import contextlib
import json
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
SR, NFFT, HOP, K_DIRS = 16000, 512, 256, 5
COPY_RATE = 6.29e12                            # bytes / s, the measured device copy rate the splice is judged against


def build(precision, chunk_samples, chunk_batch):
    from nppc_audio import enhance as EN
    from nppc_audio.fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
    from nppc_audio.nppc_model import NPPCModel, NPPCModelConfig
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="nppc_bench_enhance_")
    rest = dict(num_groups_in_drop_band=1, precision=precision)
    ck = os.path.join(tmp, "restorer.tar")
    torch.save({"model": FullSubNet_Plus(FullSubNetPlusConfig(**rest)).state_dict()}, ck)
    cfg = NPPCModelConfig(pretrained_restoration_model_configuration=rest, pretrained_restoration_model_path=ck,
                          audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(
                              num_groups_in_drop_band=2, n_directions=K_DIRS, precision=precision)),
                          stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT), device="cuda")
    with contextlib.redirect_stdout(sys.stderr):
        torch.save({"model_state_dict": NPPCModel(cfg).state_dict()}, os.path.join(tmp, "nppc.pt"))
        return EN.RecordingEnhancer(EN.RecordingEnhancerConfig(model_configuration=cfg, checkpoint_path=os.path.join(tmp, "nppc.pt"),
                                                               chunk_samples=chunk_samples, chunk_batch=chunk_batch))


def recording(seconds):
    """the benchmarks' synthetic noisy speech, 10 s clips end to end"""
    from nppc_audio.data import synth_clip
    parts, left, i = [], seconds * SR, 0
    while left > 0:
        n = min(left, 10 * SR)
        parts.append(synth_clip(700 + i, n)[0])
        left, i = left - n, i + 1
    return torch.from_numpy(np.concatenate(parts).astype(np.float32))


def torch_enhance(r, x, alphas, alpha_list):
    """enhance() from the pieces that existed before it: pc_direction_waveforms per batch of chunks, alignment and
    overlap-add with torch operators on the device"""
    from nppc_audio import ops
    from nppc_audio.enhance import hann_table
    c, st = r.config, r.config.model_configuration.stft_configuration
    C, Hh, L = c.chunk_samples, c.chunk_samples // 2, x.numel()
    plan = r.plan(L)
    n, A, dev = len(plan), alphas.numel(), x.device
    W = L if n == 1 else C
    chunks = torch.zeros(n, W, device=dev)
    if n == 1:
        chunks[0] = x
    else:
        chunks[:n - 1] = x.unfold(0, C, Hh)[:n - 1]
        chunks[n - 1, :plan[-1][1]] = x[plan[-1][0]:]
    e_all, v_all = [], []
    with torch.no_grad():
        for b0 in range(0, n, c.chunk_batch):
            xb = chunks[b0:b0 + c.chunk_batch]
            lens = [ln for _, ln in plan[b0:b0 + c.chunk_batch]]
            w_mat = r.model(xb, lengths=lens)
            f = r.model._front(xb, lengths=lens)
            e, var = ops.pc_direction_waveforms(f["pred_crm"], w_mat, alpha_list, f["re"], f["im"],
                                                W, st.nfft, st.hop_length)
            e_all.append(e), v_all.append(var)
        e, var = torch.cat(e_all), torch.cat(v_all)                                   # [n, W], [n, K, A, W]
        K = var.shape[1]
        if n > 1:
            last = plan[-1][1]
            e[n - 1, last:], var[n - 1, :, :, last:] = 0, 0                             # the uniform transform wrote past the end
        # a direction's waveform, for the alignment: (variation at alpha_hi - variation at alpha_lo) / (alpha_hi - alpha_lo)
        p = (var[:, :, -1] - var[:, :, 0]) / (alphas[-1] - alphas[0])                 # [n, K, W]
        perm = torch.arange(K, device=dev).repeat(n, 1)
        sign = torch.ones(n, K, device=dev)
        if n > 1:
            a, b = p[:-1, :, Hh:].double(), p[1:, :, :Hh].double()
            G = torch.einsum("cji,cki->cjk", a, b)
            d = (a * a).sum(-1)[:, :, None] * (b * b).sum(-1)[:, None, :]
            cos = torch.where(d == 0, torch.zeros_like(G), G / d.sqrt()).abs()
            for ch in range(1, n):
                taken = torch.zeros(K, dtype=torch.bool, device=dev)
                for s in range(K):
                    j = perm[ch - 1, s]
                    k = torch.where(taken, -1.0, cos[ch - 1, j]).argmax()
                    taken[k] = True
                    perm[ch, s] = k
                    sign[ch, s] = sign[ch - 1, s] * torch.where(G[ch - 1, j, k] >= 0, 1.0, -1.0)
        # aligned variations: e + sign (var[perm] - e), then the weighted overlap-add
        idx = perm[:, :, None, None].expand(n, K, A, W)
        y = e[:, None, None] + sign[:, :, None, None] * (var.gather(1, idx) - e[:, None, None])
        rows = torch.cat([e[:, None], y.reshape(n, K * A, W)], 1)                    # [n, V, W]
        if n == 1:
            return {"enhanced": rows[0, 0], "variations": rows[0, 1:].view(K, A, L)}
        w = hann_table(C, dev)
        head = torch.cat([torch.ones(1, Hh, device=dev), w.repeat(n - 1, 1)])         # weight of a chunk's first half
        tail = torch.cat([(1 - w).repeat(n - 1, 1), torch.ones(1, Hh, device=dev)])   # and of its second half
        out = torch.zeros(rows.shape[1], (n + 1) * Hh, device=dev)
        out[:, :n * Hh].unflatten(1, (n, Hh)).add_((rows[:, :, :Hh] * head[:, None]).transpose(0, 1))
        out[:, Hh:].unflatten(1, (n, Hh)).add_((rows[:, :, Hh:] * tail[:, None]).transpose(0, 1))
        return {"enhanced": out[0, :L], "variations": out[1:, :L].unflatten(0, (K, A))}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, rounds, warmup):
    ts = []
    for i in range(warmup + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def one(r, seconds, alphas, alpha_list, rounds, warmup):
    from nppc_audio import enhance as EN
    x = recording(seconds).cuda()
    runs = {"enhance": lambda: r.enhance(x, alphas), "torch_pieces": lambda: torch_enhance(r, x, alphas, alpha_list)}
    times, outs = {k: [] for k in runs}, {}
    for rnd in range(warmup + rounds):
        for k, fn in runs.items():                                          # alternated: one of each per round
            ms, outs[k] = timed(fn)
            if rnd >= warmup:
                times[k].append(ms)
    res = {"seconds": seconds, "samples": x.numel(), "chunks": len(outs["enhance"]["chunks"])}
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(t, 3) for t in v]}
    res["torch_over_enhance"] = res["torch_pieces_ms"]["median"] / res["enhance_ms"]["median"]
    peak = float(outs["enhance"]["variations"].abs().max())
    # the last n_fft samples are left out: the uniform inverse STFT of the pieces normalises the shorter last chunk's end by
    # an envelope that counts the padded frames
    cut = x.numel() - NFFT
    res["variations_max_abs_diff_vs_torch_over_peak"] = float(
        (outs["enhance"]["variations"][..., :cut] - outs["torch_pieces"]["variations"][..., :cut]).abs().max()) / peak
    res["finite"] = bool(torch.isfinite(outs["enhance"]["variations"]).all())
    res["continuity_min_median"] = [float(outs["enhance"]["continuity"].min()), float(outs["enhance"]["continuity"].median())]
    outs.clear()
    # the three kernels on their own, on the chunk waveforms of one call
    plan = r.plan(x.numel())
    buf = r.chunk_waveforms(x, plan)
    enh, pcs, last = buf[:, 0], buf[:, 1:], plan[-1][1]
    n, K, C = pcs.shape
    L, A = x.numel(), alphas.numel()
    if n > 1:
        work, S = EN.boundary_gram(pcs)
        perm, sign, _ = EN.chain(work, n, K)
        res["gram_split"] = S
        res["gram_ms"] = event_ms(lambda: EN.boundary_gram(pcs), rounds, warmup)
        res["chain_ms"] = event_ms(lambda: EN.chain(work, n, K), rounds, warmup)
        res["gram_bytes"] = 8 * K * (C // 2) * (n - 1)
        res["gram_share_of_copy_rate"] = res["gram_bytes"] / (res["gram_ms"] * 1e-3) / COPY_RATE
    else:
        perm, sign, _ = EN.chain(None, 1, K, device=x.device)
    res["splice_ms"] = event_ms(lambda: EN.splice(enh, pcs, last, alphas, perm, sign), rounds, warmup)
    res["splice_bytes"] = 4 * L * (2 * (K + 1) + 1 + K * A)
    res["splice_bytes_per_s"] = res["splice_bytes"] / (res["splice_ms"] * 1e-3)
    res["splice_share_of_copy_rate"] = res["splice_bytes_per_s"] / COPY_RATE
    res["new_kernels_share_of_call"] = (res.get("gram_ms", 0.0) + res.get("chain_ms", 0.0) + res["splice_ms"]) / res["enhance_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--chunk-samples", type=int, default=65536)
    ap.add_argument("--chunk-batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance_recording_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enhance_recording needs a HIP device")
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas
    r = build(a.precision, a.chunk_samples, a.chunk_batch)
    alphas = default_alphas("cuda").float()
    alpha_list = [float(v) for v in alphas.tolist()]                         # one host read, before anything is timed
    res = {"tool": "bench_enhance_recording", "sample_rate": SR, "directions": K_DIRS, "alphas": int(alphas.numel()),
           "chunk_samples": a.chunk_samples, "chunk_batch": a.chunk_batch, "precision": a.precision, "rounds": a.rounds,
           "warmup": a.warmup, "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0),
           "recordings": [one(r, s, alphas, alpha_list, a.rounds, a.warmup) for s in a.seconds]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
