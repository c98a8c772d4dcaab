#!/usr/bin/env python3
"""Held-out validation of the NPPC speech-enhancement step: ragged batches vs one clip at a time.

Workload: --clips seeded synthetic 16 kHz clips, lengths uniform in [--min-s, --max-s] seconds, at the BASELINE C2 network
size (F = 257, sub-band hidden 384, K = 5 directions, bf16 by default, torch default-init weights as in bench.py).
  (a) one clip at a time through the UNIFORM kernels (batch of one: NPPCModel.forward, nppc_cirm_build_compress, NPPCLoss),
      the per-clip loss terms gathered on the device and copied to the host once, as validate does;
  (b) NPPCAudioTrainer.validate on ragged batches (data.pad_collate) of every size in --batches, clips sorted by length
      (--order dataset: in dataset order).
Every run goes twice; the second (warm: per-shape buffers exist) is timed with device events around the whole pass,
host work of the pass included.  Prints ONE JSON line: ms and ms per clip of each run, the padding fraction of each
batching, and the ratio (a) / (b).
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, ROOT)
SR, NFFT, HOP, K_DIRS = 16000, 512, 256, 5


def log(msg):
    print(f"[bench-nppc-val {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def clip_lengths(n, min_s, max_s, seed):
    g = torch.Generator().manual_seed(seed)
    return [int(SR * (min_s + (max_s - min_s) * float(u))) for u in torch.rand(n, generator=g)]


def plan_batches(lengths, bs, order):
    """index lists of the batches and the padding fraction: frames computed past an item's end / frames computed"""
    idx = sorted(range(len(lengths)), key=lambda i: lengths[i]) if order == "sorted" else list(range(len(lengths)))
    groups = [idx[k:k + bs] for k in range(0, len(idx), bs)]
    frames = lambda n: 1 + n // HOP
    computed = sum(len(g) * frames(max(lengths[i] for i in g)) for g in groups)
    return groups, 1.0 - sum(frames(n) for n in lengths) / computed


def build_trainer(precision, n_dirs=K_DIRS):
    from nppc_audio.data import SyntheticNoisySpeech
    from nppc_audio.fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
    from nppc_audio.trainer import NPPCAudioTrainer, NPPCAudioTrainerConfig
    torch.manual_seed(0)
    rest_cfg = dict(num_groups_in_drop_band=1, precision=precision)
    tmp = tempfile.mkdtemp(prefix="nppc_val_bench_")
    ck = os.path.join(tmp, "restorer.tar")
    torch.save({"model": FullSubNet_Plus(FullSubNetPlusConfig(**rest_cfg)).state_dict()}, ck)
    cfg = NPPCAudioTrainerConfig(
        nppc_model_configuration=dict(
            pretrained_restoration_model_configuration=rest_cfg, pretrained_restoration_model_path=ck,
            audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(
                num_groups_in_drop_band=2, n_directions=n_dirs, precision=precision)),
            stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT), device="cuda"),
        data_configuration=dict(data_path=".", dataset=dict(clean_path=".", noisy_path=".")),
        data_loader_configuration=dict(batch_size=2, num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=0)),
        device="cuda")
    with contextlib.redirect_stdout(sys.stderr):
        return NPPCAudioTrainer(cfg, dataset=SyntheticNoisySpeech(2, SR))


def one_clip_uniform(model, noisy, clean, lam):
    """the loss terms of ONE clip through the uniform kernels (a batch of one never drop-bands): [1, 2 + 3K]"""
    from nppc_audio import _hip as H
    from nppc_audio import ops
    from nppc_audio.pc_ops import NPPCLoss
    st = model.config.stft_configuration
    w = model(noisy[None])
    f = model._front(noisy[None])
    _, c_re, c_im = ops.stft(clean[None], st.nfft, st.hop_length, want_mag=False)
    B, F, T = f["re"].shape
    gt = torch.empty(B, 2, F, T, dtype=torch.float32, device=noisy.device)
    H.call("nppc_cirm_build_compress", f["re"], f["im"], c_re, c_im, gt, B, F, T, 1, ops.EPS32, H.stream())
    rec, _, en, _, _, pm, wn, sm = NPPCLoss.apply(w, gt, f["pred_crm"], lam)
    return torch.cat([en[:, None], rec[:, None], pm, wn, sm], dim=1)


def timed(fn):
    fn()                                    # cold pass: per-shape buffers, plans
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batches", default="4,8,16,32", help="ragged batch sizes, comma separated")
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=6.0)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--order", default="sorted", choices=["sorted", "dataset"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-one-by-one", action="store_true", help="leave run (a) out")
    a = ap.parse_args(argv)
    sizes = [int(s) for s in a.batches.split(",") if s]
    from nppc_audio.data import pad_collate, synth_clip
    lengths = clip_lengths(a.clips, a.min_s, a.max_s, a.seed)
    items = [tuple(torch.from_numpy(x) for x in synth_clip(500 + i, n)) for i, n in enumerate(lengths)]
    tr = build_trainer(a.precision)
    dev = torch.device("cuda")
    res = dict(tool="bench_nppc_validation", clips=a.clips, seconds=[a.min_s, a.max_s], precision=a.precision, order=a.order,
               n_directions=K_DIRS, total_audio_s=round(sum(lengths) / SR, 1), frames=sum(1 + n // HOP for n in lengths))
    if not a.no_one_by_one:
        log("(a) one clip at a time, uniform kernels")
        dev_items = [(n.to(dev), c.to(dev)) for n, c in items]

        def one_by_one():
            with torch.no_grad():
                return torch.cat([one_clip_uniform(tr.nppc_model, n, c, 1.0) for n, c in dev_items]).cpu()
        ms, block = timed(one_by_one)
        res["one_by_one"] = dict(ms=round(ms, 2), ms_per_clip=round(ms / a.clips, 3), reconst_err=float(block[:, 1].mean()))
    res["ragged"] = {}
    for bs in sizes:
        groups, pad = plan_batches(lengths, bs, a.order)
        loader = [pad_collate([items[i] for i in g]) for g in groups]
        loader = [type(b)(b.noisy.to(dev), b.clean.to(dev), b.lengths) for b in loader]
        log(f"(b) validate, ragged batches of {bs}")
        with contextlib.redirect_stdout(sys.stderr):
            ms, m = timed(lambda: tr.validate(loader))
        r = dict(ms=round(ms, 2), ms_per_clip=round(ms / a.clips, 3), padding_fraction=round(pad, 4), reconst_err=m["reconst_err"])
        if "one_by_one" in res:
            r["speedup_vs_one_by_one"] = round(res["one_by_one"]["ms"] / ms, 3)
        res["ragged"][str(bs)] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
