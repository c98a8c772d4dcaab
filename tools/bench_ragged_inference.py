#!/usr/bin/env python3
"""Validation-set inference of the FullSubNet+ restorer: one clip at a time vs ragged batches.

Workload: a seeded validation set of --clips synthetic 16 kHz clips, lengths uniform in [--min-s, --max-s] seconds, at the
train.toml restorer shape (F = 257, sub-band hidden 384, bf16, random weights from oracle/weights.py).  Three runs through
ModelValidator.enhance_audio:
  (a) one clip at a time (the reference validates with batch size 1);
  (b) ragged batches of --batch clips in dataset order (data.pad_collate, enhance_audio(lengths=));
  (c) the same clips in batches sorted by length.
Each run goes twice; the second (warm: the engine's per-shape buffers exist) is timed with device events.  Also: the
padding fraction (frames computed past an item's end / frames computed) of (b) and (c), and the time of scoring (c)'s
enhanced clips with STOI and SI-SDR (metrics.stoi / si_sdr_zero_mean with lengths).  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, ROOT)
SR = 16000


def log(msg):
    print(f"[bench-ragged {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def synth_clips(lengths, dev, seed=1234):
    """(noisy, clean) device clips: amplitude-modulated low-passed noise as 'speech', white noise at 0..20 dB SNR"""
    g = torch.Generator(device=dev).manual_seed(seed)
    k = torch.ones(1, 1, 9, device=dev) / 9.0
    out = []
    for n in lengths:
        t = torch.arange(n, device=dev, dtype=torch.float32) / SR
        col = torch.nn.functional.conv1d(torch.randn(1, 1, n, generator=g, device=dev), k, padding=4)[0, 0]
        env = 0.5 * (1 - torch.cos(2 * torch.pi * 4.0 * t + float(torch.rand(1, generator=g, device=dev)) * 6.28))
        clean = 0.05 * col / col.std() * (0.2 + env)
        noise = torch.randn(n, generator=g, device=dev)
        snr = float(torch.rand(1, generator=g, device=dev)) * 20.0
        noise = noise * (clean.pow(2).mean() / noise.pow(2).mean() / 10 ** (snr / 10)).sqrt()
        out.append((clean + noise, clean))
    return out


def make_validator(precision, tmp):
    from oracle import weights as W
    from nppc_audio.model_validator import ModelValidator, ModelValidatorConfig
    wts = W.make_weights(W.restorer_spec(num_freqs=257, sb_neighbors=15, sb_hidden=384), 5)
    ck = os.path.join(tmp, "restorer.tar")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in wts.items()}}, ck)
    cfg = ModelValidatorConfig(model_path=ck, model_configuration=dict(num_freqs=257, sb_num_neighbors=15,
                                                                         sb_model_hidden_size=384, precision=precision),
                               device="cuda", audio_config=dict(sr=SR, stft_configuration=dict(nfft=512, hop_length=256,
                                                                                                win_length=512)))
    return ModelValidator(cfg)


def batches(items, order, bs):
    from nppc_audio.data import pad_collate
    return [pad_collate([items[i] for i in order[k:k + bs]]) for k in range(0, len(order), bs)]


def timed(fn):
    fn()                                    # cold pass: per-shape buffers, plans
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=150)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=12.0)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--runs", default="abc", help="subset of a, b, c")
    a = ap.parse_args()
    from nppc_audio import metrics
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(a.seed)
    lengths = [int(SR * (a.min_s + (a.max_s - a.min_s) * float(u))) for u in torch.rand(a.clips, generator=g)]
    items = [(n.cpu(), c.cpu()) for n, c in synth_clips(lengths, dev)]
    with tempfile.TemporaryDirectory() as tmp:
        mv = make_validator(a.precision, tmp)
    hop = 256
    frames = [1 + n // hop for n in lengths]
    res = dict(tool="bench_ragged_inference", clips=a.clips, batch=a.batch, seconds=[a.min_s, a.max_s],
               precision=a.precision, total_audio_s=round(sum(lengths) / SR, 1), frames=sum(frames))
    dev_items = [(n.to(dev), c.to(dev)) for n, c in items]

    if "a" in a.runs:
        log("(a) one clip at a time")
        ms, _ = timed(lambda: [mv.enhance_audio(n) for n, _ in dev_items])
        res["a_one_by_one"] = dict(ms=round(ms, 2), clips_per_s=round(a.clips / ms * 1e3, 2))
    for tag, order in (("b_ragged_dataset_order", list(range(a.clips))),
                       ("c_ragged_sorted", sorted(range(a.clips), key=lambda i: lengths[i]))):
        if tag[0] not in a.runs:
            continue
        log(f"({tag[0]}) ragged batches of {a.batch}")
        bl = batches(items, order, a.batch)
        dl = [(b.noisy.to(dev), b.lengths) for b in bl]
        computed = sum(len(b.lengths) * (1 + int(b.lengths.max()) // hop) for b in bl)
        ms, enh = timed(lambda: [mv.enhance_audio(n, lengths=L) for n, L in dl])
        res[tag] = dict(ms=round(ms, 2), clips_per_s=round(a.clips / ms * 1e3, 2),
                        padding_fraction=round(1 - sum(frames) / computed, 4))
        if tag[0] == "c":
            sc = [(b.clean.to(dev), e, b.lengths.to(dev, torch.int32)) for b, e in zip(bl, enh)]
            ms_s, _ = timed(lambda: [(metrics.stoi(c, e, lengths=L), metrics.si_sdr_zero_mean(c, e, lengths=L))
                                     for c, e, L in sc])
            res[tag]["scoring_ms"] = round(ms_s, 2)
    if "a_one_by_one" in res:
        for tag in ("b_ragged_dataset_order", "c_ragged_sorted"):
            if tag in res:
                res[tag]["speedup_vs_a"] = round(res["a_one_by_one"]["ms"] / res[tag]["ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
