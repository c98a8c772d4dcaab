#!/usr/bin/env python3
"""Train step of the speech-enhancement restorer (FullSubNetPlusTrainer.train_step): STFT of noisy and clean, compressed
cIRM target with drop-band, FullSubNet+ train-mode forward, cIRM MSE, full backward, fused clip_grad_norm_(10) + Adam(1e-3),
and the per-step check of the cooperative-LSTM hand-off time-out counters (a host read: the step is waited for).

Default shape: FullSubNet_plus/config/train.toml, batch 18 x 3.072 s at 16 kHz, STFT 512 / 256, num_groups_in_drop_band 2
(T = 193, F' = 128, 2304 sub-band sequences); `--batch 32 --seconds 4` is the C2 batch.  Clips are synthetic and made on
the device.  Runs bf16 and fp32 (or one of them with --precision) and prints ONE JSON line: ms/step and spectrogram
frames/s per precision.
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, ROOT)
SR, NFFT, HOP = 16000, 512, 256


def log(msg):
    print(f"[bench-fsn-restorer {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def synth(B, L, dev):
    """noisy / clean [B, L] on the device: amplitude-modulated low-passed noise as 'speech', white noise at 0..20 dB SNR"""
    g = torch.Generator(device=dev).manual_seed(1234)
    t = torch.arange(L, device=dev, dtype=torch.float32) / SR
    w = torch.randn(B, L, generator=g, device=dev)
    k = torch.ones(1, 1, 9, device=dev) / 9.0
    col = torch.nn.functional.conv1d(w[:, None], k, padding=4)[:, 0]
    env = 0.5 * (1 - torch.cos(2 * torch.pi * 4.0 * t[None] + torch.rand(B, 1, generator=g, device=dev) * 6.28))
    clean = 0.05 * col / col.std(dim=1, keepdim=True) * (0.2 + env)
    snr = torch.rand(B, 1, generator=g, device=dev) * 20.0
    n = torch.randn(B, L, generator=g, device=dev)
    n = n * torch.sqrt(clean.pow(2).mean(1, keepdim=True) / 10 ** (snr / 10) / n.pow(2).mean(1, keepdim=True))
    return (clean + n).contiguous(), clean.contiguous()


def build(precision, B, groups):
    from nppc_audio.restorer_trainer import FullSubNetPlusTrainer, FullSubNetPlusTrainerConfig
    torch.manual_seed(0)
    cfg = FullSubNetPlusTrainerConfig(
        model_configuration=dict(num_groups_in_drop_band=groups, precision=precision),
        dataloader_configuration=dict(batch_size=B, num_workers=0, pin_memory=False, shuffle=False),
        stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT), device="cuda")

    class One(torch.utils.data.Dataset):
        def __len__(self):
            return B

        def __getitem__(self, i):
            raise IndexError

    with contextlib.redirect_stdout(sys.stderr):
        return FullSubNetPlusTrainer(cfg, dataset=One())


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="both", choices=["both", "bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=18)
    ap.add_argument("--seconds", type=float, default=3.072)
    ap.add_argument("--groups", type=int, default=2, help="num_groups_in_drop_band")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.seconds <= 0 or a.groups < 1:
        ap.error("--seconds must be > 0 and --groups >= 1")
    if a.batch <= a.groups:
        ap.error(f"--batch must be larger than --groups (drop_band needs batch > num_groups): {a.batch} <= {a.groups}")
    return a


def run(a, precision):
    L = int(round(a.seconds * SR))
    T = 1 + L // HOP
    tr = build(precision, a.batch, a.groups)
    batch = synth(a.batch, L, "cuda")
    log(f"{precision}: batch [{a.batch}, {L}] (T = {T}); {a.warmup} warm-up + {a.steps} timed steps")
    for _ in range(a.warmup):
        tr.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, _ = tr.train_step(batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1e3 * dt / a.steps
    log(f"{precision}: {ms:.2f} ms/step")
    return {"ms_per_step": ms, "frames_per_s": a.batch * T * a.steps / dt, "loss_last": float(loss.detach())}, T


def main(argv=None):
    a = parse(argv)
    torch.cuda.set_device(0)
    precs = ["bf16", "fp32"] if a.precision == "both" else [a.precision]
    res, T = {}, None
    for p in precs:
        res[p], T = run(a, p)
    head = res[precs[0]]
    out = {
        "metric": "spectrogram-frames/sec, FullSubNet+ restorer train step",
        "value": head["frames_per_s"], "unit": "frames/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "dtype": precs[0], "data": "synthetic",
        "per_precision": res,
        "config": {"workload": f"FullSubNet+ restorer, batch={a.batch}x{a.seconds:g}s@16kHz, STFT {NFFT}/{HOP} (F=257, "
                               f"T={T}), drop-band G={a.groups}, full train step (STFT+target+fwd+loss+bwd+clip+Adam)",
                   "frames_per_step": a.batch * T},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
