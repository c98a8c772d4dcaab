#!/usr/bin/env python3
"""One minibatch of the DNS dynamic mixer on the device (nppc_audio.dns_data.DeviceReverbMixLoader) at the shape of
FullSubNet_plus/config/train.toml: batch 18 x 3.072 s at 16 kHz, reverb_proportion 0.75, SNR -5..20 dB, level -25 +- 10.

Per room-impulse-response length (default 4000, 16000 and L = 49152 taps) it times, with device events, the upload of the
un-mixed ingredients, nppc_rir_convolve and nppc_dns_snr_mix (medians over --steps batches, every batch newly drawn), and
reports the convolution's multiply-adds per second against the fp32 vector peak (157.3 TFLOP/s = 78.65 T multiply-adds/s;
the kernel runs fp64 FMAs, whose peak is half of that), each time as a share of the restorer's train step
(tools/bench_fsn_restorer.py, run in the same process unless --no-restorer), the host's gather time and, for orientation,
what the reference does per batch on the host: snr_mix with scipy's fftconvolve over the same 18 items
(dns_data.snr_mix_host, at most 16 threads).  Clips are synthetic.  Prints ONE JSON line."""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PEAK_FMA = 157.3e12 / 2


def log(msg):
    print(f"[bench-dns-mix {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def make_dataset(batch, taps, seed):
    from nppc_audio.dns_data import DNSDatasetConfig, DynamicMixDataset
    rng = np.random.Generator(np.random.PCG64(seed))
    cfg = DNSDatasetConfig()
    clean = [(0.1 * rng.standard_normal(4 * cfg.sr)).astype(np.float32) for _ in range(batch)]
    noise = [(0.05 * rng.standard_normal(int(n * cfg.sr))).astype(np.float32) for n in (1.0, 2.5, 5.0, 0.7)]
    rir = [(rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.0))).astype(np.float32) for _ in range(4)]
    return DynamicMixDataset(cfg, clean, noise, rir, seed=seed)


def macs(rir_len, L):
    n = np.minimum(rir_len.astype(np.int64), L)
    return int((n * L - n * (n - 1) // 2).sum())


def run(batch, taps, steps, warmup):
    from nppc_audio.dns_data import DeviceReverbMixLoader, rir_convolve_on_device, snr_mix_host, snr_mix_on_device
    ds = make_dataset(batch, taps, seed=taps)
    loader = DeviceReverbMixLoader(ds, None, device="cuda", pin_memory=True)
    L, idxs = ds.config.crop_length, list(range(batch))
    rows = {k: [] for k in ("gather_ms", "upload_ms", "conv_ms", "mix_ms", "conv_macs")}
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        host = loader.gather(idxs)
        gather = 1e3 * (time.perf_counter() - t0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        clean, noise, rir, rir_len, meta = loader.upload(host)
        ev[1].record()
        rev = rir_convolve_on_device(clean, rir, rir_len, check_lengths=False)
        ev[2].record()
        noisy, cl = snr_mix_on_device(rev, noise, meta[:, 0].contiguous(), meta[:, 1].contiguous(), ds.config.target_dB_FS)
        ev[3].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, v in zip(rows, (gather, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3]),
                                   macs(host[3].numpy(), L))):
                rows[k].append(v)
    assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(cl).all())
    out = {k: statistics.median(v) for k, v in rows.items()}
    out["conv_macs_per_s"] = out["conv_macs"] / (1e-3 * out["conv_ms"]) if out["conv_ms"] > 0 else 0.0
    out["conv_share_of_fp32_vector_peak"] = out["conv_macs_per_s"] / PEAK_FMA
    out["reverberant_items"] = int((host[3] > 0).sum())
    # the reference's per-batch host work on the same kind of items
    items = [ds.draw(i) for i in idxs]
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(max_workers=min(16, batch)) as ex:
        list(ex.map(lambda i: snr_mix_host(i.clean, i.noise, i.snr, ds.config.target_dB_FS, i.level, rir=i.rir), items))
    out["host_snr_mix_ms"] = 1e3 * (time.perf_counter() - t0)
    log(f"{taps} taps: gather {out['gather_ms']:.2f} ms, upload {out['upload_ms']:.3f}, convolve {out['conv_ms']:.3f} "
        f"({out['conv_macs_per_s'] / 1e12:.2f} T multiply-adds/s), mix {out['mix_ms']:.3f}; host snr_mix {out['host_snr_mix_ms']:.1f} ms")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=18)
    ap.add_argument("--taps", type=int, nargs="+", default=[4000, 16000, 49152])
    ap.add_argument("--no-restorer", action="store_true", help="skip the restorer train step the shares refer to")
    a = ap.parse_args(argv)
    torch.cuda.set_device(0)
    res = {str(t): run(a.batch, t, a.steps, a.warmup) for t in a.taps}
    step_ms = None
    if not a.no_restorer:
        import bench_fsn_restorer as R
        step_ms = R.run(R.parse(["--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch)]), "bf16")[0]["ms_per_step"]
        for r in res.values():
            for k in ("upload_ms", "conv_ms", "mix_ms"):
                r[k.replace("_ms", "_share_of_step")] = r[k] / step_ms
    print(json.dumps({"metric": "DNS dynamic mixing, one minibatch on the device", "unit": "ms", "batch": a.batch,
                      "steps": a.steps, "warmup": a.warmup, "restorer_step_ms_bf16": step_ms, "per_rir_taps": res}))


if __name__ == "__main__":
    main()
