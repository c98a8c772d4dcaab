#!/usr/bin/env python3
"""One minibatch of the inpainting dataset at the shape of the reference's training yaml: batch 128 x 2.044 s at 16 kHz,
nfft 255 / hop 128, a 128 ms gap placed by the voice-activity detector.

It times three things (medians over --steps batches after --warmup, a host clock around work that ends in a device
synchronise):
- device_loader_ms: nppc_audio.inpainting.data.InpaintingDeviceLoader.batch, every batch newly drawn (another epoch);
- host_loader_ms: the same batch assembled on the host, the only way without the loader -- a torch Dataset that does the
  restatement's work per item (tests/vad_ref.py: crop, gain, energy VAD, gap draw) plus torch.stft and the frame mask,
  behind a DataLoader with at most 16 workers, then one upload per tensor;
- c3_step_ms: the inpainting NPPC train step (tools/bench_inpainting.py, what bench.py --config c3 runs) at the same batch
  shape, bf16, for scale.
It reports the loader's achieved bytes per second -- the bytes the three launches have to move, from the shapes -- against
the HBM rate (6.29 TB/s measured copy rate, 8 TB/s specified).  Clips are synthetic noise bursts.  Prints ONE JSON line."""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
SR, NFFT, HOP = 16000, 255, 128


def log(msg):
    print(f"[bench-inpaint-data {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def make_clips(n, seconds, seed):
    import vad_ref as R
    rng = np.random.Generator(np.random.PCG64(seed))
    clips = []
    for i in range(n):
        flen, spans, pos = int(seconds * SR), [], int(rng.integers(0, 8000))
        while pos < flen - 4000:
            dur = int(rng.integers(3000, 24000))
            spans.append((pos, min(pos + dur, flen)))
            pos += dur + int(rng.integers(800, 12000))
        clips.append(torch.from_numpy(R.bursts(flen, spans, seed * 1000 + i)))
    return clips


def data_config(seconds, missing_seconds):
    from nppc_audio.inpainting.trainer.nppc_trainer import AudioInpaintingConfig
    return AudioInpaintingConfig(clean_path=".", stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT),
                                 sub_sample_length_seconds=seconds, missing_length_seconds=missing_seconds, use_vad=True)


def loader_bytes(B, L, F, T):
    """what the three launches have to move: crop read + clean write; clean read + masked audio and frame mask write;
    clean read + two spectra write"""
    return 4 * (B * L * 5 + B * T * 2 + 2 * B * 2 * F * T)


class HostItems(torch.utils.data.Dataset):
    """the batch the parent commit's trainers could be fed: every item prepared on the host"""

    def __init__(self, ds, epoch):
        self.clips = [c.numpy() for c in ds.clean]
        self.gain = [float(g) for g in ds.gain]
        self.L, self.miss, self.seed, self.epoch = ds.sub_sample_length, ds.missing_length, ds.seed, epoch
        self.window = torch.hann_window(NFFT)

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        import vad_ref as R
        it = R.item(self.clips[i], self.gain[i], self.L, self.miss, self.seed, i, self.epoch)
        clean = torch.from_numpy(it["clean"])
        spec = torch.view_as_real(torch.stft(clean, NFFT, HOP, NFFT, self.window, center=True, pad_mode="reflect",
                                             return_complex=True)).permute(2, 0, 1).contiguous()
        T = spec.shape[2]
        t = torch.arange(T)
        s, e = (t * HOP - NFFT // 2).clamp(min=0), (t * HOP - NFFT // 2 + NFFT).clamp(max=self.L)
        mask = (~((s < it["gap_end"]) & (e > it["gap_start"]))).float()
        masked_audio = clean.clone()
        masked_audio[it["gap_start"]:it["gap_end"]] = 0
        return spec * mask, mask, spec, masked_audio[None]


def median_ms(fn, steps, warmup):
    rows = []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(it)
        torch.cuda.synchronize()
        if it >= warmup:
            rows.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(rows), min(rows), max(rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=2.044)
    ap.add_argument("--clip-seconds", type=float, default=12.0, help="length of every synthetic recording")
    ap.add_argument("--workers", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--no-step", action="store_true", help="skip the C3 train step the share refers to")
    ap.add_argument("--no-host", action="store_true", help="skip the host-assembled batch")
    a = ap.parse_args(argv)
    from nppc_audio.inpainting.data import AudioInpaintingDataset, InpaintingDeviceLoader
    torch.cuda.set_device(0)
    ds = AudioInpaintingDataset(data_config(a.seconds, 0.128), clean_clips=make_clips(a.batch, a.clip_seconds, 7), seed=11)
    loader = InpaintingDeviceLoader(ds, None)
    idxs, L = list(range(a.batch)), ds.sub_sample_length
    F, T = NFFT // 2 + 1, 1 + L // HOP
    keep = {}

    def device_batch(it):
        loader.set_epoch(it)
        keep["out"] = loader.batch(idxs)

    dev = median_ms(device_batch, a.steps, a.warmup)
    meta = keep["out"][4]
    nbytes = loader_bytes(a.batch, L, F, T)
    out = {"metric": "inpainting minibatch assembly", "unit": "ms", "batch": a.batch, "seconds": a.seconds, "samples": L,
           "frames": T, "steps": a.steps, "warmup": a.warmup,
           "device_loader_ms": dev[0], "device_loader_ms_min_max": dev[1:],
           "fallback_items": int((meta["used_fallback"] != 0).sum()), "segments_per_item": float(meta["n_segments"].float().mean()),
           "gap_frames": sorted(set((keep["out"][1] == 0).sum(1).tolist())),
           "loader_bytes": nbytes, "loader_bytes_per_s": nbytes / (1e-3 * dev[0]),
           "share_of_hbm_measured_6.29TBps": nbytes / (1e-3 * dev[0]) / HBM_MEASURED,
           "share_of_hbm_spec_8TBps": nbytes / (1e-3 * dev[0]) / HBM_SPEC}
    log(f"device loader {dev[0]:.3f} ms ({out['loader_bytes_per_s'] / 1e9:.1f} GB/s)")
    if not a.no_host:
        def host_batch(it):
            dl = torch.utils.data.DataLoader(HostItems(ds, it), batch_size=a.batch, shuffle=False, num_workers=a.workers)
            keep["host"] = tuple(t.cuda() for t in next(iter(dl)))

        host = median_ms(host_batch, max(2, a.steps // 5), 1)
        out.update(host_loader_ms=host[0], host_loader_ms_min_max=host[1:], host_workers=a.workers)
        log(f"host dataset + DataLoader({a.workers} workers) + upload {host[0]:.1f} ms")
    if not a.no_step:
        import contextlib
        import bench_inpainting as C3
        with contextlib.redirect_stdout(sys.stderr):
            tr = C3.build("bf16", a.batch, F, T)
        batch = C3.synth(a.batch, F, T, "cuda")
        step = median_ms(lambda it: tr.train_step(batch), a.steps, a.warmup)
        out.update(c3_step_ms=step[0], c3_step_ms_min_max=step[1:], device_loader_share_of_c3_step=dev[0] / step[0])
        if "host_loader_ms" in out:
            out["host_loader_share_of_c3_step"] = out["host_loader_ms"] / step[0]
        log(f"C3 train step {step[0]:.2f} ms: the device loader is {100 * dev[0] / step[0]:.2f} % of it")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
