#!/usr/bin/env python3
"""Times the spectrogram pictures of the inpainting validator (nppc_audio/spectrogram_png.py, csrc/spec_png.hip,
csrc/png_core.h) from tensors in device memory to PNG bytes in host memory, at the validator's shape:
B = 16 items, K = 5 directions, A = 13 alphas, F = 128, T = 256, a 17-frame gap (a 51-frame context window), every source
pixel 2 x 2: per item 4 + K (1 + A) = 74 individual panels and one 6 x 14 sheet, 1200 files in all.

  (device) save_pc_spectrograms' device call: windows from the mask, render_png (layout, autoscale, render, memset, plan,
           scan, write, finish), one small read, one copy of exactly the encoded bytes
  (split)  HIP events around the entry points of one such call made in its three parts (windows, render, encode)
  (a)      the reference's own way: one matplotlib figure and one savefig per panel plus the sheet, on the host, for ONE item
           (the reference handles one sample at a time); not extrapolated.  "not measured" where matplotlib is missing
  (b)      download the index images and write them with Pillow (mode P, into memory) on a pool of 16 threads
  (c)      download the index images and encode them with the serial host encoder of this project on the same pool
and the encoded size over W * H.  Medians of --runs runs after --warmup warm-ups, with min and max.

    python tools/bench_spec_png.py [--runs 20] [--warmup 5] [--out FILE]
"""
import argparse
import io
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from bench_flac_decode import ROOT, repeat, stats

B, K, F, T, GAP = 16, 5, 128, 256, 17
THREADS = 16


def matplotlib_one_item(planes, alphas, t0, t1, gap):
    """plot_pc_spectrograms' work for one item: a figure, an imshow, a colour bar, two axvlines and a savefig per panel, and
    the (1 + K) x (A + 1) sheet; into memory"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    clean, masked, pred, pcs = planes[0], planes[1], planes[2], planes[3:]
    panels = [(clean, -3, 3), (masked, -3, 3), (pred, -3, 3), (np.abs(clean - pred), 0, 3)]
    for k in range(K):
        panels.append((pcs[k], -3, 3))
        panels += [(pred + a * pcs[k], -3, 3) for a in alphas]
    n = 0
    for data, lo, hi in panels:
        fig, ax = plt.subplots(figsize=(10, 6))
        im = ax.imshow(data[:, t0:t1], origin="lower", aspect="auto", vmin=lo, vmax=hi)
        plt.colorbar(im, ax=ax)
        ax.axvline(x=gap[0] - t0, color="r", linestyle="--", alpha=0.5)
        ax.axvline(x=gap[1] - t0, color="r", linestyle="--", alpha=0.5)
        plt.tight_layout()
        buf = io.BytesIO()
        fig.savefig(buf, format="png")
        plt.close(fig)
        n += buf.tell()
    cols = len(alphas) + 1
    fig, axs = plt.subplots(1 + K, cols, figsize=(3 * cols, 3 * (1 + K)))
    for j, (data, lo, hi) in enumerate(panels[:4] + [panels[0], panels[2]]):
        plt.colorbar(axs[0, j].imshow(data[:, t0:t1], origin="lower", aspect="auto", vmin=lo, vmax=hi), ax=axs[0, j])
    for j in range(6, cols):
        axs[0, j].remove()
    for k in range(K):
        for j in range(cols):
            data, lo, hi = panels[4 + k * cols + j]
            plt.colorbar(axs[k + 1, j].imshow(data[:, t0:t1], origin="lower", aspect="auto", vmin=lo, vmax=hi), ax=axs[k + 1, j])
    plt.tight_layout()
    buf = io.BytesIO()
    fig.savefig(buf, format="png")
    plt.close(fig)
    return n + buf.tell(), len(panels) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true", help="the device path only (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_png_bench.json"))
    a = ap.parse_args()
    from PIL import Image
    from nppc_audio import _hip as H
    from nppc_audio import png
    from nppc_audio import spectrogram_png as SP
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas, pc_spectrogram_sheets
    H.require_gpu()
    alphas = [float(x) for x in default_alphas()]
    g = torch.Generator().manual_seed(7)
    planes = (1.5 * torch.randn(B, 3 + K, F, T, generator=g)).cuda()
    mask = torch.ones(B, T)
    for b in range(B):
        mask[b, 60 + 7 * b:60 + 7 * b + GAP] = 0
    mask = mask.cuda()
    names, sheets = pc_spectrogram_sheets(B, K, alphas, True, 2, 2, 4)
    pal = png.palette("viridis")
    torch.cuda.synchronize()
    res = {"tool": "bench_spec_png", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "host_cpus_used": THREADS, "shape": dict(B=B, K=K, A=len(alphas), F=F, T=T, gap_frames=GAP, sx=2, sy=2, gutter=4),
           "files": len(sheets)}
    files = []

    def device():
        files[:] = SP.render_png(planes, sheets, SP.windows_from_mask(mask), palette=pal, max_frames=3 * GAP)

    res["device_tensors_to_png_bytes_ms"] = stats(repeat(device, a.runs, a.warmup))
    dev_files = list(files)
    idx = SP.render_indices(planes, sheets, SP.windows_from_mask(mask), max_frames=3 * GAP)
    pixels = sum(i.numel() for i in idx)
    res.update(pixels_MB=pixels / 1e6, png_MB=sum(map(len, dev_files)) / 1e6, png_over_pixels=sum(map(len, dev_files)) / pixels,
               largest_image=list(max((tuple(i.shape) for i in idx), key=lambda s: s[0] * s[1])))
    # the three parts of the same work, with events around the entry points
    d = SP._prepare(planes, sheets, SP.windows_from_mask(mask), 3 * GAP)
    work = png.EncodeWork(d["dims"], planes.device)
    H.PROFILE = []
    SP.windows_from_mask(mask)
    H.call("nppc_spec_render", *SP._render_args(d), H.stream())
    H.call("nppc_png_encode", d["pix"], d["pix"].numel(), d["meta"], d["nimg"], *work.args(pal), H.stream())
    torch.cuda.synchronize()
    ev = {}
    for k, e0, e1 in H.PROFILE:
        if k != "nppc_png_bound":
            ev[k] = ev.get(k, 0.0) + e0.elapsed_time(e1)
    H.PROFILE = None
    res["device_entry_point_events_ms"] = ev
    assert work.files() == dev_files, "the three parts and the fused call differ"
    if not a.no_baselines:
        host_idx = []

        def download():
            host_idx[:] = [i.cpu().numpy() for i in SP.render_indices(planes, sheets, SP.windows_from_mask(mask), max_frames=3 * GAP)]

        flat_pal = pal.reshape(-1).tolist()

        def pil_one(arr):
            im = Image.fromarray(arr, mode="P")
            im.putpalette(flat_pal)
            buf = io.BytesIO()
            im.save(buf, format="PNG")
            return buf.getvalue()

        blobs = []

        def pillow_pool():
            download()
            with ThreadPoolExecutor(max_workers=THREADS) as ex:
                blobs[:] = list(ex.map(pil_one, host_idx))

        def host_pool():
            download()
            blobs[:] = png.encode_indexed([torch.from_numpy(x) for x in host_idx], pal, backend="host")

        res["render_download_only_ms"] = stats(repeat(download, a.runs, a.warmup))
        res["render_download_pillow_pool_ms"] = stats(repeat(pillow_pool, a.runs, a.warmup))
        res["pillow_png_MB"] = sum(map(len, blobs)) / 1e6
        assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), x) for f, x in list(zip(dev_files, host_idx))[::97])
        res["render_download_host_encoder_pool_ms"] = stats(repeat(host_pool, max(3, a.runs // 4), 1))
        assert blobs == dev_files, "host and device files differ"
        try:
            import matplotlib  # noqa: F401
            win = SP.windows_from_mask(mask).cpu().tolist()[0]
            x0 = planes[0].cpu().numpy()
            t0 = time.perf_counter()
            nbytes, nfig = matplotlib_one_item(x0, alphas, win[0], win[1], (win[2], win[3]))
            res["matplotlib_one_item_ms"] = (time.perf_counter() - t0) * 1e3
            res["matplotlib_one_item_figures"] = nfig
            res["matplotlib_one_item_MB"] = nbytes / 1e6
        except ImportError:
            res["matplotlib_one_item_ms"] = "not measured (matplotlib is not installed here)"
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
