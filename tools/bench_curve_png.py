#!/usr/bin/env python3
"""Times the pitch figures of the inpainting validator (nppc_audio/curve_png.py, csrc/curve_png.hip, csrc/curve_core.h;
DESIGN.md section 8m) from the contours in device memory to PNG bytes in host memory, at the validator's shape: B = 16 items,
K = 5 directions, A = 13 alphas, 4 s clips (126 pitch frames): 16 x 66 contours, per item K individual figures and the
stacked one, 96 files in all, every frame 8 pixels wide and every panel 240 pixels high.

  (device) save_pc_pitch_plots' device call: curve_png.render_png (layout, autoscale, render, memset, plan, scan, write,
           finish), one small read, one copy of exactly the encoded bytes
  (split)  HIP events around nppc_curve_render and nppc_png_encode of one such call made in its parts, and the wall time of
           the read and the copy behind them
  (host)   the same files from backend="host": download the contours, the serial renderer, the serial encoder on 16 threads
  (a)      download the contours and draw the same sheets with Pillow's ImageDraw (lines, box, grid, labels in its default
           font, legend swatches) and save (mode P, into memory) on a pool of 16 threads
  (b)      the reference's own way for ONE item: plot_pitch_comparison's matplotlib figures and savefig, on the host; not
           extrapolated.  "not measured" where matplotlib is missing
Medians of --runs runs after --warmup warm-ups, with min and max.

    python tools/bench_curve_png.py [--runs 20] [--warmup 5] [--out FILE]
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

B, K, T = 16, 5, 126
SX, PH = 8, 240
THREADS = 16


def contours(A):
    """speech-like contours: a slow melody, a bump per (direction, alpha) and unvoiced stretches"""
    rng = np.random.default_rng(5)
    t = np.arange(T)
    clean = 160.0 + 50.0 * np.sin(t[None, :] / 11.0 + rng.uniform(0, 6, (B, 1)))
    bump = np.exp(-((t[None, None, None, :] - rng.uniform(30, 90, (B, K, 1, 1))) / 12.0) ** 2)
    f0 = clean[:, None, None, :] + (np.arange(A)[None, None, :, None] - A // 2) * rng.uniform(2, 6, (B, K, 1, 1)) * bump
    f0[rng.random(f0.shape) < 0.03] = np.nan
    clean[:, 100:108] = np.nan
    f0[..., 100:108] = np.nan
    return {"f0_clean": torch.from_numpy(clean.astype(np.float32)).cuda(), "f0": torch.from_numpy(f0.astype(np.float32)).cuda()}


def pillow_sheet(values, sheet, window, pal_flat, pal):
    """the sheet by ImageDraw at the renderer's own layout: box, grid, labels, legend, polylines broken at NaN"""
    from PIL import Image, ImageDraw
    import curve_ref as R
    t0, t1, m0, m1 = window
    L = R.layout(sheet, t1 - t0, values.shape[1])
    im = Image.new("P", (L["W"], L["H"]), 255)
    im.putpalette(pal_flat)
    d = ImageDraw.Draw(im)
    for p, top in zip(sheet.panels, L["tops"]):
        x0, y0 = L["ML"], top + 4
        x1, y1 = x0 + L["PW"] + 1, y0 + PH + 1
        ypix = lambda v: y1 - 1 - (v - p.ymin) * PH / (p.ymax - p.ymin)
        for v in p.yticks:
            d.line([(x0, ypix(v)), (x1, ypix(v))], fill=251)
            d.text((2, ypix(v) - 5), R.label(v), fill=250)
        for t in range(0, values.shape[1], p.xtick_every):
            x = x0 + 1 + (t - t0) * sheet.sx + sheet.sx // 2
            d.line([(x, y0), (x, y1)], fill=251)
            d.text((x - 8, y1 + 2), R.label(t * p.x_unit), fill=250)
        for m in (m0, m1):
            if p.markers and t0 <= m < t1:
                x = x0 + 1 + (m - t0) * sheet.sx + sheet.sx // 2
                for y in range(y0 + 1, y1, 8):
                    d.line([(x, y), (x, min(y + 3, y1 - 1))], fill=254)
        for c in p.curves:
            run = []
            for t in range(t0, t1):
                v = values[c.row, t]
                if np.isnan(v):
                    if run:
                        d.line(run, fill=c.colour, width=c.width) if len(run) > 1 else d.point(run, fill=c.colour)
                    run = []
                else:
                    run.append((x0 + 1 + (t - t0) * sheet.sx + sheet.sx // 2, float(np.clip(ypix(v), y0 + 1, y1 - 1))))
            if run:
                d.line(run, fill=c.colour, width=c.width) if len(run) > 1 else d.point(run, fill=c.colour)
        d.rectangle([x0, y0, x1, y1], outline=250)
        for n, (colour, text) in enumerate(p.legend):
            d.rectangle([x1 + 3, y0 + 1 + 8 * n, x1 + 9, y0 + 7 + 8 * n], fill=colour)
            d.text((x1 + 11, y0 - 2 + 8 * n), text, fill=250)
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def matplotlib_one_item(f0_clean, f0, alphas):
    """plot_pitch_comparison's figures for one item: the stacked figure and one per direction; into memory"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    times = np.arange(T) * 512 / 16000
    colors = plt.cm.viridis(np.linspace(0, 1, len(alphas)))
    fig, axes = plt.subplots(K + 1, 1, figsize=(15, 4 * (K + 1)))
    axes[0].plot(times, f0_clean, color="black", label="Clean", linewidth=2)
    axes[0].set_ylim(80, 400), axes[0].grid(True), axes[0].legend()
    n = 0
    for k in range(K):
        ax = axes[k + 1]
        ax.plot(times, f0_clean, color="black", label="Clean", linewidth=2)
        for a, alpha in enumerate(alphas):
            ax.plot(times, f0[k, a], color=colors[a], label=f"a={alpha:.1f}", alpha=0.7)
        ax.set_ylim(80, 400), ax.grid(True), ax.legend(bbox_to_anchor=(1.05, 1), loc="upper left")
        fig_pc, ax_pc = plt.subplots(figsize=(15, 4))
        ax_pc.plot(times, f0_clean, color="black", label="Clean", linewidth=2)
        for a, alpha in enumerate(alphas):
            ax_pc.plot(times, f0[k, a], color=colors[a], label=f"a={alpha:.1f}" if a % 2 == 0 else "_nolegend_", alpha=0.7)
        ax_pc.set_ylim(80, 400), ax_pc.grid(True), ax_pc.legend(bbox_to_anchor=(1.02, 1), loc="upper left")
        buf = io.BytesIO()
        fig_pc.savefig(buf, format="png", bbox_inches="tight")
        plt.close(fig_pc)
        n += buf.tell()
    plt.tight_layout()
    buf = io.BytesIO()
    fig.savefig(buf, format="png")
    plt.close(fig)
    return n + buf.tell(), K + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curve_png_bench.json"))
    a = ap.parse_args()
    from nppc_audio import _hip as H
    from nppc_audio import curve_png as CP
    from nppc_audio import png
    from nppc_audio.inpainting.validator.validator_nppc_model import default_alphas
    H.require_gpu()
    alphas = [float(x) for x in default_alphas()]
    A = len(alphas)
    pitch = contours(A)
    win = torch.tensor([[0, T, 40 + b, 60 + b] for b in range(B)], dtype=torch.int32).cuda()
    names, sheets = CP.pitch_sheets(B, K, alphas, T, 512 / 16000, sx=SX, plot_height=PH)
    pal = CP.plot_palette()
    torch.cuda.synchronize()
    res = {"tool": "bench_curve_png", "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "host_cpus_used": THREADS, "shape": dict(B=B, K=K, A=A, T=T, contours=B * (1 + K * A), sx=SX, plot_height=PH),
           "files": len(sheets)}
    files = []

    def device():
        files[:] = CP.render_png(CP.stack_contours(pitch), sheets, win, palette=pal, backend="hip")

    res["device_contours_to_png_bytes_ms"] = stats(repeat(device, a.runs, a.warmup))
    dev_files = list(files)
    idx = CP.render_indices(CP.stack_contours(pitch), sheets, win)
    pixels = sum(i.numel() for i in idx)
    res.update(pixels_MB=pixels / 1e6, png_MB=sum(map(len, dev_files)) / 1e6, png_over_pixels=sum(map(len, dev_files)) / pixels,
               image_sizes=sorted({(int(i.shape[1]), int(i.shape[0])) for i in idx}))
    # the parts of the same work: events around the two entry points, then the read and the copy
    render_ms, encode_ms, copy_ms = [], [], []
    for _ in range(a.warmup + a.runs):
        values = CP.stack_contours(pitch)
        d = CP._prepare(values, sheets, win, None)
        t, args = CP._device_args(d)
        work = png.EncodeWork(d["dims"], values.device)
        H.PROFILE = []
        H.call("nppc_curve_render", *args, H.stream())
        H.call("nppc_png_encode", t["pix"], t["pix"].numel(), t["meta"], d["nimg"], *work.args(pal), H.stream())
        torch.cuda.synchronize()
        ev = {k: e0.elapsed_time(e1) for k, e0, e1 in H.PROFILE}
        H.PROFILE = None
        t0 = time.perf_counter()
        parts = work.files()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
        render_ms.append(ev["nppc_curve_render"]), encode_ms.append(ev["nppc_png_encode"])
    assert parts == dev_files, "the parts and the fused call differ"
    res["split_ms"] = {"render": stats(render_ms[a.warmup:]), "encode": stats(encode_ms[a.warmup:]), "read_and_copy": stats(copy_ms[a.warmup:])}
    res["split_note"] = "the rest of device_contours_to_png_bytes_ms is host work: tables, the shape queries, uploads, allocation"

    def host():
        files[:] = CP.render_png(CP.stack_contours(pitch), sheets, win, palette=pal, backend="host")

    res["host_backend_ms"] = stats(repeat(host, a.runs, a.warmup))
    assert files == dev_files, "host and device files differ"
    flat_pal = pal.reshape(-1).tolist()
    windows = win.cpu().tolist()
    blobs = []

    def pillow_pool():
        values = CP.stack_contours(pitch).cpu().numpy()
        with ThreadPoolExecutor(max_workers=THREADS) as ex:
            blobs[:] = list(ex.map(lambda s: pillow_sheet(values, s, windows[s.item], flat_pal, pal), sheets))

    res["download_pillow_imagedraw_pool_ms"] = stats(repeat(pillow_pool, a.runs, a.warmup))
    res["pillow_png_MB"] = sum(map(len, blobs)) / 1e6
    try:
        import matplotlib  # noqa: F401
        c0, f0 = pitch["f0_clean"][0].cpu().numpy(), pitch["f0"][0].cpu().numpy()
        t0 = time.perf_counter()
        nbytes, nfig = matplotlib_one_item(c0, f0, alphas)
        res["matplotlib_one_item_ms"] = (time.perf_counter() - t0) * 1e3
        res["matplotlib_one_item_figures"] = nfig
        res["matplotlib_one_item_MB"] = nbytes / 1e6
    except ImportError:
        res["matplotlib_one_item_ms"] = "not measured (matplotlib is not installed here)"
    med = lambda k: res[k]["median"]
    res["auto_backend"] = "hip" if med("device_contours_to_png_bytes_ms") < med("host_backend_ms") else "host"
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
