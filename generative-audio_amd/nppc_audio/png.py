"""Indexed PNG files written on the device (csrc/png_core.h + csrc/spec_png.hip; specification
tests/png_ref.py).

`encode_indexed` turns uint8 index images into PNG files: 8-bit indexed colour, a 256-entry palette, every scanline with the
Up filter, one fixed-Huffman deflate block whose only matches are runs (distance 1).  One stated token rule: the bytes are a
function of the pixels alone, the same from the serial host encoder and from the device (a memset and four launches: plan,
scan, write, finish; one small host read and one copy of exactly the encoded bytes per batch).  Pillow, zlib and every
viewer read the files.  Not built: stored blocks, dynamic Huffman codes, other filters, RGB or 16-bit images.

`palette` gives the 256 x 3 table: entries 0..253 a colour map, 254 the gap marker, 255 the background.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _hip as H

TILE = 4096                  # bytes of filtered stream per workgroup (PNG_TILE of csrc/png_core.h)
MAX_DIM = 16384
MAX_PIXELS = 1 << 26
HOST_THREADS = 16

# matplotlib's viridis at 254 evenly spaced points, rounded to 8 bits (generated once; matplotlib is not imported)
_VIRIDIS = bytes.fromhex(
    "44015444025645045745055946075a46085c460a5d460b5e470d60470e6147106347116447136548146748166848176948186a481a6c481b6d"
    "481c6e481d6f481f70482071482173482374482475482576482677482878482979472a7a472c7a472d7b472e7c472f7d46307e46327e46337f"
    "463480453581453781453882443983443a83443b84433d84433e85423f854240864241864142874144874045884046883f47883f48893e4989"
    "3e4a893e4c8a3d4d8a3d4e8a3c4f8a3c508b3b518b3b528b3a538b3a548c39558c39568c38588c38598c375a8c375b8d365c8d365d8d355e8d"
    "355f8d34608d34618d33628d33638d32648e32658e31668e31678e30698e306a8e2f6b8e2f6c8e2e6d8e2e6e8e2e6f8e2d708e2d718e2c718e"
    "2c728e2c738e2b748e2b758e2a768e2a778e2a788e29798e297a8e297b8e287c8e287d8e277e8e277f8e27808e26818e26828e26828e25838e"
    "25848e25858e24868e24878e23888e23898e238a8d228b8d228c8d228d8d218e8d218f8d21908d21918c20928c20928c20938c1f948c1f958b"
    "1f968b1f978b1f988b1f998a1f9a8a1e9b8a1e9c891e9d891f9e891f9f881fa0881fa1881fa1871fa28720a38620a48621a58521a68522a785"
    "22a88423a98324aa8325ab8225ac8226ad8127ad8128ae8029af7f2ab07f2cb17e2db27d2eb37c2fb47c31b57b32b67a34b67937b87838b977"
    "3aba763bbb753dbc743fbc7340bd7242be7144bf7046c06f48c16e4ac16d4cc26c4ec36b50c46a52c56954c56856c66758c7655ac8645cc863"
    "5ec96260ca6063cb5f65cb5e67cc5c69cd5b6ccd5a6ece5870cf5773d05675d05477d1537ad1517cd2507fd34e81d34d84d44b86d54989d548"
    "8bd6468ed64590d74393d74195d84098d83e9bd93c9dd93ba0da39a2da37a5db36a8db34aadc32addc30b0dd2fb2dd2db5de2bb8de29bade28"
    "bddf26c0df25c2df23c5e021c8e020cae11fcde11dd0e11cd2e21bd5e21ad8e219dae319dde318dfe318e2e418e5e419e7e419eae51aece51b"
    "efe51cf1e51df4e61ef6e620f8e621fbe723fde725")


def palette(name="viridis", marker=(255, 0, 0), background=(255, 255, 255)):
    """256 x 3 uint8: entries 0..253 the colour map ("viridis", matplotlib's default, or "gray"), 254 marker, 255 background"""
    if name == "viridis":
        cmap = np.frombuffer(_VIRIDIS, np.uint8).reshape(254, 3)
    elif name == "gray":
        cmap = np.repeat(np.rint(np.arange(254) * (255.0 / 253.0)).astype(np.uint8)[:, None], 3, axis=1)
    else:
        raise ValueError(f"palette must be 'viridis' or 'gray', got {name!r}")
    out = np.empty((256, 3), np.uint8)
    out[:254], out[254], out[255] = cmap, marker, background
    return out


def _palette(p):
    p = np.ascontiguousarray(np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p))
    if p.dtype != np.uint8 or p.shape != (256, 3):
        raise ValueError("the palette is a 256 x 3 uint8 table")
    return p


def bound(width, height):
    """no file of a width x height image is longer (nppc_png_bound)"""
    n = ctypes.c_long()
    H.call("nppc_png_bound", int(width), int(height), ctypes.byref(n))
    return n.value


def _encode_host(a, pal):
    h, w = a.shape
    cap = bound(w, h)
    out = np.empty(cap, np.uint8)
    n = ctypes.c_long()
    H.call("nppc_png_encode_host", a.ctypes.data, w, h, pal.ctypes.data, out.ctypes.data, cap, ctypes.byref(n))
    return out[:n.value].tobytes()


def tile_tables(pixels):
    """(ttab [ntiles, 2] int32, tfirst [nimg + 1] int32) for images of at most pixels[i] = (W, H): every tile of every stream"""
    tiles = np.array([-(-(h * (w + 1)) // TILE) for w, h in pixels], np.int64)
    tfirst = np.concatenate([[0], np.cumsum(tiles)])
    ttab = np.empty((int(tfirst[-1]), 2), np.int32)
    ttab[:, 0] = np.repeat(np.arange(len(tiles)), tiles)
    ttab[:, 1] = np.arange(len(ttab)) - np.repeat(tfirst[:-1], tiles)
    return ttab, tfirst.astype(np.int32)


class EncodeWork:
    """the device buffers of one nppc_png_encode / nppc_spec_render_png call, for images of at most dims[i] = (W, H)"""

    def __init__(self, dims, dev):
        ttab, tfirst = tile_tables(dims)
        if len(ttab) >= 2 ** 31:
            raise ValueError("png: too many tiles in one batch")
        self.nimg, self.ntiles = len(dims), len(ttab)
        each = {d: bound(*d) for d in set(dims)}                         # the shape query, once per distinct shape
        self.cap = (sum(each[d] for d in dims) + 3) & ~3
        self.ttab, self.tfirst = torch.from_numpy(ttab).to(dev), torch.from_numpy(tfirst).to(dev)
        self.plan = torch.empty(self.ntiles * 4, dtype=torch.int32, device=dev)
        self.toff = torch.empty(self.ntiles, dtype=torch.int64, device=dev)
        self.stats = torch.empty((self.nimg + 1) * 4, dtype=torch.int64, device=dev)
        self.out = torch.empty(self.cap, dtype=torch.uint8, device=dev)

    def args(self, pal):
        return (self.ttab, self.tfirst, self.ntiles, pal.ctypes.data, self.plan, self.toff, self.stats, self.out, self.cap)

    def files(self):
        """the small read (sizes and offsets), then one copy of exactly the encoded bytes"""
        host = self.stats.cpu().numpy().reshape(self.nimg + 1, 4)
        data = self.out[:int(host[self.nimg, 0])].cpu().numpy()
        return [data[int(host[f, 0]):int(host[f, 1])].tobytes() for f in range(self.nimg)]


def _encode_device(flat, dims, pal):
    """flat: uint8 device tensor, the images back to back; dims[i] = (W, H) -> list of bytes"""
    dev = flat.device
    off = np.concatenate([[0], np.cumsum([w * h for w, h in dims])])
    meta = np.zeros((len(dims), 4), np.int64)
    meta[:, 0], meta[:, 1], meta[:, 2] = off[:-1], [w for w, _ in dims], [h for _, h in dims]
    work = EncodeWork(dims, dev)
    with torch.cuda.device(dev):
        H.call("nppc_png_encode", flat, flat.numel(), torch.from_numpy(meta).to(dev), len(dims), *work.args(pal), H.stream())
        return work.files()


def _backend(backend):
    if backend not in ("auto", "hip", "host"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'host', got {backend!r}")
    if backend == "hip":
        H.require_gpu()
    return backend == "hip" or (backend == "auto" and torch.cuda.is_available())


def encode_indexed(images, palette, backend="auto", device="cuda"):
    """uint8 index images -> PNG files: a list of [H, W] tensors (host or device), or one [N, H, W] tensor -> a list of bytes.
    backend "host" runs the serial encoder on a pool of 16 threads, "hip" the device kernels (the whole ragged batch in one
    call) and "auto" the device when there is one; both give the same bytes.  ValueError, before anything is launched, for
    an empty image, one wider or higher than 16384 or of more than 2^26 pixels, or a palette that is not 256 x 3."""
    pal = _palette(palette)
    if isinstance(images, torch.Tensor):
        if images.dim() != 3:
            raise ValueError("encode_indexed takes a list of [H, W] tensors or one [N, H, W] tensor")
        images = list(images)
    images = list(images)
    for t in images:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2:
            raise ValueError("encode_indexed takes uint8 tensors [H, W]")
        h, w = t.shape
        if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM and h * w <= MAX_PIXELS):
            raise ValueError(f"encode_indexed: an image of {w} x {h} pixels (1..{MAX_DIM} each way, at most 2^26 pixels)")
    on_device = _backend(backend)
    if not images:
        return []
    if not on_device:
        arrays = [np.ascontiguousarray(t.cpu().numpy()) for t in images]
        with ThreadPoolExecutor(max_workers=max(1, min(HOST_THREADS, os.cpu_count() or 1, len(arrays)))) as ex:
            return list(ex.map(lambda a: _encode_host(a, pal), arrays))      # ctypes releases the GIL
    images = [t if t.is_cuda else t.to(device) for t in images]
    flat = images[0].contiguous().view(-1) if len(images) == 1 else torch.cat([t.reshape(-1) for t in images])
    return _encode_device(flat, [(t.shape[1], t.shape[0]) for t in images], pal)


def write_files(paths, blobs):
    """blobs (what encode_indexed returns) -> files; directories are made as needed"""
    paths = [str(p) for p in paths]
    if len(paths) != len(blobs):
        raise ValueError(f"{len(paths)} paths for {len(blobs)} files")
    for p, b in zip(paths, blobs):
        d = os.path.dirname(p)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(p, "wb") as f:
            f.write(b)
