"""fp64 NumPy restatement of the ragged-gap MC-dropout + PCA baseline (csrc/mc_pca_ragged.hip, csrc/mc_pca.hip): the
yardstick of tests/test_mc_ragged_cpu.py and tests/test_mc_ragged_gpu.py.  Straight loops over the items, no chunking."""
import numpy as np


def gap_index(mask):
    """mask [B, ...] (0 = gap) -> (idx [B, Nmax] int32: row-major positions of the gap elements, -1 after them; counts [B])"""
    m = np.asarray(mask).reshape(len(mask), -1)
    pos = [np.flatnonzero(row == 0) for row in m]
    counts = np.array([len(p) for p in pos], dtype=np.int32)
    idx = np.full((len(m), int(counts.max())), -1, dtype=np.int32)
    for b, p in enumerate(pos):
        idx[b, :len(p)] = p
    return idx, counts


def gather(values, idx):
    """values [B, ...] -> [B, Nmax]: values through idx, 0 at padded positions"""
    v = np.asarray(values).reshape(len(idx), -1)
    out = np.zeros(idx.shape, dtype=v.dtype)
    for b in range(len(idx)):
        keep = idx[b] >= 0
        out[b, keep] = v[b, idx[b, keep]]
    return out


def scatter(values, idx, N):
    """values [B, Nmax] or [B, n, Nmax] -> zeros [B, N] / [B, n, N] with the gap elements filled through idx"""
    v = np.asarray(values)
    out = np.zeros(v.shape[:-1] + (N,), dtype=v.dtype)
    for b in range(len(idx)):
        keep = idx[b] >= 0
        out[b][..., idx[b, keep]] = v[b][..., keep]
    return out


def pca_item(x, n_components):
    """x [K, D] fp32, one item's MC samples -> (components [n, D], scaled [n, D], weights [n], mean [D] fp32, singular [n])
    in fp64.  As compute_pca_batch: the mean is rounded to fp32 and subtracted in fp32 (scikit-learn centres in the input
    dtype); the singular pairs come from np.linalg.eigh of the centred K x K Gram; the largest-magnitude entry of every
    component is positive, the lowest index among equals."""
    x = np.asarray(x, dtype=np.float32)
    K, D = x.shape
    n = min(int(n_components), K)
    mean = (x.astype(np.float64).sum(axis=0) / K).astype(np.float32)
    xc = (x - mean).astype(np.float64)                               # fp32 subtraction, then exact widening
    lam, U = np.linalg.eigh(xc @ xc.T)
    order = np.argsort(lam)[::-1][:n]
    s = np.sqrt(np.maximum(lam[order], 0.0))
    comps = np.zeros((n, D))
    for i in range(n):
        if s[i] > 0:
            comps[i] = U[:, order[i]] @ xc / s[i]
        j = int(np.argmax(np.abs(comps[i])))                         # first index on ties
        if comps[i, j] < 0:
            comps[i] = -comps[i]
    return comps, comps * s[:, None], s / s.sum(), mean, s


def pca_ragged(stack, counts, n_components):
    """stack [K, B, Nmax], item b owns its first counts[b] elements -> compute_pca_ragged's 5-tuple, padded with zeros"""
    stack = np.asarray(stack, dtype=np.float32)
    K, B, Nmax = stack.shape
    n = min(int(n_components), K)
    comps, scaled = np.zeros((B, n, Nmax)), np.zeros((B, n, Nmax))
    weights, svals, mean = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, Nmax), dtype=np.float32)
    for b in range(B):
        c = int(counts[b])
        comps[b, :, :c], scaled[b, :, :c], weights[b], mean[b, :c], svals[b] = pca_item(stack[:, b, :c], n)
    return comps, scaled, weights, mean, svals


def gap_frames(start, length, gap=2048, win=255, hop=128):
    """AudioInpaintingDataset.time_to_spec_mask (centred) for a gap of `gap` samples at `start` in a clip of `length`
    samples: the number of zeroed frames.  Frame t of the 1 + length // hop frames covers samples
    [t hop - win // 2, t hop - win // 2 + win) clamped to the clip and is zeroed iff it holds a gap sample."""
    zeroed = 0
    for t in range(1 + length // hop):
        lo = max(t * hop - win // 2, 0)
        hi = min(t * hop - win // 2 + win, length)
        if hi <= lo or (lo < start + gap and hi > start):
            zeroed += 1
    return zeroed


def gap_frames_closed_form(start, win=255, hop=128):
    """18 + [r >= 3] - [r > 0], r = (start - 127) mod 128: the count while every touched frame exists (win 255, hop 128,
    gap 2048)"""
    r = (start - win // 2) % hop
    return 18 + int(r >= 3) - int(r > 0)
