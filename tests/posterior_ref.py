"""fp64 numpy restatement of the posterior sampler's rule (csrc/posterior.hip).

pred [B,2,F,T] compressed cIRM, w [B,K,2,F,T], noisy re / im [B,F,T], z [B,S,K,2] (real, imaginary):
    compressed:    M = D(pred + sum_k z_k w_k)        (complex z w; D on the real and on the imaginary part)
    decompressed:  M = D(pred) + sum_k z_k D(w_k)
    D(m) = -10 log((10 - c) / (10 + c)),  c = clip(m, -9.9, 9.9) with 9.9 the fp32 constant
    X = M * noisy (true complex product); y = centred inverse STFT, periodic hann, of X
Ragged: item b uses its first 1 + L_b // hop frames and is 0 in samples L_b .. length - 1."""
import numpy as np

CLAMP = np.float64(np.float32(9.9))


def decompress(m):
    c = np.clip(np.asarray(m, np.float64), -CLAMP, CLAMP)
    return -10.0 * np.log((10.0 - c) / (10.0 + c))


def masks(pred, w, z, domain="compressed"):
    """-> (Mr, Mi) [B,S,F,T] in fp64, k ascending"""
    pred, w, z = (np.asarray(a, np.float64) for a in (pred, w, z))
    B, S, K = z.shape[:3]
    if domain == "compressed":
        mr = np.repeat(pred[:, None, 0], S, axis=1)
        mi = np.repeat(pred[:, None, 1], S, axis=1)
        wr, wi = w[:, :, 0], w[:, :, 1]
    elif domain == "decompressed":
        mr = np.repeat(decompress(pred[:, None, 0]), S, axis=1)
        mi = np.repeat(decompress(pred[:, None, 1]), S, axis=1)
        wr, wi = decompress(w[:, :, 0]), decompress(w[:, :, 1])
    else:
        raise ValueError(domain)
    for k in range(K):
        zr, zi = z[:, :, k, 0, None, None], z[:, :, k, 1, None, None]
        a, c = wr[:, None, k], wi[:, None, k]
        mr = mr + (zr * a - zi * c)
        mi = mi + (zr * c + zi * a)
    if domain == "compressed":
        mr, mi = decompress(mr), decompress(mi)
    return mr, mi


def spectra(pred, w, re, im, z, domain="compressed"):
    """the sampled spectra (xr, xi) [B,S,F,T]"""
    mr, mi = masks(pred, w, z, domain)
    a, c = np.asarray(re, np.float64)[:, None], np.asarray(im, np.float64)[:, None]
    return mr * a - mi * c, mi * a + mr * c


def istft(xr, xi, nfft, hop, length):
    """[F,Tb] -> [length]: irfft of every frame (imaginary part of DC and Nyquist ignored), window, overlap-add, division
    by the window envelope of these frames (0 where it is below 1e-11)"""
    F, Tb = xr.shape
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)
    frames = np.fft.irfft((xr + 1j * xi).T, n=nfft, axis=1)
    num = np.zeros(nfft + hop * (Tb - 1))
    den = np.zeros_like(num)
    for t in range(Tb):
        num[t * hop:t * hop + nfft] += win * frames[t]
        den[t * hop:t * hop + nfft] += win * win
    num, den = num[nfft // 2:nfft // 2 + length], den[nfft // 2:nfft // 2 + length]
    y = np.zeros(length)
    ok = den > 1e-11
    y[:len(num)][ok] = num[ok] / den[ok]
    return y


def sample_waveforms(pred, w, re, im, z, length, nfft, hop, lengths=None, domain="compressed"):
    """-> dict: samples [B,S,length], mag [B,S,F,T] (|X_s|, 0 in frames past an item's end), all fp64"""
    xr, xi = spectra(pred, w, re, im, z, domain)
    B, S, F, T = xr.shape
    out = np.zeros((B, S, length))
    mag = np.zeros((B, S, F, T))
    for b in range(B):
        Lb = length if lengths is None else int(lengths[b])
        Tb = min(1 + Lb // hop, T)
        mag[b, :, :, :Tb] = np.sqrt(xr[b, :, :, :Tb] ** 2 + xi[b, :, :, :Tb] ** 2)
        for s in range(S):
            out[b, s, :Lb] = istft(xr[b, s, :, :Tb], xi[b, s, :, :Tb], nfft, hop, Lb)
    return dict(samples=out, mag=mag)


def stats(x, axis=1):
    """two-pass mean and unbiased standard deviation over `axis`, fp64"""
    x = np.asarray(x, np.float64)
    m = x.mean(axis=axis)
    return m, np.sqrt(((x - np.expand_dims(m, axis)) ** 2).sum(axis=axis) / (x.shape[axis] - 1))


def tiling(B, S, T, nfft, hop, length, stats=0, tile=8, fill=1024, max_stat_tiles=32):
    """(tiles, samples per tile, workspace bytes): the restatement of nppc_post_sample_shape"""
    cdiv = lambda a, b: -(-a // b)
    nblk = max(cdiv(length + nfft // 2, 4 * hop), cdiv(T, 4))
    n = cdiv(S, tile)
    if stats:
        n = min(n, min(max(cdiv(fill, B * nblk), 1), max_stat_tiles))
    per = cdiv(S, n)
    n = cdiv(S, per)
    F = nfft // 2 + 1
    return n, per, 16 * n * B * ((length if stats & 1 else 0) + (F * T if stats & 2 else 0))


def case(B, S, K, nfft, hop, length, seed, zscale=1.0, complex_coeffs=False):
    """the inputs of the tests: pred uniform in [-3, 3], w at scale 0.5, noisy planes normal, z normal times zscale"""
    rng = np.random.default_rng(seed)
    F, T = nfft // 2 + 1, 1 + length // hop
    pred = rng.uniform(-3, 3, (B, 2, F, T)).astype(np.float32)
    w = (0.5 * rng.standard_normal((B, K, 2, F, T))).astype(np.float32)
    re = rng.standard_normal((B, F, T)).astype(np.float32)
    im = rng.standard_normal((B, F, T)).astype(np.float32)
    z = np.zeros((B, S, K, 2), np.float32)
    z[..., 0] = zscale * rng.standard_normal((B, S, K))
    if complex_coeffs:
        z[..., 1] = zscale * rng.standard_normal((B, S, K))
    return pred, w, re, im, z
