"""fp64 numpy restatement of the posterior samples of a whole recording (item 4 of csrc/enhance_core.h, csrc/enhance_post.hip,
DESIGN.md section 7j), on top of tests/posterior_ref.py (the sample of one chunk) and tests/enhance_ref.py (plan, table).

A recording of L samples in n chunks of C at a hop of H = C / 2; chunk c has planes pred [n,2,F,T], w [n,K,2,F,T], noisy
re / im [n,F,T] and len[c] samples (C, the last one L - (n - 1) H).  perm, sign [n,K] are the tables of the chain, z [S,K,2]
one set of coefficients per recording, indexed by slot.  Sample s:
    direction k of chunk c:  sign[c][k] w[c][perm[c][k]]                 (slot order; the negation is exact)
    y_{c,s} = posterior_ref.sample_waveforms of chunk c with these directions and z_s, ragged at len[c]
    out[m]:  cur = min(m // H, n - 1), i = m - cur H;
             cur >= 1 and i < H:  y_{cur-1,s}[i + H] (1 - w[i]) + y_{cur,s}[i] w[i];  otherwise y_{cur,s}[i]
with w the fp32 table of enhance_ref.table, used at its fp32 values."""
import numpy as np

import enhance_ref as ER
import posterior_ref as PR

TILE = 8                     # NPPC_POST_TILE
FR = 4                       # ISTFT_FR: a workgroup owns FR * hop output samples


def chunk_lengths(n, C, last):
    return [C] * (n - 1) + [int(last)]


def slot_directions(w, perm, sign):
    """w [n,K,2,F,T], perm / sign [n,K] -> the directions in slot order, signed, in w's dtype (exact)"""
    w, perm, sign = np.asarray(w), np.asarray(perm), np.asarray(sign)
    n = w.shape[0]
    s = np.where(sign < 0, -1, 1).astype(w.dtype)
    return s[:, :, None, None, None] * w[np.arange(n)[:, None], perm]


def chunk_waveforms(pred, w, re, im, z, perm, sign, last, C, nfft, hop, domain="compressed"):
    """-> y [n,S,W] fp64, W the padded chunk width (C, or `last` for a single chunk), zeros past a chunk's length"""
    n = np.asarray(pred).shape[0]
    z = np.asarray(z)
    W = C if n > 1 else int(last)
    zz = np.broadcast_to(z[None], (n,) + z.shape)
    return PR.sample_waveforms(pred, slot_directions(w, perm, sign), re, im, zz, W, nfft, hop, lengths=chunk_lengths(n, C, last),
                               domain=domain)["samples"]


def crossfade(y, last, C):
    """y [n,S,W] fp64 -> [S,L] fp64"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    H = C // 2
    L = (n - 1) * H + int(last)
    w = ER.table(C).astype(np.float64)
    m = np.arange(L)
    cur = np.minimum(m // H, n - 1)
    i = m - cur * H
    blend = (cur >= 1) & (i < H)
    prev, ip, wi = np.where(blend, cur - 1, 0), np.where(blend, i + H, 0), w[np.where(blend, i, 0)]
    yc, yp = y[cur, :, i].T, y[prev, :, ip].T                     # [S,L]
    return np.where(blend, yp * (1.0 - wi) + yc * wi, yc)


def sample_recording(pred, w, re, im, z, perm, sign, last, C, nfft, hop, domain="compressed"):
    """-> samples [S,L] fp64"""
    return crossfade(chunk_waveforms(pred, w, re, im, z, perm, sign, last, C, nfft, hop, domain), last, C)


def shape_ok(n, S, K, C, L, T, nfft, hop, stats=0):
    """what nppc_enh_post_sample_shape accepts"""
    if nfft not in (64, 128, 256, 512) or hop <= 0 or nfft % hop or not 2 <= nfft // hop <= 8:
        return False
    if n < 1 or not 0 <= K <= 16 or C < 2 or C % 2 or (C // 2) % (FR * hop) or S < 1 or T <= 0 or stats not in (0, 1):
        return False
    if not 0 < L - (n - 1) * (C // 2) <= C:
        return False
    return not stats or 2 <= S <= 4096


def tiling(S, L, hop, stats=0, tile=TILE, fill=1024, max_stat_tiles=32):
    """(tiles, samples per tile, workspace bytes): the restatement of nppc_enh_post_sample_shape"""
    cdiv = lambda a, b: -(-a // b)                                 # noqa: E731
    nblk = cdiv(L, FR * hop)
    nt = cdiv(S, tile)
    if stats:
        nt = min(nt, min(max(cdiv(fill, nblk), 1), max_stat_tiles))
    per = cdiv(S, nt)
    nt = cdiv(S, per)
    return nt, per, 16 * nt * L if stats else 0


def one_pass_stats(y, tiles, per):
    """the statistics as the launch forms them, operation for operation: per sample tile the fp64 sums of y and y^2 over its
    samples in order, the tiles folded in order, mean = s1 / S, std = sqrt(max(0, (s2 - s1 s1 / S) / (S - 1))), each rounded
    to fp32 once.  y [S,L] fp32 -> (mean, std) fp32"""
    y = np.asarray(y, np.float64)
    S, L = y.shape
    s1, s2 = np.zeros(L), np.zeros(L)
    for t in range(tiles):
        p1, p2 = np.zeros(L), np.zeros(L)
        for s in range(t * per, min(S, (t + 1) * per)):
            p1 = p1 + y[s]
            p2 = p2 + y[s] * y[s]
        s1, s2 = s1 + p1, s2 + p2
    var = (s2 - s1 * s1 / S) / (S - 1)
    return (s1 / S).astype(np.float32), np.sqrt(np.where(var > 0.0, var, 0.0)).astype(np.float32)


def case(n, S, K, C, last, nfft, hop, seed, zscale=1.0, complex_coeffs=False):
    """posterior_ref.case with the chunks as the batch and one set of coefficients -> (pred, w, re, im, z [S,K,2])"""
    W = C if n > 1 else int(last)
    pred, w, re, im, z = PR.case(n, S, K, nfft, hop, W, seed, zscale=zscale, complex_coeffs=complex_coeffs)
    return pred, w, re, im, np.ascontiguousarray(z[0])


def moved_tables(perm, sign, perms, signs):
    """the tables of the same physical directions after enhance_ref.apply_signed(., perms, signs) moved the raw ones:
    slot s of chunk c finds its direction at the k with perms[c][k] == perm[c][s], under the sign signs[c][k] sign[c][s]"""
    inv = np.argsort(perms, axis=1)
    where = np.take_along_axis(inv, np.asarray(perm, np.int64), axis=1)
    return where.astype(np.int32), (np.asarray(sign) * np.take_along_axis(signs, where, axis=1)).astype(np.int32)
