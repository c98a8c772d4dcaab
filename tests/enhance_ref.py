"""Numpy restatement of whole-recording enhancement's device steps (csrc/enhance_core.h) and the
constructed inputs the tests share.  Nothing here imports the package."""
import numpy as np

F32 = np.float32


def plan(L, C):
    """[(start, length)]"""
    H = C // 2
    if L <= C:
        return [(0, L)]
    n = -(-(L - C) // H) + 1
    return [(c * H, min(C, L - c * H)) for c in range(n)]


def table(C):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(C // 2, dtype=np.float64) / C)).astype(F32)


def gram(pcs):
    """pcs [n, K, C] fp32 -> (G [n-1, K, K], na [n-1, K], nb [n-1, K], absG [n-1, K, K] = sum |a b|), fp64"""
    p = np.asarray(pcs, np.float64)
    n, K, C = p.shape
    H = C // 2
    a, b = p[:-1, :, H:], p[1:, :, :H]
    G = np.einsum("cji,cki->cjk", a, b)
    absG = np.einsum("cji,cki->cjk", np.abs(a), np.abs(b))
    return G, (a * a).sum(-1), (b * b).sum(-1), absG


def cosines(G, na, nb):
    d = na[:, :, None] * nb[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0.0, 0.0, G / np.sqrt(d))


def chain(pcs, match="greedy"):
    """-> perm [n, K] int32, sign [n, K] int32, continuity [n-1, K] fp64, gap: the smallest distance between a chosen
    |cosine| and the best one it was chosen over (inf when there never was a choice)"""
    n, K, _ = pcs.shape
    G, na, nb, _ = gram(pcs)
    cos = cosines(G, na, nb)
    perm = np.zeros((n, K), np.int32)
    sign = np.ones((n, K), np.int32)
    cont = np.zeros((n - 1, K))
    perm[0] = np.arange(K)
    gap = np.inf
    for c in range(1, n):
        taken = []
        for s in range(K):
            j = perm[c - 1, s]
            if match == "sign":
                k = j
            else:
                free = [k for k in range(K) if k not in taken]
                mags = [abs(cos[c - 1, j, k]) for k in free]
                k = free[int(np.argmax(mags))]                    # argmax: the first of equal values, i.e. the lowest k
                if len(free) > 1:
                    top = sorted(mags)
                    gap = min(gap, top[-1] - top[-2])
            taken.append(k)
            perm[c, s] = k
            sign[c, s] = sign[c - 1, s] * (1 if G[c - 1, j, k] >= 0 else -1)
            cont[c - 1, s] = abs(cos[c - 1, j, k])
    return perm, sign, cont, gap


def splice(enh, pcs, last_length, alphas, perm, sign):
    """enh [n, C], pcs [n, K, C] fp32 -> [1 + K A, L] fp32, every operation rounded to fp32 on its own"""
    enh = np.asarray(enh, F32)
    n, C = enh.shape
    H = C // 2
    L = (n - 1) * H + last_length
    alphas = np.zeros(0, F32) if alphas is None else np.asarray(alphas, F32).reshape(-1)
    A = alphas.size
    K = 0 if A == 0 or pcs is None else pcs.shape[1]
    w = table(C)
    m = np.arange(L)
    cur = np.minimum(m // H, n - 1)
    i = m - cur * H
    blend = (cur >= 1) & (i < H)
    prev = np.where(blend, cur - 1, 0)
    ip = np.where(blend, i + H, 0)
    wi = w[np.where(blend, i, 0)]
    out = np.empty((1 + K * A, L), F32)

    def mix(yc, yp):
        both = (yp * (F32(1) - wi)).astype(F32) + (yc * wi).astype(F32)
        return np.where(blend, both.astype(F32), yc).astype(F32)

    out[0] = mix(enh[cur, i], enh[prev, ip])
    for s in range(K):
        pc = np.asarray(pcs, F32)[cur, perm[cur, s], i]
        pp = np.asarray(pcs, F32)[prev, perm[prev, s], ip]
        for a in range(A):
            ac = (alphas[a] * sign[cur, s].astype(F32)).astype(F32)
            ap = (alphas[a] * sign[prev, s].astype(F32)).astype(F32)
            yc = (enh[cur, i] + (ac * pc).astype(F32)).astype(F32)
            yp = (enh[prev, ip] + (ap * pp).astype(F32)).astype(F32)
            out[1 + s * A + a] = mix(yc, yp)
    return out


def enhance(enh, pcs, last_length, alphas, match="greedy"):
    perm, sign, cont, _ = chain(np.asarray(pcs, F32), match)
    return splice(enh, pcs, last_length, alphas, perm, sign), perm, sign, cont


# ---- constructed inputs --------------------------------------------------------------------------------------------------
CASES = [(1, 16, 3), (3, 64, 4), (5, 18, 3), (8, 1024, 5), (16, 512, 3)]        # (K, C, n)
# seed of `directions` per case: the first at which chain() recovers the truth and the smallest gap between a chosen
# |cosine| and the runner-up is 0.33 or more (found with this file alone; 0.67, 0.35, 0.88, 0.84 for the cases with K > 1).
# The tests assert a gap of 0.1 on their own inputs before they compare anything, so a near-tie cannot hide a wrong kernel.
SEEDS = {(1, 16, 3): 0, (3, 64, 4): 0, (5, 18, 3): 2, (8, 1024, 5): 0, (16, 512, 3): 0}


def signed_permutations(rng, n, K, first_identity=True):
    perms = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int64)
    signs = rng.choice([-1, 1], size=(n, K)).astype(np.int64)
    if first_identity:
        perms[0], signs[0] = np.arange(K), 1
    return perms, signs


def apply_signed(pcs, perms, signs):
    """direction k of chunk c becomes signs[c, k] * pcs[c, perms[c, k]]"""
    n = pcs.shape[0]
    return (signs[:, :, None] * pcs[np.arange(n)[:, None], perms]).astype(F32)


def directions(K, C, n, seed, noise=0.05):
    """K base signals over the whole recording, cut into n chunks; per chunk a random signed permutation (the identity for
    chunk 0), amplitudes 1 + 0.1 k, added noise -> (enh [n, C], pcs [n, K, C], truth_perm [n, K], truth_sign [n, K]):
    slot s of the aligned result is base s, so perm[c][s] = the place base s took in chunk c and sign its sign there"""
    rng = np.random.default_rng(seed)
    H = C // 2
    L = (n - 1) * H + C
    base = rng.standard_normal((K, L))
    enh = rng.standard_normal((n, C)).astype(F32)
    perms, signs = signed_permutations(rng, n, K)
    pcs = np.empty((n, K, C), F32)
    for c in range(n):
        seg = base[:, c * H:c * H + C] * (1 + 0.1 * np.arange(K))[:, None]
        pcs[c] = (signs[c][:, None] * seg[perms[c]] + noise * rng.standard_normal((K, C))).astype(F32)
    truth_perm = np.argsort(perms, axis=1).astype(np.int32)       # place of base s
    truth_sign = np.take_along_axis(signs, truth_perm.astype(np.int64), axis=1).astype(np.int32)
    return enh, pcs, truth_perm, truth_sign
