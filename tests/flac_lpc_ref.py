"""Restatement of the FLAC encoder's predictor "lpc" (csrc/flac_enc_core.h) in numpy integers and
fp64 scalars: the specification of the serial host encoder and of the device kernels, which are tested for BYTE equality
with `encode` below.  Like tests/flac_enc_ref.py, whose rule it extends and whose helpers it reuses, it only plans: the
specs go to tests/flac_ref.py's encoder, which writes exactly the stream it is told to write.

    a non-constant subframe of width b and block bs, max_order M in 1..12, adds to the fixed candidates (o, p):
      1. N = bs + 1, d_i = 2 i - (bs - 1), w_i = floor(2^15 (N^2 - d_i^2) / N^2), x_i = (s_i w_i) >> 15 (int64, arithmetic)
      2. r_l = sum_i x_i x_{i+l}, l = 0..M, exact (an empty sum is 0); r_0 == 0: no LPC candidates
      3. Levinson-Durbin in fp64, one rounding per operation, in THIS order:
           err = r_0;  order m = 1..min(M, bs):
             acc = r_m;  for j = 0..m-2: acc = acc - a_j r_{m-1-j};  k = acc / err
             k not finite or |k| >= 1: the list ends (this order and every higher one are no candidates)
             t_j = a_j - k a_{m-2-j} for j = 0..m-2;  t_{m-1} = k;  err = err (1 - k k)
             err not finite or <= 0: the list ends;  a = t
      4. P = 12 for bps <= 16, else 15; shift = the largest s in 0..15 with floor(max|a_j| 2^s + 0.5) <= 2^(P-1) - 1 (none:
         the order is no candidate); q_j = floor(a_j 2^shift + 0.5) clamped to [-2^(P-1), 2^(P-1) - 1]
      5. e_i = s_i - ((sum_j q_j s_{i-1-j}) >> shift); any e_i outside [-2^28, 2^28): the order is no candidate
      6. partitions and parameters as for the fixed orders; cost = 8 + m b + 4 + 5 + m P + 6 + sum(pbits + bits)
      7. the cheapest of all fixed (o, p) and LPC (m, p): ties to fixed before LPC, then the lower order, then the lower p;
         constant, the verbatim comparison and the stereo assignment as in tests/flac_enc_ref.py.

`rectangular=True` replaces the window by 2^15 everywhere (x = s): not a mode of the library, only the means by which
tools/bench_flac_lpc.py states what the window is worth.
"""
import math

import numpy as np

import flac_enc_ref as E
import flac_ref

MAX_ORDER = 12


def precision(bps):
    return 12 if bps <= 16 else 15


def window(bs):
    n = bs + 1
    d = 2 * np.arange(bs, dtype=np.int64) - (bs - 1)
    return ((n * n - d * d) << 15) // (n * n)


def autocorrelation(s, rectangular=False):
    """s: int64 [bs] -> r_0..r_12 as Python ints"""
    bs = len(s)
    x = s if rectangular else (s * window(bs)) >> 15
    return [int((x[:bs - lag] * x[lag:]).sum()) if lag < bs else 0 for lag in range(MAX_ORDER + 1)]


def levinson(r, top):
    """-> the coefficient lists of orders 1, 2, ... as far as the rule lets the recursion go"""
    out, a, err = [], [], float(r[0])
    for m in range(1, top + 1):
        acc = float(r[m])
        for j in range(m - 1):
            prod = a[j] * float(r[m - 1 - j])
            acc = acc - prod
        k = acc / err
        if not math.isfinite(k) or not abs(k) < 1.0:
            break
        t = []
        for j in range(m - 1):
            prod = k * a[m - 2 - j]
            t.append(a[j] - prod)
        t.append(k)
        kk = k * k
        one = 1.0 - kk
        err = err * one
        if not math.isfinite(err) or not err > 0.0:
            break
        a = t
        out.append(list(a))
    return out


def _round_half_up(v):
    return math.floor(v + 0.5) if math.isfinite(v) else v


def quantise(a, p_bits):
    """-> (q, shift) or None"""
    lim, low = (1 << (p_bits - 1)) - 1, -(1 << (p_bits - 1))
    cmax = max(abs(c) for c in a)
    for shift in range(15, -1, -1):
        if _round_half_up(cmax * float(1 << shift)) <= lim:
            return [int(min(lim, max(low, _round_half_up(c * float(1 << shift))))) for c in a], shift
    return None


def lpc_residual(s, q, shift):
    """s: int64 [bs] -> e_m .. e_{bs-1}"""
    m, bs = len(q), len(s)
    pred = np.zeros(bs - m, np.int64)
    for j, c in enumerate(q):
        pred += c * s[m - 1 - j:bs - 1 - j]
    return s[m:] - (pred >> shift)


def lpc_candidates(s, max_order, p_bits, rectangular=False):
    """-> [(m, q, shift, residual)] of the orders that are candidates"""
    bs = len(s)
    r = autocorrelation(s, rectangular)
    if r[0] == 0:
        return []
    out = []
    for a in levinson(r, min(max_order, bs)):
        qs = quantise(a, p_bits)
        if qs is None:
            continue
        res = lpc_residual(s, *qs)
        if len(res) and (res.min() < -(1 << 28) or res.max() >= 1 << 28):
            continue
        out.append((len(a), qs[0], qs[1], res))
    return out


def plan_subframe(s, b, method, max_order, p_bits, rectangular=False):
    """s: int64 array -> (spec for flac_ref, bits)"""
    bs = len(s)
    if (s == s[0]).all():
        return flac_ref.constant(), 8 + b
    kmax, pbits = (30, 5) if method else (14, 4)
    ks = np.arange(kmax + 1, dtype=np.int64)
    pmax = 0
    while pmax < 8 and bs % (2 << pmax) == 0:
        pmax += 1
    cands = []                                                        # (head bits, order, residual, spec maker), in tie order
    for o in range(min(4, bs) + 1):
        res = s
        for _ in range(o):
            res = np.diff(res)
        cands.append((8 + o * b + 6, o, res, lambda o=o, **kw: flac_ref.fixed(o, **kw)))
    for m, q, shift, res in lpc_candidates(s, max_order, p_bits, rectangular):
        cands.append((8 + m * b + 4 + 5 + m * p_bits + 6, m, res,
                      lambda q=q, shift=shift, **kw: flac_ref.lpc(q, p_bits, shift, **kw)))
    best = None
    for head, o, res, make in cands:
        u = np.concatenate([np.zeros(o, np.int64), (res << 1) ^ (res >> 63)])
        for p in range(pmax + 1):
            parts, ps = 1 << p, bs >> p
            if ps < o:
                continue
            cnt = np.full(parts, ps, np.int64)
            cnt[0] -= o
            bits = (u.reshape(parts, ps)[:, :, None] >> ks).sum(1) + cnt[:, None] * (1 + ks)      # [parts, k], exact
            cost = head + int((pbits + bits.min(1)).sum())
            if best is None or cost < best[0]:
                best = (cost, make, p, [int(k) for k in bits.argmin(1)])
    cost, make, p, params = best
    if cost >= 8 + bs * b:
        return flac_ref.verbatim(), 8 + bs * b
    return make(method=method, porder=p, params=params), cost


def plan(pcm, bps, rate=16000, block_size=4096, max_order=8, rectangular=False):
    """pcm [C][n] -> (blocksizes, frame specs, the subframes' bits per frame)"""
    assert 1 <= max_order <= MAX_ORDER
    pcm = np.asarray(pcm, np.int64)
    C, n = pcm.shape
    method, p_bits = (0 if bps <= 16 else 1), precision(bps)
    rate_code = {v: k for k, v in flac_ref.RATES.items()}.get(rate, 0)
    sizes, specs, bits = [], [], []
    for pos in range(0, n, block_size):
        blk = pcm[:, pos:pos + block_size]
        sizes.append(blk.shape[1])
        sub = lambda x, b: plan_subframe(x, b, method, max_order, p_bits, rectangular)  # noqa: E731
        if C == 2:
            left, right = blk
            cands = [sub(x, bps + int(i == 3)) for i, x in enumerate((left, right, (left + right) >> 1, left - right))]
            totals = [cands[0][1] + cands[1][1], cands[0][1] + cands[3][1], cands[3][1] + cands[1][1], cands[2][1] + cands[3][1]]
            a = totals.index(min(totals))                             # the first: the lowest code
            subs, total = [cands[i][0] for i in ((0, 1), (0, 3), (3, 1), (2, 3))[a]], totals[a]
        else:
            planned = [sub(x, bps) for x in blk]
            a, subs, total = 0, [p[0] for p in planned], sum(p[1] for p in planned)
        specs.append(dict(subframes=subs, assign=a, rate_code=rate_code))
        bits.append(total)
    return sizes, specs, bits


def encode(pcm, bps, rate=16000, block_size=4096, max_order=8, return_plan=False, rectangular=False):
    """pcm [C][n] ints -> the bytes the encoder has to produce with predictor "lpc" """
    sizes, specs, _ = plan(pcm, bps, rate, block_size, max_order, rectangular)
    rows = [[int(v) for v in c] for c in np.asarray(pcm, np.int64)]
    data = bytearray(flac_ref.encode(rows, bps, rate, blocksizes=sizes, frames=specs))
    data[8:10] = data[10:12] = block_size.to_bytes(2, "big")
    data[26:42] = E.pcm_md5(pcm, bps)
    return (bytes(data), specs) if return_plan else bytes(data)


def subframe_bits(pcm, bps, block_size=4096, max_order=8, rectangular=False):
    """the sum of the subframes' exact bit counts (no frame headers, padding or CRCs): what a size comparison needs"""
    return sum(plan(pcm, bps, 16000, block_size, max_order, rectangular)[2])
