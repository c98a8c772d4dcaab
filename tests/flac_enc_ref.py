"""Restatement of the FLAC encoder's decision rule (csrc/flac_enc_core.h) in numpy integers: the
specification of the host encoder and of the device kernels, which are tested for BYTE equality with `encode` below.

The rule only plans: it returns the `frames=` specs that tests/flac_ref.py's encoder, which writes exactly the stream it is
told to write, turns into bytes.  Two STREAMINFO fields are then set that flac_ref.encode leaves to its caller: min = max
blocksize = block_size whatever the length (flac_ref takes them from the first frame, which for a stream of one short frame
would state a blocksize below 16), and the MD5 of the unencoded samples (flac_ref writes sixteen zero bytes).

    subframe of width b (bps, or bps + 1 for a side channel):
      constant when all samples are equal; otherwise for fixed orders o = 0..min(4, bs) and partition orders
      p = 0..min(8, trailing_zeros(bs)) with (bs >> p) >= o every partition takes the Rice parameter k (0..14 in method 0,
      0..30 in method 1, the lowest on ties) that minimises the exact sum(u >> k) + cnt (1 + k), u = zigzag(residual);
      cost = 8 + o b + 6 + sum over partitions of (pbits + partition bits); the cheapest (o, p), ties to the lower o, then
      the lower p; verbatim when that cost >= 8 + bs b.  Method 0 when the frame's bps <= 16, else method 1.
    stereo: L, R, M = (L + R) >> 1, S = L - R costed as above; the cheapest of 0 (L,R), 1 (L,S), 2 (S,R), 3 (M,S), the
      lowest code on ties.  Other channel counts are coded independently.
"""
import hashlib

import numpy as np

import flac_ref


def plan_subframe(s, b, method):
    """s: int64 array -> (spec for flac_ref, bits)"""
    bs = len(s)
    if (s == s[0]).all():
        return flac_ref.constant(), 8 + b
    kmax, pbits = (30, 5) if method else (14, 4)
    ks = np.arange(kmax + 1, dtype=np.int64)
    pmax = 0
    while pmax < 8 and bs % (2 << pmax) == 0:
        pmax += 1
    best = None
    for o in range(min(4, bs) + 1):
        res = s
        for _ in range(o):
            res = np.diff(res)                                        # the fixed predictors are the finite differences
        u = np.concatenate([np.zeros(o, np.int64), (res << 1) ^ (res >> 63)])
        for p in range(pmax + 1):
            parts, ps = 1 << p, bs >> p
            if ps < o:
                continue
            cnt = np.full(parts, ps, np.int64)
            cnt[0] -= o
            bits = (u.reshape(parts, ps)[:, :, None] >> ks).sum(1) + cnt[:, None] * (1 + ks)      # [parts, k], exact
            cost = 8 + o * b + 6 + int((pbits + bits.min(1)).sum())
            if best is None or cost < best[0]:
                best = (cost, o, p, [int(k) for k in bits.argmin(1)])  # argmin: the first, so the lowest k
    cost, o, p, params = best
    if cost >= 8 + bs * b:
        return flac_ref.verbatim(), 8 + bs * b
    return flac_ref.fixed(o, method=method, porder=p, params=params), cost


def plan(pcm, bps, rate=16000, block_size=4096):
    """pcm [C][n] -> (blocksizes, frame specs)"""
    pcm = np.asarray(pcm, np.int64)
    C, n = pcm.shape
    method = 0 if bps <= 16 else 1
    rate_code = {v: k for k, v in flac_ref.RATES.items()}.get(rate, 0)
    sizes, specs = [], []
    for pos in range(0, n, block_size):
        blk = pcm[:, pos:pos + block_size]
        sizes.append(blk.shape[1])
        if C == 2:
            left, right = blk
            cands = [plan_subframe(x, bps + int(i == 3), method) for i, x in enumerate((left, right, (left + right) >> 1, left - right))]
            totals = [cands[0][1] + cands[1][1], cands[0][1] + cands[3][1], cands[3][1] + cands[1][1], cands[2][1] + cands[3][1]]
            a = totals.index(min(totals))                             # the first: the lowest code
            subs = [cands[i][0] for i in ((0, 1), (0, 3), (3, 1), (2, 3))[a]]
        else:
            a, subs = 0, [plan_subframe(x, bps, method)[0] for x in blk]
        specs.append(dict(subframes=subs, assign=a, rate_code=rate_code))
    return sizes, specs


def pcm_md5(pcm, bps):
    a = np.asarray(pcm, np.int64).T.reshape(-1)
    nb = (bps + 7) // 8
    return hashlib.md5(b"".join(int(v).to_bytes(nb, "little", signed=True) for v in a)).digest() if len(a) < 1 << 16 else \
        hashlib.md5(np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]).tobytes()).digest()


def encode(pcm, bps, rate=16000, block_size=4096, return_plan=False):
    """pcm [C][n] ints -> the bytes the encoder has to produce"""
    sizes, specs = plan(pcm, bps, rate, block_size)
    rows = [[int(v) for v in c] for c in np.asarray(pcm, np.int64)]
    data = bytearray(flac_ref.encode(rows, bps, rate, blocksizes=sizes, frames=specs))
    data[8:10] = data[10:12] = block_size.to_bytes(2, "big")
    data[26:42] = pcm_md5(pcm, bps)
    return (bytes(data), specs) if return_plan else bytes(data)
