"""Restatement of the FLAC format in pure Python integers: the specification of csrc/flac_core.h.

`decode(data)` is the reference decoder.  `encode(...)` is a small encoder that writes EXACTLY the stream it is told to
write: the blocksizes, every subframe's type / order / coefficients / precision / shift / wasted bits, the Rice method,
partition order and per-partition parameter or escape, the channel assignment, the header codes and the metadata blocks are
all arguments.  Coefficients are arbitrary: the stream stays lossless because the residual is formed with the decoder's own
integer formula, and the encoder asserts that every residual fits in 32 bits.

No file written by libFLAC or any other encoder was available when this was written: the format is pinned by this file
alone, from the published specification (big-endian bit order throughout).
"""

OK, BAD_MARKER, TRUNCATED, BAD_STREAMINFO, UNSUPPORTED, BAD_HEADER, RESERVED, CRC16, COUNT_MISMATCH = range(9)
RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}
FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


class FlacRefError(ValueError):
    def __init__(self, status, what=""):
        super().__init__(f"status {status} {what}")
        self.status = status


def _table(poly, bits):
    top, mask, out = 1 << (bits - 1), (1 << bits) - 1, []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


# ---- bits ------------------------------------------------------------------------------------------------------------
class BitReader:
    def __init__(self, data, byte=0):
        self.data, self.pos, self.n = data, byte * 8, len(data) * 8

    def read(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.n:
            raise FlacRefError(TRUNCATED, "read past the end")
        a, b = self.pos >> 3, (self.pos + n + 7) >> 3
        v = int.from_bytes(self.data[a:b], "big") >> (b * 8 - self.pos - n)
        self.pos += n
        return v & ((1 << n) - 1)

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = 0
        while self.read(1) == 0:
            q += 1
        return q


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def write(self, value, n):
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.v, self.n = (self.v << n) | value, self.n + n

    def signed(self, value, n):
        assert -(1 << (n - 1)) <= value < (1 << (n - 1)), (value, n)
        self.write(value & ((1 << n) - 1), n)

    def unary(self, q):
        self.write(1, q + 1)

    def align(self):
        self.write(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def utf8_number(v):
    """the "UTF-8" coding of the frame header, up to 36 bits"""
    if v < 0x80:
        return bytes([v])
    for n, lead in ((2, 0xC0), (3, 0xE0), (4, 0xF0), (5, 0xF8), (6, 0xFC), (7, 0xFE)):
        if v < 1 << (5 * n + 1 if n < 7 else 36):
            body = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)]
            return bytes([lead | (v >> (6 * (n - 1)))] + body)
    raise ValueError(v)


# ---- reference decoder -----------------------------------------------------------------------------------------------
def probe(data):
    if data[:3] == b"ID3" or data[:4] == b"OggS":
        raise FlacRefError(UNSUPPORTED, "container")
    if len(data) < 4:
        raise FlacRefError(TRUNCATED if b"fLaC".startswith(bytes(data)) else BAD_MARKER)
    if data[:4] != b"fLaC":
        raise FlacRefError(BAD_MARKER)
    off, first, info = 4, True, None
    while True:
        if off + 4 > len(data):
            raise FlacRefError(TRUNCATED, "metadata")
        last, typ, n = data[off] >> 7, data[off] & 0x7F, int.from_bytes(data[off + 1:off + 4], "big")
        off += 4
        if typ == 127 or (first and (typ != 0 or n != 34)) or (not first and typ == 0):
            raise FlacRefError(BAD_STREAMINFO)
        if off + n > len(data):
            raise FlacRefError(TRUNCATED, "metadata")
        if first:
            r = BitReader(data, off)
            info = dict(min_blocksize=r.read(16), max_blocksize=r.read(16), min_frame=r.read(24), max_frame=r.read(24),
                        sample_rate=r.read(20), channels=r.read(3) + 1, bits_per_sample=r.read(5) + 1,
                        total_samples=r.read(36))
        off, first = off + n, False
        if last:
            break
    info["first_frame"] = off
    if info["min_blocksize"] < 1 or info["max_blocksize"] < info["min_blocksize"] or info["sample_rate"] == 0:
        raise FlacRefError(BAD_STREAMINFO)
    if info["total_samples"] == 0 or info["bits_per_sample"] not in (8, 12, 16, 20, 24):
        raise FlacRefError(UNSUPPORTED)
    return info


def parse_header(data, off, info):
    """-> dict(bs, channels, assign, bps, pos, hdr_end); FlacRefError otherwise"""
    if off >= len(data):
        raise FlacRefError(TRUNCATED, "no frame")
    r = BitReader(data, off)
    try:
        if r.read(14) != 0x3FFE or r.read(1):
            raise FlacRefError(BAD_HEADER, "sync")
        variable, bsc, src, chc, szc = r.read(1), r.read(4), r.read(4), r.read(4), r.read(3)
        if r.read(1) or bsc == 0 or src == 15 or chc > 10 or szc in (3, 7):
            raise FlacRefError(BAD_HEADER, "codes")
        b0 = r.read(8)
        if b0 < 0x80:
            n, val = 1, b0
        elif b0 == 0xFF or b0 & 0xC0 == 0x80:
            raise FlacRefError(BAD_HEADER, "number")
        else:
            n = 8 - (b0 ^ 0xFF).bit_length()
            val = b0 & ((1 << (7 - n)) - 1)
        for _ in range(n - 1):
            b = r.read(8)
            if b & 0xC0 != 0x80:
                raise FlacRefError(BAD_HEADER, "number")
            val = (val << 6) | (b & 0x3F)
        if bsc == 1:
            bs = 192
        elif bsc <= 5:
            bs = 576 << (bsc - 2)
        elif bsc == 6:
            bs = r.read(8) + 1
        elif bsc == 7:
            bs = r.read(16) + 1
        else:
            bs = 256 << (bsc - 8)
        rate = (info["sample_rate"] if src == 0 else RATES[src] if src < 12 else r.read(8) * 1000 if src == 12
                else r.read(16) if src == 13 else r.read(16) * 10)
        end = r.pos >> 3
        if crc8(data[off:end]) != r.read(8):
            raise FlacRefError(BAD_HEADER, "crc-8")
    except FlacRefError as e:
        if e.status == TRUNCATED:
            raise FlacRefError(TRUNCATED, "header") from None
        raise
    bps = info["bits_per_sample"] if szc == 0 else SIZES[szc]
    channels = chc + 1 if chc < 8 else 2
    if (channels != info["channels"] or bps != info["bits_per_sample"] or rate != info["sample_rate"]
            or bs > info["max_blocksize"]):
        raise FlacRefError(BAD_HEADER, "disagrees with STREAMINFO")
    return dict(bs=bs, channels=channels, assign=0 if chc < 8 else chc - 7, bps=bps,
                pos=val if variable else val * info["min_blocksize"], hdr_end=end + 1)


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _residual(r, out, bs, order, coefs, shift):
    method = r.read(2)
    if method > 1:
        raise FlacRefError(RESERVED, "residual method")
    pbits = 5 if method else 4
    po = r.read(4)
    psize = bs >> po
    if (po and bs % (1 << po)) or psize < order:
        raise FlacRefError(RESERVED, "partition order")
    for part in range(1 << po):
        cnt = psize - order if part == 0 else psize
        k = r.read(pbits)
        if k == (1 << pbits) - 1:
            n = r.read(5)
            res = [r.signed(n) if n else 0 for _ in range(cnt)]
        else:
            res = []
            for _ in range(cnt):
                u = ((r.unary() << k) | r.read(k)) & 0xFFFFFFFF
                res.append(_wrap32((u >> 1) ^ (-(u & 1))))
        for v in res:
            i = len(out)
            out.append(_wrap32(v + (sum(c * out[i - 1 - j] for j, c in enumerate(coefs)) >> shift)))


def _subframe(r, bs, bps):
    if r.read(1):
        raise FlacRefError(RESERVED, "subframe padding bit")
    typ, wasted = r.read(6), 0
    if r.read(1):
        wasted = r.unary() + 1
        if wasted >= bps:
            raise FlacRefError(RESERVED, "wasted bits")
    b = bps - wasted
    if typ == 0:
        out = [r.signed(b)] * bs
    elif typ == 1:
        out = [r.signed(b) for _ in range(bs)]
    elif 8 <= typ <= 12 or typ >= 32:
        order = typ - 31 if typ >= 32 else typ - 8
        if order > bs:
            raise FlacRefError(RESERVED, "order")
        out = [r.signed(b) for _ in range(order)]
        if typ >= 32:
            prec, shift = r.read(4) + 1, r.signed(5)
            if prec == 16 or shift < 0:
                raise FlacRefError(RESERVED, "lpc parameters")
            coefs = [r.signed(prec) for _ in range(order)]
        else:
            coefs, shift = FIXED[order], 0
        _residual(r, out, bs, order, coefs, shift)
    else:
        raise FlacRefError(RESERVED, "subframe type")
    return [_wrap32(v << wasted) for v in out]


def decode_frame(data, off, info, hdr):
    """-> (channels [C][bs], end offset)"""
    r = BitReader(data, hdr["hdr_end"])
    a = hdr["assign"]
    ch = [_subframe(r, hdr["bs"], hdr["bps"] + int((a, c) in ((1, 1), (2, 0), (3, 1)))) for c in range(hdr["channels"])]
    r.read(-r.pos % 8)
    want = r.read(16)
    end = r.pos >> 3
    if crc16(data[off:end - 2]) != want:
        raise FlacRefError(CRC16)
    if a == 1:
        ch[1] = [_wrap32(x - y) for x, y in zip(ch[0], ch[1])]
    elif a == 2:
        ch[0] = [_wrap32(x + y) for x, y in zip(ch[0], ch[1])]
    elif a == 3:
        m = [(x << 1) | (y & 1) for x, y in zip(ch[0], ch[1])]
        ch = [[_wrap32((mm + y) >> 1) for mm, y in zip(m, ch[1])], [_wrap32((mm - y) >> 1) for mm, y in zip(m, ch[1])]]
    return ch, end


def decode(data):
    """bytes -> (info, pcm [C][n] lists of ints): frame after frame from the first until total_samples are there"""
    data = bytes(data)
    info = probe(data)
    pcm = [[] for _ in range(info["channels"])]
    off, count = info["first_frame"], 0
    while count < info["total_samples"]:
        hdr = parse_header(data, off, info)
        if hdr["pos"] != count or hdr["bs"] > info["total_samples"] - count:
            raise FlacRefError(COUNT_MISMATCH)
        ch, off = decode_frame(data, off, info, hdr)
        for c, x in zip(pcm, ch):
            c.extend(x)
        count += hdr["bs"]
    return info, pcm


# ---- encoder ---------------------------------------------------------------------------------------------------------
def verbatim():
    return dict(type="verbatim")


def constant():
    return dict(type="constant")


def fixed(order, **kw):
    return dict(type="fixed", order=order, **kw)


def lpc(coefs, precision, shift, **kw):
    return dict(type="lpc", order=len(coefs), coefs=list(coefs), precision=precision, shift=shift, **kw)


def _best_k(res, kmax):
    best = None
    for k in range(kmax + 1):
        bits = sum((((v << 1) ^ (v >> 63)) >> k) + 1 + k for v in res)
        if best is None or bits < best[0]:
            best = (bits, k)
    return best[1] if best else 0


def _write_residual(w, res, bs, order, method, porder, params):
    pbits = 5 if method else 4
    esc = (1 << pbits) - 1
    w.write(method, 2)
    w.write(porder, 4)
    psize = bs >> porder
    assert (porder == 0 or bs % (1 << porder) == 0) and psize >= order, (bs, porder, order)
    i = 0
    for part in range(1 << porder):
        cnt = psize - order if part == 0 else psize
        vals, i = res[i:i + cnt], i + cnt
        p = params[part] if isinstance(params, (list, tuple)) and not (len(params) == 2 and params[0] == "esc") else params
        if p is None:
            p = _best_k(vals, esc - 1)
        if isinstance(p, tuple):                                   # ("esc", n)
            n = p[1]
            w.write(esc, pbits)
            w.write(n, 5)
            for v in vals:
                if n:
                    w.signed(v, n)
                else:
                    assert v == 0
        else:
            assert 0 <= p < esc
            w.write(p, pbits)
            for v in vals:
                u = (v << 1) ^ (v >> 63)                          # zigzag: even u -> u >> 1, odd u -> -(u >> 1) - 1
                w.unary(u >> p)
                w.write(u & ((1 << p) - 1), p)


def _write_subframe(w, s, bps, spec):
    bs, wasted = len(s), spec.get("wasted", 0)
    typ = spec["type"]
    order = spec.get("order", 0)
    code = {"constant": 0, "verbatim": 1}.get(typ, 8 + order if typ == "fixed" else 31 + order)
    w.write(0, 1)
    w.write(code, 6)
    w.write(1 if wasted else 0, 1)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in s), "wasted bits are not zero"
        w.unary(wasted - 1)
        s = [v >> wasted for v in s]
    b = bps - wasted
    if typ == "constant":
        assert len(set(s)) == 1
        w.signed(s[0], b)
    elif typ == "verbatim":
        for v in s:
            w.signed(v, b)
    else:
        assert order <= bs
        for v in s[:order]:
            w.signed(v, b)
        if typ == "lpc":
            prec, shift, coefs = spec["precision"], spec["shift"], spec["coefs"]
            assert 1 <= prec <= 15 and 0 <= shift <= 15 and 1 <= order <= 32
            w.write(prec - 1, 4)
            w.signed(shift, 5)
            for c in coefs:
                w.signed(c, prec)
        else:
            coefs, shift = FIXED[order], 0
        res = [s[i] - (sum(c * s[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, bs)]
        assert all(-(1 << 31) <= v < (1 << 31) for v in res), "a residual does not fit in 32 bits"
        _write_residual(w, res, bs, order, spec.get("method", 0), spec.get("porder", 0), spec.get("params"))


def _bs_code(bs):
    if bs == 192:
        return 1
    for c in range(2, 6):
        if bs == 576 << (c - 2):
            return c
    for c in range(8, 16):
        if bs == 256 << (c - 8):
            return c
    return 6 if bs <= 256 else 7


def encode_frame(block, bps, rate, number, variable, spec):
    """one frame.  block [C][bs]; spec: dict(subframes=[...] or one spec for every channel, assign=0..3, bs_code=, rate_code=,
    size_code="header" | "streaminfo")"""
    C, bs = len(block), len(block[0])
    a = spec.get("assign", 0)
    subs = spec.get("subframes", verbatim())
    subs = subs if isinstance(subs, list) else [subs] * C
    bsc = spec.get("bs_code") or _bs_code(bs)
    src = spec.get("rate_code", 0)
    szc = 0 if spec.get("size_code", "header") == "streaminfo" else {v: k for k, v in SIZES.items()}[bps]
    w = BitWriter()
    w.write(0x3FFE, 14)
    w.write(0, 1)
    w.write(int(variable), 1)
    w.write(bsc, 4)
    w.write(src, 4)
    w.write(C - 1 if a == 0 else 7 + a, 4)
    w.write(szc, 3)
    w.write(0, 1)
    for byte in utf8_number(number):
        w.write(byte, 8)
    if bsc in (6, 7):
        w.write(bs - 1, 8 if bsc == 6 else 16)
    else:
        assert _bs_code(bs) == bsc
    if src == 12:
        assert rate % 1000 == 0
        w.write(rate // 1000, 8)
    elif src == 13:
        w.write(rate, 16)
    elif src == 14:
        assert rate % 10 == 0
        w.write(rate // 10, 16)
    else:
        assert src == 0 or RATES[src] == rate
    w.write(crc8(w.bytes()), 8)
    ch = [list(x) for x in block]
    if a:
        assert C == 2
        left, right = ch
        side = [x - y for x, y in zip(left, right)]
        ch = [left, side] if a == 1 else [side, right] if a == 2 else [[(x + y) >> 1 for x, y in zip(left, right)], side]
    for c in range(C):
        _write_subframe(w, ch[c], bps + int((a, c) in ((1, 1), (2, 0), (3, 1))), subs[c])
    w.align()
    w.write(crc16(w.bytes()), 16)
    return w.bytes()


def metadata_block(typ, body, last=False):
    return bytes([(0x80 if last else 0) | typ]) + len(body).to_bytes(3, "big") + bytes(body)


def streaminfo(min_bs, max_bs, rate, channels, bps, total, min_frame=0, max_frame=0):
    w = BitWriter()
    for v, n in ((min_bs, 16), (max_bs, 16), (min_frame, 24), (max_frame, 24), (rate, 20), (channels - 1, 3), (bps - 1, 5),
                 (total, 36), (0, 128)):
        w.write(v, n)
    return w.bytes()


def encode(pcm, bps, rate=16000, blocksizes=None, frames=None, variable=False, metadata=(), numbers=None):
    """pcm [C][n] ints -> bytes.  blocksizes: the blocksize of every frame (their sum is n; default one frame); frames: one
    spec for every frame, or a list of one per frame (see encode_frame); metadata: [(type, body)] written after STREAMINFO;
    numbers: the coded number of every frame, when it is not to be the frame index (fixed) / first sample (variable)."""
    C, n = len(pcm), len(pcm[0])
    blocksizes = list(blocksizes or [n])
    assert sum(blocksizes) == n and all(len(c) == n for c in pcm)
    frames = frames if isinstance(frames, list) else [frames or {}] * len(blocksizes)
    min_bs = min(blocksizes[:-1]) if len(blocksizes) > 1 else blocksizes[0]
    max_bs = max(blocksizes)
    if not variable:
        assert all(b == blocksizes[0] for b in blocksizes[:-1]) and blocksizes[-1] <= blocksizes[0]
        min_bs = max_bs = blocksizes[0]
    out, pos = [], 0
    for i, (bs, spec) in enumerate(zip(blocksizes, frames)):
        number = numbers[i] if numbers else (pos if variable else i)
        out.append(encode_frame([c[pos:pos + bs] for c in pcm], bps, rate, number, variable, spec))
        pos += bs
    blocks = [(0, streaminfo(min_bs, max_bs, rate, C, bps, n, min(map(len, out)), max(map(len, out))))] + list(metadata)
    head = b"fLaC" + b"".join(metadata_block(t, b, i == len(blocks) - 1) for i, (t, b) in enumerate(blocks))
    return head + b"".join(out)
