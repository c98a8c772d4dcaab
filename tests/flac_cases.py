"""The streams of the FLAC tests (tests/test_flac_cpu.py and tests/test_flac_gpu.py), written by the encoder of
tests/flac_ref.py: every axis of the case table of DESIGN.md section 8h, the scan-specific cases and the corrupt files.
`cases()` builds them once per process: {name: Case(data, pcm, bps, rate)} with pcm an int32 array [C, n]."""
import functools
from typing import NamedTuple

import numpy as np

import flac_ref as R

RATE = 16000


class Case(NamedTuple):
    data: bytes
    pcm: np.ndarray
    bps: int
    rate: int


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def walk(n, bps, seed, step=0.02):
    """a bounded random walk: a signal the predictors can do something with, using most of the sample range"""
    g = rng_of(seed)
    full = (1 << (bps - 1)) - 1
    x = np.cumsum(g.standard_normal(n)) * step * full
    x = x - np.linspace(x[0], x[-1], n)
    x = x / max(1.0, np.abs(x).max() / (0.9 * full)) + g.integers(-3, 4, n)
    return np.clip(np.rint(x), -full - 1, full).astype(np.int64)


def make(pcm, bps, rate=RATE, **kw):
    pcm = np.atleast_2d(np.asarray(pcm, np.int64))
    data = R.encode([c.tolist() for c in pcm], bps, rate, **kw)
    return Case(data, pcm.astype(np.int32), bps, rate)


def lpc_coefs(order, precision, shift, bps, seed):
    """random coefficients over the whole range of `precision` bits, scaled down only as far as the 32-bit residual needs"""
    g = rng_of(seed)
    c = g.integers(-(1 << (precision - 1)), 1 << (precision - 1), order)
    limit = (1 << (30 - bps)) << shift
    total = int(np.abs(c).sum())
    if total > limit:
        c = c * limit // total
    return [int(v) for v in c]


def residual_showcase(method):
    """fixed order 1, blocksize 192, partition order 3 (partition 0 has 23 residuals, the others 24): parameter 0 with a
    quotient of 70, the largest non-escape parameter, an escape with 0 raw bits, two with 17, then chosen parameters"""
    g = rng_of(40 + method)
    kmax = 30 if method else 14
    res = np.zeros(192, np.int64)                                  # res[0] is the warm-up sample
    res[1:24] = g.integers(-3, 4, 23)
    res[5], res[9] = 35, -35                                       # u = 70 and 69 at k = 0: unary runs of 70 and 69 zeros
    amp = g.integers(9000, 20000, 12)
    res[24:48:2], res[25:48:2] = amp, -amp                         # pairs cancel: the signal returns to where it was
    res[72] = -30000                                               # 48..71 stay zero: the escape with 0 raw bits
    res[73:96] = np.where(np.arange(23) % 2 == 0, 60000, -60000)   # needs 17 bits; ends 30000 above
    res[96] = -30000
    amp = g.integers(1000, 5000, 11)
    res[97:119:2], res[98:119:2] = amp, -amp
    res[120:] = g.integers(-200, 201, 72)
    s = np.cumsum(res)
    assert np.abs(s).max() < 32768
    params = [0, kmax, ("esc", 0), ("esc", 17), ("esc", 17), None, 3, 0]
    return make(s, 16, blocksizes=[192], frames=dict(subframes=R.fixed(1, method=method, porder=3, params=params)))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    # ---- blocksize: the table's sizes, fixed blocking, two whole frames and a short last one --------------------------
    for bs in (16, 192, 576, 1152, 4096, 4608):
        x = walk(2 * bs + bs // 3 + 1, 16, bs)
        out[f"bs{bs}"] = make(x, 16, blocksizes=[bs, bs, bs // 3 + 1], frames=dict(subframes=R.fixed(2)))
    # every blocksize header code in one variable-blocksize stream: 0001, 0010-0101, 1000-1111, 0111 (300), 0110 (16, 7)
    sizes = [192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 300, 16, 7]
    x = walk(sum(sizes), 16, 7)
    frames = [dict(subframes=R.fixed(1) if bs <= 4608 else R.verbatim(), bs_code=7 if bs == 300 else None) for bs in sizes]
    out["bs_codes_variable"] = make(x, 16, blocksizes=sizes, frames=frames, variable=True)
    # ---- subframe types ----------------------------------------------------------------------------------------------
    out["constant"] = make(np.full(200, -1234), 16, blocksizes=[192, 8], frames=dict(subframes=R.constant()))
    out["verbatim"] = make(walk(200, 16, 11), 16, blocksizes=[192, 8])
    for order in range(5):
        out[f"fixed{order}"] = make(walk(200, 16, 12 + order), 16, blocksizes=[192, 8],
                                    frames=[dict(subframes=R.fixed(order)), dict(subframes=R.fixed(order))])
    for order in (1, 2, 8, 12, 32):
        for prec in (1, 12, 15):
            for shift in (0, 7, 14):
                sub = R.lpc(lpc_coefs(order, prec, shift, 16, order * 100 + prec + shift), prec, shift)
                out[f"lpc{order}_p{prec}_s{shift}"] = make(walk(192, 16, order + prec + shift), 16, frames=dict(subframes=sub))
    for wasted in (1, 5):
        out[f"wasted{wasted}"] = make(walk(192, 16 - wasted, 20 + wasted) << wasted, 16,
                                      frames=dict(subframes=R.fixed(2, wasted=wasted)))
    out["wasted_verbatim"] = make(walk(64, 13, 27) << 3, 16, frames=dict(subframes=dict(type="verbatim", wasted=3)))
    out["bs_is_order_plus_1_lpc"] = make(walk(9, 16, 28), 16, frames=dict(subframes=R.lpc(lpc_coefs(8, 12, 7, 16, 1), 12, 7)))
    out["bs_is_order_plus_1_fixed"] = make(walk(5, 16, 29), 16, frames=dict(subframes=R.fixed(4)))
    out["bs_is_order"] = make(walk(4, 16, 30), 16, frames=dict(subframes=R.fixed(4)))
    # ---- residual ----------------------------------------------------------------------------------------------------
    for method in (0, 1):
        out[f"residual_method{method}"] = residual_showcase(method)
        for porder in (0, 3, 6):                                   # 6 is the maximum at blocksize 192 (3 samples >= order 2)
            out[f"rice{method}_porder{porder}"] = make(walk(192, 16, 50 + porder), 16,
                                                       frames=dict(subframes=R.fixed(2, method=method, porder=porder)))
    out["porder_max_pow2"] = make(walk(256, 16, 57), 16, frames=dict(subframes=R.fixed(1, porder=8)))   # one sample each
    # ---- sample formats ----------------------------------------------------------------------------------------------
    for bps in (8, 12, 16, 20, 24):
        for where in ("header", "streaminfo"):
            out[f"bps{bps}_{where}"] = make(walk(200, bps, bps), bps, blocksizes=[192, 8],
                                            frames=dict(subframes=R.fixed(2), size_code=where))
    full = rng_of(60).choice([-(1 << 23), (1 << 23) - 1], 256)      # every sample at one end of the 24-bit range
    out["fullscale24_lpc32"] = make(full, 24, frames=dict(subframes=R.lpc(lpc_coefs(32, 15, 14, 24, 61), 15, 14)))
    # ---- channels ----------------------------------------------------------------------------------------------------
    left = walk(200, 16, 70) // 2
    right = left + rng_of(71).integers(-40, 41, 200)
    other = walk(200, 16, 72)
    sub = R.fixed(2)
    out["ch2_independent"] = make([left, other], 16, blocksizes=[192, 8], frames=dict(subframes=sub))
    for a, name in ((1, "left_side"), (2, "side_right"), (3, "mid_side")):
        out[f"ch2_{name}"] = make([left, right], 16, blocksizes=[192, 8], frames=dict(subframes=sub, assign=a))
    assert ((left - right) % 2).any()
    out["ch3"] = make([left, right, other], 16, blocksizes=[192, 8],
                      frames=dict(subframes=[R.fixed(1), R.verbatim(), R.lpc([3, -1], 4, 1)]))
    out["ch2_24bit_mid_side"] = make([walk(100, 24, 73), walk(100, 24, 74)], 24, frames=dict(subframes=R.fixed(1), assign=3))
    # ---- sample rate codes -------------------------------------------------------------------------------------------
    for code in (0, 5, 12, 13, 14):
        out[f"rate_code{code}"] = make(walk(100, 16, 80 + code), 16, frames=dict(subframes=sub, rate_code=code))
    # ---- speech-like: the LibriSpeech shape --------------------------------------------------------------------------
    out["speech"] = speech(2.0, 90)
    # ---- scan-specific -----------------------------------------------------------------------------------------------
    out["last_frame_1"] = make(walk(17, 16, 91), 16, blocksizes=[16, 1], frames=dict(subframes=R.fixed(1)))
    out["frames200"] = make(walk(3200, 16, 92), 16, blocksizes=[16] * 200, frames=dict(subframes=R.fixed(1)))
    out["header_in_payload"] = header_in_payload()
    out["metadata"] = make(walk(200, 16, 93), 16, blocksizes=[192, 8], frames=dict(subframes=sub), metadata=METADATA)
    return out


METADATA = [(1, bytes(37)), (3, bytes(range(36))), (4, b"\x05\x00\x00\x00hello\x00\x00\x00\x00"), (2, b"appl" + bytes(9)),
            (6, b"\xff\xf8\x15\x08" * 5), (1, b"")]


def speech(seconds, seed, bs=4096):
    """16 kHz / 16-bit noise through a two-pole resonance, blocksize 4096, LPC order 8, partition order 3"""
    g = rng_of(seed)
    n = int(seconds * RATE)
    e = g.standard_normal(n) * (0.2 + np.abs(np.sin(np.arange(n) * 2 * np.pi * 3 / RATE)))
    x = np.zeros(n)
    for i in range(n):
        x[i] = e[i] + 1.6 * x[i - 1] - 0.8 * x[i - 2] if i > 1 else e[i]
    x = np.rint(x / np.abs(x).max() * 20000).astype(np.int64)
    coefs = [1638, -819, 20, -11, 5, 3, -2, 1]                     # 1.6, -0.8 at shift 10, and small change
    sizes = [bs] * (n // bs) + ([n % bs] if n % bs else [])
    frames = [dict(subframes=R.lpc(coefs, 12, 10, porder=3 if b % 8 == 0 and b >= 64 else 0)) for b in sizes]
    return make(x, 16, blocksizes=sizes, frames=frames)


def header_bytes(bsc=1, src=5, number=0):
    """a complete valid frame header of a mono 16-bit 16 kHz stream"""
    h = bytes([0xFF, 0xF8, (bsc << 4) | src, 0x08, number])
    return h + bytes([R.crc8(h)])


def header_in_payload():
    """a verbatim mono 16-bit frame whose samples spell a complete valid frame header (sync, codes, CRC-8), twice"""
    x = walk(192, 16, 94)
    h = header_bytes()
    words = [int.from_bytes(h[i:i + 2], "big", signed=True) for i in range(0, 6, 2)]
    x[10:13] = words
    x[100:103] = words
    c = make(x, 16, blocksizes=[192])
    assert c.data.count(h) == 2
    return c


def many_headers_in_payload():
    """one verbatim frame of 4608 samples that spell 1536 valid frame headers: more candidates than decode_files first
    makes room for (twice the frames STREAMINFO promises plus 1024), so the batch is run again with the certain bound"""
    h = header_bytes()
    words = [int.from_bytes(h[i:i + 2], "big", signed=True) for i in range(0, 6, 2)]
    c = make(np.tile(words, 1536), 16, blocksizes=[4608])
    assert c.data.count(h) == 1536
    return c


def header_at(offset, seed=95):
    """a stream whose first frame header starts at byte `offset` (a PADDING block takes up the room)"""
    pad = offset - (4 + 4 + 34 + 4)
    c = make(walk(400, 16, seed), 16, blocksizes=[192, 192, 16], frames=dict(subframes=R.fixed(2)), metadata=[(1, bytes(pad))])
    assert R.probe(c.data)["first_frame"] == offset
    return c


def tail_that_neighbour_completes(neighbour_first_byte=ord("f")):
    """a good stream followed by the first five bytes of a frame header of its own format whose CRC-8 would be the first
    byte of the next file ('f' of fLaC): bytes after total_samples are ignored, and the scan may not look past the file"""
    c = make(walk(200, 16, 96), 16, blocksizes=[192, 8], frames=dict(subframes=R.fixed(2)))
    for bsc in (1, 2, 3, 4, 5, 8, 9, 10, 11, 12):
        for src in (5, 0):
            for number in range(128):
                h = header_bytes(bsc, src, number)
                if h[5] == neighbour_first_byte:
                    return Case(c.data + h[:5], c.pcm, c.bps, c.rate)
    raise AssertionError("no such header")


def two_frame_stereo():
    """the stream of the mutation sweeps (and tests/golden/flac_two_frame.flac): stereo, two frames, LPC and fixed
    predictors, both Rice methods, an escape partition, mid/side and left/side"""
    left = walk(260, 16, 97, step=0.05) // 2
    right = left + rng_of(98).integers(-300, 301, 260)
    f0 = dict(assign=3, rate_code=5, subframes=[R.lpc([1700, -900, 60], 12, 10, porder=2, params=[None, None, ("esc", 13), None]),
                                   R.fixed(2, method=1, porder=1)])
    f1 = dict(assign=1, rate_code=5, subframes=[R.fixed(3), R.fixed(1, wasted=0, porder=2)])
    return make([left, right], 16, blocksizes=[160, 100], frames=[f0, f1])


def corrupt_files():
    """[(data, status)] : a bit flip in a verbatim payload (CRC-16), a truncation in the middle of a frame (truncated) and
    a reserved subframe type.  None of them can make the decoder leave its file: tools/check/flac_host_check.cc runs these
    very mutations, and every other one, under AddressSanitizer."""
    v = make(walk(200, 16, 99), 16, blocksizes=[192, 8]).data
    first = R.probe(v)["first_frame"]
    flipped = bytearray(v)
    flipped[first + 40] ^= 0x10
    t = cases()["bs576"].data
    truncated = t[:R.probe(t)["first_frame"] + 300]
    r = bytearray(cases()["fixed2"].data)
    hdr = R.parse_header(bytes(r), R.probe(bytes(r))["first_frame"], R.probe(bytes(r)))
    r[hdr["hdr_end"]] = 0x04                                       # subframe type 000010: reserved
    return [(bytes(flipped), R.CRC16), (bytes(truncated), R.TRUNCATED), (bytes(r), R.RESERVED)]


def write_wav(path, case):
    """the PCM of a case as a wav file that scipy reads back to the same values: 8-bit unsigned, 12 in 16, 20 and 24 in 32"""
    from scipy.io import wavfile
    pcm, bps = case.pcm.T, case.bps
    if bps == 8:
        a = (pcm + 128).astype(np.uint8)
    elif bps <= 16:
        a = (pcm << (16 - bps)).astype(np.int16)
    else:
        a = (pcm.astype(np.int64) << (32 - bps)).astype(np.int32)
    wavfile.write(str(path), case.rate, a[:, 0] if a.shape[1] == 1 else a)
