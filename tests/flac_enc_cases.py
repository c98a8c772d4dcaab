"""The inputs of the FLAC encoder tests (tests/test_flac_encode_cpu.py, tests/test_flac_encode_gpu.py) and, computed once
per process and shared, what the restatement tests/flac_enc_ref.py makes of them."""
import functools
from typing import NamedTuple

import numpy as np

import flac_enc_ref as E


class Case(NamedTuple):
    name: str
    pcm: np.ndarray          # int32 [C, n]
    bps: int
    rate: int
    block_size: int


def speech(n, bps, seed, noise=0.002):
    """two slow partials and a little noise in bursts: what the fixed predictors are good at"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = 0.02 + 0.98 * np.sin(2 * np.pi * t / 2900.0 + seed) ** 8    # bursts: the partitions want different parameters
    x = env * (0.25 * np.sin(2 * np.pi * 0.011 * t + seed) + 0.12 * np.sin(2 * np.pi * 0.037 * t)
               + 8 * noise * rng.standard_normal(n))
    full = 1 << (bps - 1)
    return np.clip(np.rint(x * full), -full, full - 1).astype(np.int32)


def white(n, bps, seed):
    full = 1 << (bps - 1)
    return np.random.default_rng(seed).integers(-full, full, n).astype(np.int32)


def spike_frame(bps):
    x = np.zeros(1001, np.int32)
    x[500] = min(30000, (1 << (bps - 1)) - 1)
    return x


def stereo(bps, seed):
    """four frames of 4096 built for assignments 1 (R = L), 0 (independent noise), 2 (L = R + noise) and 3 (a common part
    plus independent noise in both), and a short last frame"""
    full = 1 << (bps - 1)
    rng = np.random.default_rng(seed)
    a = max(2, full >> 9)
    nz = lambda: rng.integers(-a, a + 1, 4096).astype(np.int32)  # noqa: E731
    s = [speech(4096, bps, seed + i, 0.0) // 2 for i in range(4)]
    left = np.concatenate([s[0], white(4096, bps, seed + 9), s[2] + nz(), s[3] + nz(), speech(333, bps, seed + 5)])
    right = np.concatenate([s[0], white(4096, bps, seed + 10), s[2], s[3] + nz(), speech(333, bps, seed + 6)])
    return np.stack([left, right]).astype(np.int32)


def mono(x):
    return np.ascontiguousarray(np.asarray(x, np.int32)[None])


@functools.lru_cache(maxsize=None)
def cases(bps, full_set=True):
    """every shape of the issue at one sample size; full_set=False: the main file, the spike, the stereo file"""
    lim = 1 << (bps - 1)
    main = np.concatenate([speech(4096, bps, 1), np.zeros(4096, np.int32), white(4096, bps, 2), speech(1000, bps, 3)])
    out = [Case("main", mono(main), bps, 16000, 4096),
           Case("spike", mono(np.concatenate([speech(4096, bps, 4), spike_frame(bps)])), bps, 16000, 4096),
           Case("stereo", stereo(bps, 20), bps, 16000, 4096)]
    if not full_set:
        return tuple(out)
    for n in (1, 15, 16, 4095, 4096, 4097):
        out.append(Case(f"n{n}", mono(speech(n, bps, 30 + n % 7)), bps, 16000, 4096))
    out.append(Case("n2_stereo", np.stack([speech(2, bps, 40), speech(2, bps, 41)]), bps, 16000, 4096))
    for bs, n in ((16, 16 * 3 + 5), (192, 192 * 2 + 50), (4608, 4608 + 300)):
        out.append(Case(f"bs{bs}", mono(speech(n, bps, 50 + bs % 5)), bps, 16000, bs))
    out.append(Case("bs4608_stereo", np.stack([speech(4608 + 77, bps, 57), speech(4608 + 77, bps, 58)]), bps, 16000, 4608))
    for frames in (130, 2050):                                     # the frame number's 1 -> 2 and 2 -> 3 byte codes
        out.append(Case(f"bs16_{frames}", mono(speech(16 * frames, bps, 60)), bps, 16000, 16))
    ramp = np.arange(min(4096, 2 * lim), dtype=np.int32) - min(2048, lim)     # orders 2, 3 and 4 leave zeros
    out.append(Case("ramp", mono(ramp), bps, 16000, 4096))
    rng = np.random.default_rng(80)                                   # loud and quiet runs of 16: the finest partitions
    amp = np.repeat(np.where(np.arange(2 * 256) % 2, max(2, lim >> 3), 2), 16)
    out.append(Case("p8", mono(np.rint(rng.uniform(-1, 1, amp.size) * amp)), bps, 16000, 4096))
    out.append(Case("rate44100", mono(speech(5000, bps, 70)), bps, 44100, 4096))
    out.append(Case("rate12345", np.stack([speech(5000, bps, 71), speech(5000, bps, 72)]), bps, 12345, 4096))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(bps, name, full_set=True):
    """-> (bytes, frame specs) of the restatement, computed once per process"""
    c = {c.name: c for c in cases(bps, full_set)}[name]
    return E.encode(c.pcm, c.bps, c.rate, c.block_size, return_plan=True)
