"""The inputs of the FLAC encoder's predictor "lpc" (tests/test_flac_lpc_cpu.py, tests/test_flac_lpc_gpu.py) and, computed
once per process and shared, what the restatement tests/flac_lpc_ref.py makes of them.  Small on purpose: the smallest
shapes at which the new code can go wrong, each at 16 and at 24 bits."""
import functools
from typing import NamedTuple

import numpy as np
from scipy.signal import lfilter

import flac_enc_cases as K
import flac_lpc_ref as L

FORMANTS = ((600.0, 80.0), (1400.0, 100.0), (2600.0, 150.0))         # (centre, bandwidth) in Hz at 16 kHz


class Case(NamedTuple):
    name: str
    pcm: np.ndarray          # int32 [C, n]
    bps: int
    rate: int
    block_size: int
    max_order: int


def voiced(n, bps, seed=0, period=130, level=0.5):
    """a pulse train (16000 / 130 = 123 Hz) plus a little noise through three formant resonators: what the fixed predictors,
    polynomial extrapolators, do not follow and a linear predictor of order 6 and more does"""
    rng = np.random.default_rng(seed)
    y = np.zeros(n)
    y[::period] = 1.0
    y += 0.01 * rng.standard_normal(n)
    for f, bw in FORMANTS:
        r = np.exp(-np.pi * bw / 16000.0)
        y = lfilter([1.0], [1.0, -2.0 * r * np.cos(2.0 * np.pi * f / 16000.0), r * r], y)
    full = 1 << (bps - 1)
    return np.clip(np.rint(y / np.abs(y).max() * level * full), -full, full - 1).astype(np.int32)


def mono(x):
    return np.ascontiguousarray(np.asarray(x, np.int32)[None])


@functools.lru_cache(maxsize=None)
def cases(bps):
    full = 1 << (bps - 1)
    out = [Case(f"voiced_m{m}", mono(voiced(2 * 4096 + 500, bps, 1)), bps, 16000, 4096, m) for m in (8, 1, 12)]
    old = {c.name: c for c in K.cases(bps)}
    for name in ("main", "ramp", "spike", "stereo"):                  # constant, verbatim, fixed must win, the assignments
        c = old[name]
        out.append(Case(name, c.pcm, bps, c.rate, c.block_size, 8))
    edge1 = np.zeros(4096 + 50, np.int32)
    edge1[0] = 1                                                      # not constant, and its windowed block is all zero
    out.append(Case("edge1", mono(edge1), bps, 16000, 4096, 8))
    alt = np.where(np.arange(4096 + 31) % 2, -(full - 1), full - 1)   # the reflection coefficient of order 1 is nearly -1
    out.append(Case("alternating", mono(alt), bps, 16000, 4096, 8))
    for n in (1, 2, 13, 16, 17):                                      # orders capped by the block, and bs <= m
        out.append(Case(f"n{n}", mono(voiced(n + 40, bps, 2)[40:]), bps, 16000, 4096, 12))
    for bs, n in ((16, 16 * 3 + 5), (192, 192 * 2 + 50), (4608, 4608 + 300)):
        out.append(Case(f"bs{bs}", mono(voiced(n, bps, 3)), bps, 16000, bs, 12))
    if bps == 24:                                                     # full scale: the side channel reaches 2^24 at bs 4608
        t = np.arange(4608 + 100)
        square = np.where((t // 37) % 2, -(full - 1), full - 1).astype(np.int32)
        sine = np.rint((full - 1) * np.sin(2 * np.pi * t / 61.7)).astype(np.int32)
        for name, x in (("square", square), ("sine", sine)):
            out.append(Case(name, mono(x), bps, 16000, 4608, 8))
            out.append(Case(name + "_stereo", np.stack([x, -x]).astype(np.int32), bps, 16000, 4608, 8))
    return tuple(out)


def case(bps, name):
    return {c.name: c for c in cases(bps)}[name]


@functools.lru_cache(maxsize=None)
def reference(bps, name):
    """-> (bytes, frame specs) of the restatement, computed once per process"""
    c = case(bps, name)
    return L.encode(c.pcm, c.bps, c.rate, c.block_size, c.max_order, return_plan=True)


@functools.lru_cache(maxsize=None)
def fixed_reference(bps, name):
    """the fixed predictors' stream of the same input (tests/flac_enc_ref.py)"""
    c = case(bps, name)
    return K.E.encode(c.pcm, c.bps, c.rate, c.block_size)
