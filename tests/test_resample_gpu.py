"""GPU: nppc_resample_sinc (csrc/resample.hip) against the fp64 restatement (tests/resample_ref.py).

Shapes: seven ratios; batches of B = 3 ragged items in a buffer wider than every item, NaN stored past each item's length;
lengths 0, 1, width - 1, the lengths whose output ends one sample before, on and after the first output-tile boundary (where
the ratio reaches them: 1 -> 3 only gives multiples of 3, the nearest lengths at or above are taken) and one that needs a
third tile.

Bound: an output is one fp32 fma chain over the n = count[p] live taps of its phase, started from 0, so
|y - ref| <= gamma_n sum_k |h_k x_k| + 1e-12, gamma_n = n u / (1 - n u), u = 2^-24, with ref the fp64 sum over the same fp32
taps.  Derived, so no slack is added.  Everything else is bit equality."""
import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
RATIOS = [(441, 160), (160, 441), (3, 1), (1, 3), (2, 1), (1, 2), (7, 5)]


def RS():
    from nppc_audio import resample
    return resample


def signal(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.3 * np.sin(0.05 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def length_for(out, orig, new):
    """the smallest input length with at least `out` outputs"""
    n = out * orig // new
    while -(-new * n // orig) < out:
        n += 1
    return n


def batches(t):
    tile = t.tile
    edge = [length_for(tile + d, t.orig, t.new) for d in (-1, 0, 1)]
    return [[0, 1, t.width - 1], edge, [length_for(2 * tile + 5, t.orig, t.new), 1, edge[1]]]


@pytest.mark.parametrize("orig,new", RATIOS)
def test_ragged_batches_within_the_derived_bound_and_bit_stable(orig, new, record_err):
    t = RS().sinc_table(orig, new)
    count = t.count.numpy()
    worst = 0.0
    for bi, lens in enumerate(batches(t)):
        ldx = max(lens) + 37
        x = np.full((3, ldx), np.nan, dtype=np.float32)
        for b, n in enumerate(lens):
            x[b, :n] = signal(n, seed=10 * bi + b)
        xd = torch.from_numpy(x).cuda()
        y, out = RS().resample(xd, orig, new, lengths=lens)
        assert y.is_cuda and y.dtype == torch.float32
        assert out.tolist() == [R.out_length(n, orig, new) for n in lens] and y.shape == (3, max(out.tolist()))
        assert bool(torch.isfinite(y).all())                               # the NaN past an item never reaches an output
        y2, _ = RS().resample(xd, orig, new, lengths=lens)
        assert torch.equal(bits(y), bits(y2))                              # run to run
        yh = y.cpu().numpy()
        for b, n in enumerate(lens):
            m = int(out[b])
            assert not yh[b, m:].any()                                     # zero past the item's outputs
            ref, mag = R.resample(x[b, :n], orig, new)
            lim = R.gamma(count[np.arange(m) % new]) * mag + 1e-12
            if m:
                worst = max(worst, float((np.abs(yh[b, :m].astype(np.float64) - ref) / lim).max()))
            alone = RS().resample(torch.from_numpy(x[b, :n].copy()).cuda(), orig, new)
            assert alone.shape == (m,) and torch.equal(bits(alone), bits(y[b, :m]))   # the batch does not matter
    print(f"{orig}->{new}: worst error / bound {worst:.4f}")
    record_err(f"hip_{orig}_{new}", worst, 1.0)


@pytest.mark.parametrize("orig,new", [(441, 160), (160, 441), (3, 1), (1, 3)])
def test_outputs_outside_the_mapped_gap_keep_their_bits(orig, new):
    t = RS().sinc_table(orig, new)
    n = length_for(2 * t.tile + 300, orig, new)
    x = signal(n, 5)
    n_out = R.out_length(n, orig, new)
    y0 = RS().resample(torch.from_numpy(x).cuda(), orig, new)
    rng = np.random.default_rng(6)
    for s, e in [(0, 9), (n // 2, n // 2 + 1), (n // 3, n // 3 + 2 * orig + 3), (n - 5, n)]:
        z = x.copy()
        z[s:e] = 5.0 + rng.standard_normal(e - s).astype(np.float32)
        a, b = RS().map_gap(s, e, t, out_len=n_out)
        assert (a, b) == R.map_gap(s, e, n, orig, new) and b > a
        y1 = RS().resample(torch.from_numpy(z).cuda(), orig, new)
        assert torch.equal(bits(y0[:a]), bits(y1[:a])) and torch.equal(bits(y0[b:]), bits(y1[b:]))
        assert float((y0 - y1)[a:b].abs().max()) > 0.5


def test_module_batch_without_lengths_and_host_input():
    x = torch.from_numpy(np.stack([signal(3000, 1), signal(3000, 2)]))
    m = RS().Resample(44100, 16000)
    y = m(x.cuda())
    assert y.shape == (2, R.out_length(3000, 441, 160)) and y.is_cuda
    assert torch.equal(bits(y), bits(m(x)))                                # a host input is uploaded
    assert torch.equal(bits(y[1]), bits(RS().resample(x[1].cuda(), 44100, 16000)))
    wide = torch.full((2, 3100), float("nan"))
    wide[:, :3000] = x
    yw, out = RS().resample(wide.cuda()[:, :3050], 44100, 16000, lengths=[3000, 3000])     # rows of a wider buffer
    assert torch.equal(bits(yw), bits(y)) and out.tolist() == [y.shape[1]] * 2
    same = x.cuda()
    assert RS().resample(same, 16000, 16000) is same
