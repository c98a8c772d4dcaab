"""The references and bound helpers of tests/unet_ref.py, checked on the CPU against torch, against the published
Philox4x32-10 known answers and against their own definitions, so that the GPU tests compare kernels with something that
has itself been tested."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
from vad_ref import philox4x32_10

# Random123 known-answer vectors of Philox4x32-10 (kat_vectors: counter, key -> output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_generators_reproduce_the_published_known_answers(ctr, key, want):
    assert tuple(philox4x32_10(ctr, key)) == want
    got = R.philox4x32_10_np(*[np.array([c], np.uint64) for c in ctr], *key)
    assert tuple(int(g[0]) for g in got) == want


def test_vectorised_philox_and_keep_bits_equal_the_scalar_generator():
    rng = np.random.default_rng(3)
    c = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    k0, k1 = 0x9ABC1234, 0x00001234
    got = np.stack(R.philox4x32_10_np(*c, k0, k1), -1)
    for i in range(c.shape[1]):
        assert tuple(int(v) for v in got[i]) == tuple(philox4x32_10(tuple(int(v) for v in c[:, i]), (k0, k1)))
    seed, stream_id = 0x1234_5678_9ABC, 6
    for p in (0.2, 0.5):
        a = R.dropout_keep_ref(9, 24, p, seed, stream_id)
        b = R.dropout_keep_ref(9, 24, p, seed, stream_id, philox=philox4x32_10)
        assert a.dtype == np.uint8 and a.shape == (9, 24) and np.array_equal(a, b)
    # the counter layout is (row, row >> 32, c4, stream): swapping c4 and the stream gives other bits
    w = philox4x32_10((5, 0, 2, stream_id), (seed & R.M32, seed >> 32))
    assert w != philox4x32_10((5, 0, stream_id, 2), (seed & R.M32, seed >> 32))
    th = R.dropout_threshold(0.2)
    assert list(R.dropout_keep_ref(9, 24, 0.2, seed, stream_id)[5, 8:12]) == [int(x >= th) for x in w]
    assert R.dropout_threshold(0.5) == 2 ** 31 and R.dropout_threshold(0.0) == 0
    assert R.dropout_threshold(0.2) == int(float(np.float32(0.2)) * 2 ** 32) and abs(th / 2 ** 32 - 0.2) < 1e-8
    keep = R.dropout_keep_ref(70, 128, 0.2, seed, stream_id)
    assert 0.78 < keep.mean() < 0.82
    assert R.drop_scale_f32(0.5) == 2.0 and abs(R.drop_scale_f32(0.2) - 1.25) < 2e-7


@pytest.mark.parametrize("H,W", [(7, 9), (2, 2), (6, 5)])
def test_tie_routing_reference_equals_torch(H, W):
    g = torch.Generator().manual_seed(H * 31 + W)
    x = R.tie_alphabet((2, 16, H, W), g)
    assert R.tie_fraction(x) > 1 / 3
    assert set(np.unique(x.numpy()).tolist()) <= {-1.0, 0.0, 1.0} and bool((torch.signbit(x) & (x == 0)).any())
    y, idx = R.maxpool_first_max_ref(x)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    assert torch.equal(y, yr.detach())
    assert int(idx.min()) >= 0 and int(idx.max()) <= 3
    dy = torch.randn(y.shape, generator=g)
    yr.backward(dy)
    assert torch.equal(R.maxpool_bwd_ref(dy, idx, H, W), xr.grad)        # torch routes to the first strict maximum too
    s = R.maxpool_bwd_ref(dy, idx, H, W, fill=7.0)
    assert bool((s[:, :, 2 * (H // 2):] == 7.0).all()) and bool((s[:, :, :, 2 * (W // 2):] == 7.0).all())
    assert torch.equal(s[:, :, :2 * (H // 2), :2 * (W // 2)], xr.grad[:, :, :2 * (H // 2), :2 * (W // 2)])
    # no ties with randn
    assert R.tie_fraction(torch.randn(2, 8, H, W, generator=g)) == 0.0


def test_batchnorm_launch_geometry():
    # (B,H,W,C) -> haloed rows P, workgroups, rows of the last workgroup, row lanes
    for (B, H, W, C), P, wg, last, rl in [((2, 30, 33, 64), 2240, 3, 192, 32), ((1, 23, 43, 512), 1125, 2, 101, 4),
                                          ((3, 9, 37, 256), 1287, 2, 263, 8), ((1, 2, 3, 128), 20, 1, 20, 16)]:
        assert B * (H + 2) * (W + 2) == P
        assert R.bn_rows_per_block(P) == 1024 and R.bn_workgroups(P) == wg
        assert P - (wg - 1) * 1024 == last and R.bn_row_lanes(C) == rl
        assert R.bn_chain(P, C) == 1024 // rl
    assert 101 % (4 * 4) != 0 and 1 * 2 * 3 < R.bn_row_lanes(128)
    assert R.bn_rows_per_block(1024) == 1024 and R.bn_rows_per_block(512 * 1024 + 1) == 1280
    P3 = 16 * 258 * 258                                   # about the C3 workload: more than one round of 256 rows
    assert R.bn_rows_per_block(P3) == 2304 and R.bn_workgroups(P3) <= 512
    # the slice walk of nppc_bn_stats_from_parts past its cap of 128 slices
    for (B, H, W), P, ntiles, per, used in [((1, 126, 127), 16512, 129, 2, 65), ((2, 126, 127), 33024, 258, 3, 86),
                                            ((1, 260, 62), 16768, 131, 2, 66)]:
        assert B * (H + 2) * (W + 2) == P and (P + 127) // 128 == ntiles and ntiles > 128
        assert (ntiles + 127) // 128 == per and (ntiles + per - 1) // per == used
    assert 129 - 64 * 2 == 1 and 258 - 85 * 3 == 3        # a partial and a full last slice
    # the last tile of the first two is all bottom halo (W + 2 >= its rows); the third's holds the last interior pixel
    assert 16512 - 128 * 128 <= 129 and 33024 - 257 * 128 <= 129 and 130 * 128 <= 260 * 64 + 62


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batchnorm_references_equal_torch_and_conditioning_leaves_no_borderline_mask(dtype):
    B, C, H, W = 2, 16, 5, 7
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    x0 = R.q(torch.randn(B, C, H, W, generator=g) * 2 + 0.5, dtype)
    x0[0, 0, 0, 0] = 0.0
    x = R.bn_condition(x0, gamma, beta, dtype)
    assert torch.equal(x, R.q(x, dtype))
    assert float((x - x0).abs().max()) <= (1e-2 if dtype == torch.float32 else 0.2) + 1e-6
    n = float(B * H * W)
    s1, s2, sa = R.bn_stats_ref(x)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    sc, sh, mean, rstd, rm_new, rv_new = R.bn_finalize_ref(s1, s2, n, gamma, beta, rm, rv)
    assert R.bn_near_zero(x, sc, sh) == 0
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm2, rv2 = rm.double(), rv.double()
    yr = F.leaky_relu(F.batch_norm(xr, rm2, rv2, gr, br, True, float(np.float32(0.1)), float(np.float32(1e-5))), R.SLOPE_F32)
    y, bound = R.bn_act_ref(x, sc, sh, dtype == torch.bfloat16)
    assert R.rel(y, yr.detach()) < 1e-13 and R.rel(rm_new, rm2) < 1e-13 and R.rel(rv_new, rv2) < 1e-13
    assert bool((bound >= 0).all())
    # the backward: with the fp32-rounded ss the device would hold, against fp64 autograd, with and without a second
    # gradient and a dropout mask
    ss = np.concatenate([sc, sh, mean, rstd])
    d1, d2 = R.q(torch.randn(B, C, H, W, generator=g), dtype), R.q(torch.randn(B, C, H, W, generator=g), dtype)
    keep = R.keep_nchw(R.dropout_keep_ref(B * (H + 2) * (W + 2), C, 0.5, 77, 3), B, H, W)
    for dyb, km, p in ((d2, None, 0.0), (None, None, 0.0), (d2, keep, 0.5)):
        for t in (xr, gr, br):
            t.grad = None
        out = yr if km is None else yr * km * 2.0
        up = d1.double() if dyb is None else d1.double() + dyb.double()
        out.backward(up, retain_graph=True)
        S1, S2, a1, a2, gq, xh = R.bn_bwd_sums_ref(x, ss, d1, dyb, km, p)
        assert R.rel(S1, br.grad) < 1e-12 and R.rel(S2, gr.grad) < 1e-12
        assert R.rel(R.bn_dx_ref(ss, S1, S2, gq, xh, n), xr.grad) < 1e-12
        assert np.all(a1 >= np.abs(S1)) and np.all(a2 >= np.abs(S2))
        b1, b2 = R.bn_bwd_sum_bounds(2240, 64, a1, a2)
        assert np.allclose(b1, 36 * 2.0 ** -24 * a1) and np.allclose(b2, 40 * 2.0 ** -24 * a2)


def test_ratio_and_rel_helpers():
    assert R.ratio([0.0, 1.0], [0.0, 2.0]) == 0.5
    assert R.ratio([1e-9, 0.0], [0.0, 1.0]) == float("inf")
    assert R.ratio([float("nan")], [1.0]) == float("inf")
    assert R.ratio([2.0], [2.0]) == 1.0
    assert R.rel([1.0, 2.0], [1.0, 4.0]) == 0.5


def test_upsample_reference_at_degenerate_sizes():
    g = torch.Generator().manual_seed(2)
    for Hi, Wi, Ht, Wt in [(1, 1, 2, 2), (1, 1, 3, 3), (1, 4, 3, 9), (3, 5, 7, 10), (4, 6, 8, 12)]:
        x = torch.randn(2, 3, Hi, Wi, generator=g)
        up, (py, px) = R.upsample_pad_ref(x, Ht, Wt)
        assert up.shape[2:] == (Ht, Wt) and (py, px) == ((Ht - 2 * Hi) // 2, (Wt - 2 * Wi) // 2)
        win = up[:, :, py:py + 2 * Hi, px:px + 2 * Wi]
        assert float(up.abs().sum() - win.abs().sum()) == 0.0                      # the ring is padding
        assert torch.equal(win[:, :, 0, 0], x[:, :, 0, 0]) and torch.equal(win[:, :, -1, -1], x[:, :, -1, -1])
        if Hi == 1:
            assert torch.equal(win[:, :, 0], win[:, :, 1])                        # one input row: both output rows copy it


def test_boundary_map_references():
    g = torch.Generator().manual_seed(4)
    spec = torch.randn(2, 2, 5, 7, generator=g)
    spec[0, :, 0, 0] = 0.0
    spec[1, 0, 1, 1], spec[1, 1, 1, 1] = 1e-40, -3e-42
    ref, bound = R.logmag_ref(spec)
    want = torch.log(torch.sqrt(spec[:, 0].double() ** 2 + spec[:, 1].double() ** 2) + 1e-6)
    assert R.rel(ref, want) < 1e-8 and abs(float(ref[0, 0, 0]) - np.log(1e-6)) < 1e-7
    assert float(bound.min()) >= 8 * R.U24 and float(bound[0, 0, 0]) > 8 * R.U24 * 13
    a = ref.float()
    s1, s2 = float(a.double().sum()), float((a.double() ** 2).sum())
    z, zb, mean, std = R.standardize_ref(a, s1, s2, float(a.numel()))
    assert abs(mean - float(a.double().mean())) < 1e-12 and abs(std - float(a.double().std())) < 1e-12
    assert abs(float(z.mean())) < 1e-12 and abs(float(z.std()) - 1) < 1e-12
    raw, xin = torch.randn(2, 3, 5, 7, generator=g), torch.randn(2, 5, 7, generator=g)
    mask = torch.tensor([[0, 1, 1, 0, 0.25, 1, 0], [1, 0, 0, 1, 0.25, 0, 1]], dtype=torch.float32)
    o0, b0 = R.unet_out_ref(raw, mask)
    assert torch.equal(o0[:, :, :, 0][0], raw.double()[0, :, :, 0]) and float(o0[0, :, :, 1].abs().max()) == 0.0
    o1, b1 = R.unet_out_ref(raw[:, :1], mask, xin)
    assert torch.equal(o1[0, 0, :, 1], xin.double()[0, :, 1]) and torch.equal(o1[0, 0, :, 0], raw.double()[0, 0, :, 0])
    assert abs(float(o1[0, 0, 2, 4]) - (0.25 * float(xin[0, 2, 4]) + 0.75 * float(raw[0, 0, 2, 4]))) < 1e-15
    d, db = R.unet_out_bwd_ref(raw, mask, True)
    assert torch.equal(d, o0) and float(db.max()) <= (3 * R.U24 + R.U8) * float(d.abs().max())
