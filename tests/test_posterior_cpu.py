"""CPU: the host side of the posterior sampler (nppc_audio/posterior.py) and its fp64 restatement (tests/posterior_ref.py):
coefficient shapes, the seeded draw, the tiling of nppc_post_sample_shape, every refusal before a launch, and two properties
of the rule itself."""
import ctypes

import numpy as np
import pytest
import torch

import posterior_ref as PR
from nppc_audio import _hip as H
from nppc_audio import posterior as P


def test_coefficient_shapes_and_conversions():
    g = torch.Generator().manual_seed(1)
    real = torch.randn(2, 3, 4, generator=g)
    z = P.as_coefficients(real)
    assert z.shape == (2, 3, 4, 2) and z.dtype == torch.float32 and z.is_contiguous()
    assert torch.equal(z[..., 0], real) and not z[..., 1].any()
    cplx = torch.complex(real, real.flip(0))
    zc = P.as_coefficients(cplx)
    assert torch.equal(zc[..., 0], real) and torch.equal(zc[..., 1], real.flip(0))
    assert torch.equal(P.as_coefficients(zc.double()), zc)
    assert P.as_coefficients(real.double()).dtype == torch.float32
    for bad in (real[0], torch.zeros(2, 3, 4, 3), torch.complex(zc, zc), [1.0]):
        with pytest.raises(ValueError):
            P.as_coefficients(bad)


def test_draw_coefficients_is_the_seeded_randn():
    z = P.draw_coefficients(2, 5, 3, seed=7, device="cpu")
    want = torch.randn(2, 5, 3, generator=torch.Generator().manual_seed(7))
    assert z.shape == (2, 5, 3, 2) and torch.equal(z[..., 0], want) and not z[..., 1].any()
    assert torch.equal(P.draw_coefficients(2, 5, 3, seed=7, temperature=0.5, device="cpu")[..., 0], want * 0.5)
    zc = P.draw_coefficients(2, 5, 3, seed=7, complex_coeffs=True, device="cpu")
    wc = torch.randn(2, 5, 3, 2, generator=torch.Generator().manual_seed(7)) * 0.5 ** 0.5
    assert torch.equal(zc, wc)
    g = torch.Generator().manual_seed(9)
    a, b = P.draw_coefficients(1, 2, 3, generator=g, device="cpu"), P.draw_coefficients(1, 2, 3, generator=g, device="cpu")
    assert not torch.equal(a, b)                                    # a generator moves on
    big = P.draw_coefficients(4, 4096, 4, seed=0, complex_coeffs=True, device="cpu")
    assert abs(float((big ** 2).sum(-1).mean()) - 1.0) < 0.02       # E|z|^2 = 1
    with pytest.raises(ValueError):
        P.draw_coefficients(1, 2, 3, seed=1, generator=g, device="cpu")
    with pytest.raises(ValueError):
        P.draw_coefficients(1, 0, 3, seed=1, device="cpu")


@pytest.mark.parametrize("B,S,T,nfft,hop,length,stats", [
    (1, 1, 13, 64, 8, 100, 0), (3, 9, 7, 64, 16, 100, 0), (3, 9, 7, 64, 16, 100, 3), (1, 4096, 251, 512, 256, 64000, 1),
    (8, 64, 251, 512, 256, 64000, 2), (8, 256, 251, 512, 256, 64000, 3), (1, 17, 40, 128, 32, 1000, 3), (2, 2, 3, 256, 256, 700, 1),
    (1, 100000, 5, 64, 32, 130, 0), (300, 4096, 5, 64, 32, 130, 3)])
def test_shape_query_matches_the_restated_tiling(B, S, T, nfft, hop, length, stats):
    got = P.sample_tiling(B, S, 5, T, nfft, hop, length, stats)
    assert got == PR.tiling(B, S, T, nfft, hop, length, stats)
    tiles, per, nbytes = got
    assert (tiles - 1) * per < S <= tiles * per and (nbytes > 0) == bool(stats)
    if not stats:
        assert per <= P.TILE


def test_shape_query_refuses_what_the_kernel_does_not_take():
    n, per, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    for args in ((1, 4, 5, 9, 100, 50, 400, 0), (1, 4, 5, 9, 512, 32, 400, 0), (1, 4, 5, 9, 512, 200, 400, 0), (1, 4, 17, 9, 64, 16, 400, 0),
                 (1, 1, 5, 9, 64, 16, 400, 1), (1, 4097, 5, 9, 64, 16, 400, 2), (0, 4, 5, 9, 64, 16, 400, 0), (1, 4, 5, 9, 64, 16, 0, 0),
                 (1, 4, 5, 9, 64, 16, 400, 4), (1, 8 * 65536, 5, 9, 64, 16, 400, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            H.call("nppc_post_sample_shape", *args, ctypes.byref(n), ctypes.byref(per), ctypes.byref(nbytes))
    # null pointers are rejected before any launch
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_post_sample", None, None, None, None, None, None, 0, 1, 1, 1, 9, 64, 16, 100, None, None, None, None, None,
               None, 0, None)


def _shapes(B=2, S=4, K=3, nfft=64, hop=16, length=100):
    F, T = nfft // 2 + 1, 1 + length // hop
    return dict(pred_shape=(B, 2, F, T), w_shape=(B, K, 2, F, T), re_shape=(B, F, T), im_shape=(B, F, T), z_shape=(B, S, K, 2),
                length=length, nfft=nfft, hop=hop, lengths=None, domain="compressed", samples=True, stats=False, spec_stats=False)


@pytest.mark.parametrize("change,match", [
    (dict(nfft=100), "n_fft"), (dict(hop=24), "n_fft"), (dict(hop=4), "n_fft"), (dict(hop=0), "n_fft"),
    (dict(w_shape=(2, 17, 2, 33, 7), z_shape=(2, 4, 17, 2)), "at most 16"),
    (dict(z_shape=(2, 4097, 3, 2), stats=True), "statistics need"), (dict(z_shape=(2, 4097, 3, 2), spec_stats=True), "statistics need"),
    (dict(z_shape=(2, 1, 3, 2), stats=True), "statistics need"),
    (dict(lengths=[100, 32]), "too short"), (dict(lengths=[100, 101]), "exceeds"), (dict(lengths=[100]), "entries"),
    (dict(length=112), "frames"), (dict(length=0), "frames"),
    (dict(re_shape=(2, 33, 6)), "noisy planes"), (dict(im_shape=(1, 33, 7)), "noisy planes"), (dict(w_shape=(2, 3, 2, 33, 8)), "w_mat"),
    (dict(pred_shape=(2, 2, 32, 7)), "pred_crm"), (dict(z_shape=(2, 4, 2, 2)), "coefficients"), (dict(z_shape=(1, 4, 3, 2)), "coefficients"),
    (dict(domain="linear"), "domain"), (dict(samples=False), "nothing asked")])
def test_every_refusal_is_a_value_error_from_shapes_alone(change, match):
    P.check_sample_args(**_shapes())
    with pytest.raises(ValueError, match=match):
        P.check_sample_args(**dict(_shapes(), **change))


def test_sample_waveforms_refuses_before_it_needs_a_device():
    """the refusals come before any device work: they are raised on CPU tensors, with or without a GPU in the machine"""
    pred, w, re, im, z = (torch.from_numpy(a) for a in PR.case(1, 2, 3, 64, 16, 100, 0))
    with pytest.raises(ValueError, match="n_fft"):
        P.sample_waveforms(pred, w, re, im, z, 100, nfft=64, hop=4)
    with pytest.raises(ValueError, match="at most 16"):
        P.sample_waveforms(pred, w.repeat(1, 6, 1, 1, 1), re, im, z.repeat(1, 1, 6, 1), 100, nfft=64, hop=16)
    with pytest.raises(ValueError, match="statistics need"):
        P.sample_waveforms(pred, w, re, im, z[:, :1], 100, nfft=64, hop=16, stats=True)
    with pytest.raises(ValueError, match="too short"):
        P.sample_waveforms(pred, w, re, im, z, 100, nfft=64, hop=16, lengths=[30])


def test_restatement_at_zero_is_the_inverse_stft_of_the_decompressed_restoration():
    nfft, hop, L = 64, 16, 100
    pred, w, re, im, z = PR.case(2, 1, 3, nfft, hop, L, 3)
    for domain in ("compressed", "decompressed"):
        got = PR.sample_waveforms(pred, w, re, im, 0 * z, L, nfft, hop, domain=domain)["samples"][:, 0]
        mr, mi = PR.decompress(pred[:, 0]), PR.decompress(pred[:, 1])
        xr, xi = mr * re - mi * im, mi * re + mr * im
        for b in range(2):
            assert np.array_equal(got[b], PR.istft(xr[b], xi[b], nfft, hop, L))
    # and the inverse STFT is torch's
    want = torch.istft(torch.complex(torch.from_numpy(xr), torch.from_numpy(xi)), nfft, hop, nfft,
                       torch.hann_window(nfft, dtype=torch.float64), center=True, length=L).numpy()
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()
    # the ragged rule: the item alone at its own length, zeros after
    rag = PR.sample_waveforms(pred, w, re, im, z, L, nfft, hop, lengths=[L, 37])
    alone = PR.sample_waveforms(pred[1:, :, :, :3], w[1:, :, :, :, :3], re[1:, :, :3], im[1:, :, :3], z[1:], 37, nfft, hop)
    assert np.array_equal(rag["samples"][1, :, :37], alone["samples"][0]) and not rag["samples"][1, :, 37:].any()
    assert not rag["mag"][1, :, :, 3:].any() and rag["mag"][1, :, :, :3].all()


def test_decompressed_domain_is_linear_in_z_and_the_compressed_domain_is_not():
    nfft, hop, L = 64, 16, 100
    pred, w, re, im, z = PR.case(1, 2, 3, nfft, hop, L, 5, complex_coeffs=True)
    z = z.astype(np.float64)
    z3 = np.concatenate([z, 0.5 * (z[:, :1] + z[:, 1:2])], axis=1)             # the midpoint of the two draws, exact in fp64
    lin = PR.sample_waveforms(pred, w, re, im, z3, L, nfft, hop, domain="decompressed")["samples"][0]
    peak = np.abs(lin).max()
    assert np.abs(lin[2] - 0.5 * (lin[0] + lin[1])).max() < 1e-12 * peak
    com = PR.sample_waveforms(pred, w, re, im, z3, L, nfft, hop, domain="compressed")["samples"][0]
    assert np.abs(com[2] - 0.5 * (com[0] + com[1])).max() > 1e-4 * np.abs(com).max()
