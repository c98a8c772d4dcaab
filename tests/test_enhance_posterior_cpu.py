"""CPU: the host half of the posterior samples of whole recordings: what nppc_enh_post_sample_shape
accepts and refuses, every refusal of enhance.sample_chunks from shapes alone, and two properties of the fp64 restatement
(tests/enhance_posterior_ref.py): at z = 0 it is the splice of the chunks' waveforms, and it does not change under a signed
permutation of a chunk's raw directions when the tables move with them."""
import ctypes

import numpy as np
import pytest
import torch

import enhance_posterior_ref as EP
import enhance_ref as ER
import posterior_ref as PR
from nppc_audio import _hip as H

CONFIGS = [(64, 8), (64, 16), (64, 32), (512, 256)]               # test_posterior_gpu.CONFIGS


def E():
    from nppc_audio import enhance
    return enhance


# ---- the shape function --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,K,C,L,T,nfft,hop,stats", [
    (1, 1, 1, 128, 100, 7, 64, 16, 0), (5, 9, 5, 256, 640, 17, 64, 16, 1), (3, 4096, 16, 1024, 2048, 65, 64, 32, 1),
    (18, 16, 5, 65536, 589824 + 7, 257, 512, 256, 0),             # a 60 s recording at the default configuration
    (292, 64, 5, 65536, 9600000, 257, 512, 256, 1),               # 10 min, statistics
    (5, 3, 2, 1024, 2603, 33, 64, 32, 0),                         # the end-to-end test: g0_tiny's STFT, chunks of 1024
    (2, 17, 0, 64, 33 + 32, 9, 64, 8, 0), (2, 100000, 5, 256, 300, 9, 128, 32, 0)])
def test_shape_query_matches_the_restated_tiling(n, S, K, C, L, T, nfft, hop, stats):
    assert EP.shape_ok(n, S, K, C, L, T, nfft, hop, stats)
    got = E().enh_post_shape(n, S, K, C, L, T, nfft, hop, stats)
    assert got == EP.tiling(S, L, hop, stats)
    tiles, per, nbytes = got
    assert (tiles - 1) * per < S <= tiles * per and (nbytes > 0) == bool(stats)
    if not stats:
        assert per <= EP.TILE


@pytest.mark.parametrize("nfft,hop", CONFIGS + [(64, 64), (128, 64), (256, 32), (512, 64), (512, 128)])
def test_shape_query_takes_the_configurations_with_two_to_eight_frames_per_sample(nfft, hop):
    """every configuration of the clip sampler's tests but hop == n_fft: n_fft / 2 has to lie on the frame grid"""
    C = 8 * 4 * hop
    args = (3, 3, 5, C, 2 * C - 5, 1 + C // hop, nfft, hop, 0)
    ok = EP.shape_ok(*args)
    assert ok == (nfft // hop >= 2)
    if ok:
        E().enh_post_shape(*args)
    else:
        with pytest.raises(ValueError, match="bad argument"):
            E().enh_post_shape(*args)


BASE = dict(n=3, S=4, K=5, C=256, L=300 + 128, T=17, nfft=64, hop=16, stats=0)


@pytest.mark.parametrize("change", [
    dict(hop=64), dict(hop=4), dict(hop=24), dict(hop=0), dict(nfft=100), dict(nfft=1024, hop=256),
    dict(C=192),                                                  # H = 96 is no multiple of 4 hop = 64
    dict(C=254), dict(C=255), dict(C=0),
    dict(L=256), dict(L=513), dict(n=0), dict(n=1),               # L outside the plan of n chunks
    dict(K=17), dict(K=-1), dict(S=0), dict(T=0), dict(stats=2), dict(stats=3),
    dict(S=1, stats=1), dict(S=4097, stats=1), dict(S=8 * 65536 + 1)])
def test_shape_query_refuses_what_the_kernel_does_not_take(change):
    a = dict(BASE, **change)
    assert EP.shape_ok(**BASE) and (not EP.shape_ok(**a) or a["S"] > 8 * 65535)
    n, per, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    order = ("n", "S", "K", "C", "L", "T", "nfft", "hop", "stats")
    H.call("nppc_enh_post_sample_shape", *(BASE[k] for k in order), ctypes.byref(n), ctypes.byref(per), ctypes.byref(nbytes))
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_enh_post_sample_shape", *(a[k] for k in order), ctypes.byref(n), ctypes.byref(per), ctypes.byref(nbytes))


def test_entry_point_refuses_null_pointers_before_any_launch():
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_enh_post_sample", None, None, None, None, None, None, None, None, 0, 1, 1, 1, 128, 100, 7, 64, 16, None, 100,
               None, None, None, 0, None)


# ---- sample_chunks -------------------------------------------------------------------------------------------------------
def _shapes(n=3, S=4, K=3, C=256, last=200, nfft=64, hop=16):
    F, T = nfft // 2 + 1, 1 + C // hop
    return dict(pred_shape=(n, 2, F, T), w_shape=(n, K, 2, F, T), re_shape=(n, F, T), im_shape=(n, F, T), lengths=None,
                z_shape=(S, K, 2), perm_shape=(n, K), sign_shape=(n, K), last_length=last, chunk_samples=C, nfft=nfft, hop=hop,
                domain="compressed", samples=True, stats=False)


@pytest.mark.parametrize("change,match", [
    (dict(nfft=100), "n_fft"), (dict(hop=24), "n_fft"), (dict(hop=4), "n_fft"), (dict(hop=0), "n_fft"), (dict(hop=64), "n_fft"),
    (dict(chunk_samples=192), "half a chunk"), (dict(chunk_samples=255), "half a chunk"), (dict(chunk_samples=0), "half a chunk"),
    (dict(domain="linear"), "domain"), (dict(samples=False), "nothing asked"),
    (dict(pred_shape=(3, 2, 32, 17)), "pred_crm"), (dict(pred_shape=(3, 1, 33, 17)), "pred_crm"),
    (dict(w_shape=(3, 3, 2, 33, 18)), "w_mat"), (dict(w_shape=(2, 3, 2, 33, 17)), "w_mat"),
    (dict(w_shape=(3, 17, 2, 33, 17), z_shape=(4, 17, 2), perm_shape=(3, 17), sign_shape=(3, 17)), "at most 16"),
    (dict(re_shape=(3, 33, 16)), "noisy planes"), (dict(im_shape=(2, 33, 17)), "noisy planes"),
    (dict(z_shape=(4, 2, 2)), "coefficients"), (dict(z_shape=(3, 4, 3, 2)), "coefficients"), (dict(z_shape=(0, 3, 2)), "coefficients"),
    (dict(z_shape=(1, 3, 2), stats=True), "statistics need"), (dict(z_shape=(4097, 3, 2), stats=True), "statistics need"),
    (dict(perm_shape=(3, 2)), "perm"), (dict(sign_shape=(2, 3)), "perm"),
    (dict(last_length=128), "last_length"), (dict(last_length=257), "last_length"), (dict(last_length=0), "last_length"),
    (dict(lengths=[256, 256, 199]), "lengths"), (dict(lengths=[256, 200]), "lengths"), (dict(lengths=[256, 200, 200]), "lengths"),
    (dict(pred_shape=(3, 2, 33, 16), w_shape=(3, 3, 2, 33, 16), re_shape=(3, 33, 16), im_shape=(3, 33, 16)), "frames")])
def test_every_refusal_is_a_value_error_from_shapes_alone(change, match):
    E().check_sample_chunk_args(**_shapes())
    E().check_sample_chunk_args(**dict(_shapes(), lengths=[256, 256, 200]))
    with pytest.raises(ValueError, match=match):
        E().check_sample_chunk_args(**dict(_shapes(), **change))


def test_a_single_chunk_may_be_short_but_not_shorter_than_half_a_frame():
    one = dict(_shapes(n=1, last=100), pred_shape=(1, 2, 33, 7), w_shape=(1, 3, 2, 33, 7), re_shape=(1, 33, 7), im_shape=(1, 33, 7))
    assert E().check_sample_chunk_args(**one) == (1, 4, 3, 33, 7, 100)
    with pytest.raises(ValueError, match="too short"):
        E().check_sample_chunk_args(**dict(one, last_length=32))


def test_sample_chunks_refuses_before_it_needs_a_device():
    """the refusals are raised on CPU tensors, with or without a GPU in the machine"""
    n, S, K, C, last = 2, 2, 3, 256, 200
    pred, w, re, im, z = (torch.from_numpy(a) for a in EP.case(n, S, K, C, last, 64, 16, 0))
    perm = torch.arange(K, dtype=torch.int32).repeat(n, 1)
    sign = torch.ones_like(perm)
    sc = E().sample_chunks
    with pytest.raises(ValueError, match="n_fft"):
        sc(pred, w, re, im, None, z, perm, sign, last, C, 64, 4)
    with pytest.raises(ValueError, match="half a chunk"):
        sc(pred, w, re, im, None, z, perm, sign, last, 192, 64, 16)
    with pytest.raises(ValueError, match="statistics need"):
        sc(pred, w, re, im, None, z[:1], perm, sign, last, C, 64, 16, stats=True)
    with pytest.raises(ValueError, match="last_length"):
        sc(pred, w, re, im, None, z, perm, sign, 128, C, 64, 16)
    with pytest.raises(ValueError, match="coeffs are"):
        sc(pred, w, re, im, None, z[None], perm, sign, last, C, 64, 16)
    with pytest.raises(ValueError, match="coefficients"):
        sc(pred, w, re, im, None, z[:, :2], perm, sign, last, C, 64, 16)
    with pytest.raises(ValueError, match="perm"):
        sc(pred, w, re, im, None, z, perm[:1], sign, last, C, 64, 16)
    with pytest.raises(ValueError, match="coeffs"):
        sc(pred, w, re, im, None, [[0.0] * K], perm, sign, last, C, 64, 16)


# ---- the restatement -----------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24


@pytest.mark.parametrize("n,C,last", [(1, 256, 100), (2, 128, 65), (3, 256, 255), (5, 128, 128)])
@pytest.mark.parametrize("domain", ["compressed", "decompressed"])
def test_restatement_at_zero_is_the_splice_of_the_chunk_waveforms(n, C, last, domain):
    """enhance_ref.splice works in fp32 with every operation rounded on its own, the restatement in fp64: on waveforms of
    peak P the two differ by the roundings of the fp32 one: y_prev and y_cur to fp32 (together at most P 2^-24, weighted by
    1 - w and w), 1 - w (P 2^-24), the two products (together P 2^-24) and the sum (P 2^-24): 4 P 2^-24."""
    nfft, hop, K = 64, 16, 3
    pred, w, re, im, z = EP.case(n, 2, K, C, last, nfft, hop, seed=7)
    rng = np.random.default_rng(0)
    perm = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int32)
    sign = rng.choice([-1, 1], (n, K)).astype(np.int32)
    got = EP.sample_recording(pred, w, re, im, 0 * z, perm, sign, last, C, nfft, hop, domain)
    W = C if n > 1 else last
    y = PR.sample_waveforms(pred, w, re, im, np.zeros((n, 1, K, 2)), W, nfft, hop, lengths=EP.chunk_lengths(n, C, last),
                            domain=domain)["samples"][:, 0]
    enh = np.zeros((n, C), np.float32)
    enh[:, :W] = y
    want = ER.splice(enh, None, last, None, None, None)[0]
    L = (n - 1) * (C // 2) + last
    assert got.shape == (2, L) and np.array_equal(got[0], got[1])
    peak = np.abs(y).max()
    assert np.abs(got[0] - want).max() <= 4 * U24 * peak
    # outside the cross-fades nothing but the rounding of the waveform to fp32 separates them
    H = C // 2
    flat = np.r_[np.arange(min(H, L)), np.arange((n - 1) * H + H, L)] if n > 1 else np.arange(L)
    assert np.array_equal(got[0][flat].astype(np.float32), want[flat])


@pytest.mark.parametrize("n,K,C,last", [(2, 1, 128, 65), (3, 5, 128, 100), (5, 16, 128, 128)])
@pytest.mark.parametrize("domain", ["compressed", "decompressed"])
def test_restatement_does_not_change_under_signed_permutations_of_the_raw_directions(n, K, C, last, domain):
    nfft, hop, S = 64, 16, 3
    pred, w, re, im, z = EP.case(n, S, K, C, last, nfft, hop, seed=11, complex_coeffs=True)
    rng = np.random.default_rng(3)
    perm = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int32)
    sign = rng.choice([-1, 1], (n, K)).astype(np.int32)
    base = EP.sample_recording(pred, w, re, im, z, perm, sign, last, C, nfft, hop, domain)
    perms, signs = ER.signed_permutations(rng, n, K, first_identity=False)
    moved = ER.apply_signed(w.reshape(n, K, -1), perms, signs).reshape(w.shape)
    mperm, msign = EP.moved_tables(perm, sign, perms, signs)
    again = EP.sample_recording(pred, moved, re, im, z, mperm, msign, last, C, nfft, hop, domain)
    assert np.array_equal(base, again)
    if K > 1:                                                       # and only with the tables: the old ones give another recording
        plain = EP.sample_recording(pred, moved, re, im, z, perm, sign, last, C, nfft, hop, domain)
        assert not np.array_equal(base, plain)
