"""CPU: the host half of whole-recording enhancement: plan_chunks, the declarations, the refusals of
the entry points, the serial host core (nppc_enh_chain_host / nppc_enh_splice_host) against the numpy restatement
(tests/enhance_ref.py), and properties of the restatement itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import enhance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nppc_enh_shape", "nppc_enh_gram", "nppc_enh_chain", "nppc_enh_splice", "nppc_enh_chain_host", "nppc_enh_splice_host"]
STFT = dict(n_fft=4, hop_length=2, kersize=(2, 3))                # small enough for chunks of 16 samples


def E():
    from nppc_audio import enhance
    return enhance


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,C", [(10, 16), (16, 16), (17, 16), (24, 16), (25, 16), (32, 16), (41, 16), (100001, 4096)])
def test_plan_chunks(L, C):
    kw = STFT if C == 16 else dict(n_fft=256, hop_length=128, kersize=(3, 5, 10))
    plan = E().plan_chunks(L, C, **kw)
    assert plan == R.plan(L, C)
    H = C // 2
    if L <= C:
        assert plan == [(0, L)]
        return
    n = len(plan)
    assert n == -(-(L - C) // H) + 1
    assert [s for s, _ in plan] == [c * H for c in range(n)]
    assert all(ln == C for _, ln in plan[:-1]) and H < plan[-1][1] <= C
    assert plan[-1][0] + plan[-1][1] == L
    for (s0, l0), (s1, _) in zip(plan, plan[1:]):
        assert s0 + l0 - s1 == H                                   # adjacent chunks share exactly H samples


def test_plan_chunks_refusals():
    pc = E().plan_chunks
    for C in (15, 0, -16):
        with pytest.raises(ValueError, match="chunk_samples"):
            pc(100, C, **STFT)
    with pytest.raises(ValueError, match="half a chunk"):
        pc(100, 16, n_fft=4, hop_length=2, kersize=(5,))            # H = 8 < 2 x 5
    with pytest.raises(ValueError, match="half a chunk"):
        pc(100, 16, n_fft=32, hop_length=2, kersize=(2,))           # H = 8 < 16
    with pytest.raises(ValueError, match="recording"):
        pc(2, 16, **STFT)                                           # not more than n_fft // 2
    with pytest.raises(ValueError, match="recording"):
        pc(3, 16, **STFT)                                           # 2 frames, the largest kernel needs 3
    assert pc(4, 16, **STFT) == [(0, 4)]


# ---- declarations and refusals -------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_entry_points():
    from nppc_audio import _hip
    header = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _hip.SIGS and hasattr(_hip.lib(), name)
    for macro, value in (("NPPC_ENH_MAX_K", E().MAX_K), ("NPPC_ENH_MAX_SPLIT", E().MAX_SPLIT)):
        assert int(re.search(rf"#define {macro}\s+(\d+)", header).group(1)) == value


def test_shape_query():
    en = E()
    assert en.enh_shape(3, 5, 65536, 1) == (1, 8 * 2 * 1 * 35)
    assert en.enh_shape(3, 5, 65536, 1000) == (64, 8 * 2 * 64 * 35)
    assert en.enh_shape(3, 5, 2, 7) == (1, 8 * 2 * 35)              # H = 1: one sample cannot be split
    assert en.enh_shape(1, 5, 16, 0)[1] == 0
    S, nbytes = en.enh_shape(293, 5, 65536, 0)
    assert 1 <= S <= 64 and nbytes == 8 * 292 * S * 35
    assert en.enh_shape(2, 16, 65536, 0)[0] == 64                   # one boundary: split as far as it goes


def test_entry_points_refuse_bad_arguments_without_a_device():
    from nppc_audio import _hip
    call, P = _hip.call, _hip.c_p
    buf = (ctypes.c_double * 4096)()
    p = P(ctypes.addressof(buf))                                    # a non-null pointer no refused call may follow
    S, nb = ctypes.c_int(), ctypes.c_long()
    for args in ((0, 5, 16, 0), (3, 0, 16, 0), (3, 5, 15, 0), (3, 5, 0, 0), (3, 5, 16, -1)):
        with pytest.raises(RuntimeError, match="bad argument"):
            call("nppc_enh_shape", *args, ctypes.byref(S), ctypes.byref(nb))
    with pytest.raises(RuntimeError, match="unsupported"):
        call("nppc_enh_shape", 3, 17, 16, 0, ctypes.byref(S), ctypes.byref(nb))
    # gram: null pointers, one chunk, odd C, K over the cap, a split beyond the cap or beyond H
    for args, word in (((P(0), 32, 16, 3, 2, 16, 1, p), "bad argument"), ((p, 32, 16, 3, 2, 16, 1, P(0)), "bad argument"),
                       ((p, 32, 16, 1, 2, 16, 1, p), "bad argument"), ((p, 32, 16, 3, 2, 15, 1, p), "bad argument"),
                       ((p, 32, 16, 3, 17, 16, 1, p), "unsupported"), ((p, 32, 16, 3, 2, 16, 65, p), "bad argument"),
                       ((p, 32, 16, 3, 2, 16, 9, p), "bad argument"), ((p, -32, 16, 3, 2, 16, 1, p), "bad argument")):
        with pytest.raises(RuntimeError, match=word):
            call("nppc_enh_gram", *args, P(0))
    for args, word in (((p, 3, 2, 1, 0, P(0), p, p, p), "bad argument"), ((p, 0, 2, 1, 0, p, p, p, p), "bad argument"),
                       ((p, 3, 17, 1, 0, p, p, p, p), "unsupported"), ((p, 3, 2, 1, 2, p, p, p, p), "bad argument"),
                       ((P(0), 3, 2, 1, 0, p, p, p, p), "bad argument"), ((p, 3, 2, 0, 0, p, p, p, p), "bad argument"),
                       ((p, 3, 2, 1, 0, p, p, P(0), p), "bad argument"), ((p, 3, 2, 1, 0, p, p, p, P(0)), "bad argument")):
        with pytest.raises(RuntimeError, match=word):
            call("nppc_enh_chain", *args, P(0))
    good = dict(enh=p, e_cs=16, pcs=p, p_cs=32, p_ks=16, n=3, K=2, C=16, L=30, alphas=p, A=2, w=p, perm=p, sign=p, out=p, ldo=32)
    for change, word in ((dict(enh=P(0)), "bad argument"), (dict(out=P(0)), "bad argument"), (dict(pcs=P(0)), "bad argument"),
                         (dict(perm=P(0)), "bad argument"), (dict(sign=P(0)), "bad argument"), (dict(alphas=P(0)), "bad argument"),
                         (dict(w=P(0)), "bad argument"), (dict(n=0, L=5), "bad argument"), (dict(C=15), "bad argument"),
                         (dict(K=17), "unsupported"), (dict(L=16), "bad argument"), (dict(L=33), "bad argument"),
                         (dict(ldo=29), "bad argument"), (dict(A=-1), "bad argument"), (dict(p_ks=-1), "bad argument")):
        args = list({**good, **change}.values())
        with pytest.raises(RuntimeError, match=word):
            call("nppc_enh_splice", *args, P(0))
        with pytest.raises(RuntimeError, match=word):
            call("nppc_enh_splice_host", *args)
    for args, word in (((P(0), 32, 16, 3, 2, 16, 0, p, p, p, P(0)), "bad argument"), ((p, 32, 16, 0, 2, 16, 0, p, p, p, P(0)), "bad argument"),
                       ((p, 32, 16, 3, 2, 15, 0, p, p, p, P(0)), "bad argument"), ((p, 32, 16, 3, 17, 16, 0, p, p, p, P(0)), "unsupported"),
                       ((p, 32, 16, 3, 2, 16, 0, P(0), p, p, P(0)), "bad argument"), ((p, 32, 16, 3, 2, 16, 3, p, p, p, P(0)), "bad argument")):
        with pytest.raises(RuntimeError, match=word):
            call("nppc_enh_chain_host", *args)


def test_python_surface_refuses_before_any_launch():
    en = E()
    enh, pcs = torch.zeros(3, 16), torch.zeros(3, 2, 16)
    with pytest.raises(ValueError, match="match"):
        en.splice_chunks(enh, pcs, 16, [1.0], match="optimal")
    with pytest.raises(ValueError, match="want"):
        en.splice_chunks(enh, torch.zeros(2, 2, 16), 16, [1.0])
    with pytest.raises(ValueError, match="even"):
        en.splice_chunks(torch.zeros(3, 15), torch.zeros(3, 2, 15), 15, [1.0])
    with pytest.raises(ValueError, match="at most 16"):
        en.splice_chunks(enh, torch.zeros(3, 17, 16), 16, [1.0])
    for last in (0, 8, 17):
        with pytest.raises(ValueError, match="last_length"):
            en.splice_chunks(enh, pcs, last, [1.0])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            en.splice_chunks(enh, pcs, 16, [1.0])
    cfg = en.RecordingEnhancerConfig.model_fields if hasattr(en.RecordingEnhancerConfig, "model_fields") \
        else en.RecordingEnhancerConfig.__fields__
    assert {"model_configuration", "checkpoint_path", "device", "sample_rate", "chunk_samples", "chunk_batch", "match"} <= set(cfg)
    d = {k: (v.default if hasattr(v, "default") else None) for k, v in cfg.items()}
    assert (d["sample_rate"], d["chunk_samples"], d["chunk_batch"], d["match"]) == (16000, 65536, 32, "greedy")


# ---- the host core against the restatement -------------------------------------------------------------------------------
def host_case(K, C, n, last, alphas, match, seed):
    en = E()
    enh, pcs, truth_perm, truth_sign = R.directions(K, C, n, seed)
    want, perm, sign, cont, = R.enhance(enh, pcs, last, alphas, match)
    hp, hs, hc, hg = en.chain_host(torch.from_numpy(pcs), match, want_gram=True)
    assert np.array_equal(hp.numpy(), perm) and np.array_equal(hs.numpy(), sign)
    if n > 1:
        G, na, nb, absG = R.gram(pcs)
        ref = np.concatenate([G.reshape(n - 1, -1), na, nb], axis=1)
        H = C // 2
        lim = 2 * H * 2.0 ** -53 * np.concatenate([absG.reshape(n - 1, -1), na, nb], axis=1)
        assert np.all(np.abs(hg.numpy() - ref) <= lim)
        assert np.allclose(hc.numpy(), cont, rtol=0, atol=1e-12)
    got = en.splice_host(torch.from_numpy(enh), torch.from_numpy(pcs), last, alphas, hp, hs).numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return perm, sign, truth_perm, truth_sign


@pytest.mark.parametrize("K,C,n", R.CASES)
@pytest.mark.parametrize("match", ["greedy", "sign"])
def test_host_core_equals_the_restatement(K, C, n, match):
    seed = R.SEEDS[(K, C, n)]
    perm, sign, tp, ts = host_case(K, C, n, C, [-1.5, 0.75], match, seed)
    if match == "greedy":
        assert R.chain(R.directions(K, C, n, seed)[1])[3] >= 0.1 or K == 1
        assert np.array_equal(perm, tp) and np.array_equal(sign, ts)        # the restatement recovers the truth
    else:
        assert np.array_equal(perm, np.tile(np.arange(K), (n, 1)))


@pytest.mark.parametrize("K,C,n,last,alphas", [(2, 16, 1, 11, [1.0, -2.0]), (3, 16, 2, 9, [0.5]), (2, 16, 3, 16, [3.0]),
                                               (3, 64, 4, 33 + 17, [1.0, 2.0, 3.0]), (2, 16, 3, 13, None), (2, 18, 3, 10, [1.0])])
def test_host_splice_at_the_edges_of_the_plan(K, C, n, last, alphas):
    host_case(K, C, n, last, alphas, "greedy", 7)


def test_a_direction_that_is_zero_in_an_overlap():
    en = E()
    K, C, n = 3, 16, 3
    enh, pcs, _, _ = R.directions(K, C, n, 11)
    pcs[1, 1, :C // 2] = 0                                          # b_1 of boundary 1: every cosine with it is 0
    pcs[1, 2, C // 2:] = 0                                          # a_2 of boundary 2: its slot has no cosine at all
    perm, sign, cont, _ = R.chain(pcs)
    hp, hs, hc = en.chain_host(torch.from_numpy(pcs))
    assert np.array_equal(hp.numpy(), perm) and np.array_equal(hs.numpy(), sign) and np.array_equal(hc.numpy() == 0, cont == 0)
    s = int(np.flatnonzero(perm[1] == 2)[0])                        # the slot that follows direction 2 of chunk 1
    free = [k for k in range(K) if k not in perm[2][:s]]
    assert cont[1, s] == 0 and perm[2, s] == free[0] and sign[2, s] == sign[1, s]
    assert np.count_nonzero(cont[0] == 0) == 1 and sorted(perm[1]) == [0, 1, 2]


# ---- properties of the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 16, 18, 1024, 65536])
def test_the_two_weights_of_an_overlapped_sample_sum_to_one(C):
    w = R.table(C)
    assert w.dtype == np.float32 and w.shape == (C // 2,) and w[0] == 0
    assert np.array_equal(w, E().hann_table(C).numpy())
    other = (np.float32(1) - w).astype(np.float32)
    worst = np.abs(other.astype(np.float64) + w.astype(np.float64) - 1.0).max()
    assert worst <= 2.0 ** -24, worst


@pytest.mark.parametrize("K,C,n", R.CASES)
def test_a_signed_permutation_of_the_directions_changes_nothing(K, C, n):
    seed = R.SEEDS[(K, C, n)]
    enh, pcs, _, _ = R.directions(K, C, n, seed)
    alphas = [-2.0, 0.5, 3.0]
    base, perm, sign, _ = R.enhance(enh, pcs, C - 3, alphas)
    perms, signs = R.signed_permutations(np.random.default_rng(seed + 1), n, K)
    again, perm2, sign2, _ = R.enhance(enh, R.apply_signed(pcs, perms, signs), C - 3, alphas)
    assert np.array_equal(base.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(perms[np.arange(n)[:, None], perm2], perm)          # the same directions, found in their new places
    if K > 1:
        plain = R.splice(enh, R.apply_signed(pcs, perms, signs), C - 3, alphas, np.tile(np.arange(K, dtype=np.int32), (n, 1)),
                         np.ones((n, K), np.int32))
        assert not np.array_equal(plain, base)                                 # without alignment the splice does change

