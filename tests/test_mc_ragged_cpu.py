"""CPU: the fp64 restatement of the ragged-gap MC-dropout + PCA baseline (tests/mc_ragged_ref.py) is the yardstick of the
GPU tests, so its own properties are checked here; plus the argument rules of the Python wrappers and of the entry points,
which refuse before anything asks for a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mc_ragged_ref as R
from oracle import inpaint_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, GAP, WIN, HOP = 32704, 2048, 255, 128


def separated_stack(rng, K, D, n_sig=8, noise=1e-3):
    """K samples of D elements, U diag(s) V^T + small noise with singular values 16, 8, 4, ...: no near-degenerate pair
    among the leading min(n_sig, K - 1, D) components"""
    r = max(1, min(n_sig, K - 1, D))
    U = np.linalg.qr(rng.standard_normal((K, r)))[0]
    V = np.linalg.qr(rng.standard_normal((D, r)))[0] if D >= r else rng.standard_normal((D, r))
    s = 16.0 * 0.5 ** np.arange(r)
    x = (U * s) @ V.T + noise * rng.standard_normal((K, D)) + rng.standard_normal(D)      # + a mean to remove
    return x.astype(np.float32)


def test_gap_frame_counts_of_the_reference_dataset():
    """every start the dataset can draw: 17 frames for two residues of (s - 127) mod 128, 18 for the other 126, as long as
    every touched frame exists; fewer once the last touched frame would lie past the end of the clip.  (At the front the
    clamped window removes nothing: frame 0 exists, and the closed form already holds from s = 0.)"""
    T = 1 + L // HOP
    counts = {s: R.gap_frames(s, L, GAP, WIN, HOP) for s in range(0, L - GAP + 1)}
    closed = {s: R.gap_frames_closed_form(s, WIN, HOP) for s in counts}
    last_touched = lambda s: (s + GAP - 1 + WIN // 2) // HOP
    interior = [s for s in counts if s >= WIN // 2 and last_touched(s) <= T - 1]
    clamped_end = [s for s in counts if last_touched(s) > T - 1]
    clamped_front = [s for s in counts if s < WIN // 2]
    assert len(interior) > 30000 and len(clamped_end) > 0 and len(clamped_front) == WIN // 2
    assert all(counts[s] == closed[s] for s in interior)
    assert all(counts[s] < closed[s] for s in clamped_end)
    assert all(counts[s] <= closed[s] for s in clamped_front)
    # 17 frames for exactly two residues out of 128
    by_res = {}
    for s in interior:
        by_res.setdefault((s - WIN // 2) % HOP, set()).add(counts[s])
    assert sorted(r for r, v in by_res.items() if v == {17}) == [1, 2]
    assert all(v == {18} for r, v in by_res.items() if r not in (1, 2)) and len(by_res) == HOP
    # the same count through the project's own restatement of time_to_spec_mask
    for s in (0, 1, 2, 127, 128, 129, 130, 5000, 30593, 30594, L - GAP):
        mt = torch.ones(1, L)
        mt[0, s:s + GAP] = 0
        assert int((O.time_to_spec_mask(mt, T, L, WIN, HOP) == 0).sum()) == counts[s], s


def test_index_gather_scatter_restatement_against_boolean_indexing():
    rng = np.random.default_rng(0)
    B, F, T = 4, 8, 21
    mask = np.ones((B, F, T), dtype=np.float32)
    mask[0, :, 4] = 0
    mask[1, :, 2:4] = 0
    mask[1, :, 17] = 0
    mask[2] = (rng.random((F, T)) > 0.3)
    mask[3] = 0
    mask[3, 5, 11] = 1
    idx, counts = R.gap_index(mask)
    hole = torch.from_numpy(mask.reshape(B, -1) == 0)
    assert counts.tolist() == hole.sum(1).tolist() and idx.shape == (B, counts.max())
    vals = rng.standard_normal((B, F * T)).astype(np.float32)
    g = R.gather(vals, idx)
    for b in range(B):
        assert np.array_equal(idx[b, :counts[b]], torch.nonzero(hole[b])[:, 0].numpy()) and np.all(idx[b, counts[b]:] == -1)
        assert np.array_equal(g[b, :counts[b]], vals[b][hole[b].numpy()]) and np.all(g[b, counts[b]:] == 0)
        full = torch.zeros(F * T)
        full.masked_scatter_(hole[b], torch.from_numpy(g[b, :counts[b]]))
        assert np.array_equal(R.scatter(g, idx, F * T)[b], full.numpy())
    assert R.scatter(np.stack([g, 2 * g], axis=1), idx, F * T).shape == (B, 2, F * T)


@pytest.mark.parametrize("K,n", [(2, 1), (7, 5), (60, 8)])
def test_ragged_restatement_equals_the_uniform_oracle_item_by_item(K, n):
    """pca_ragged's item b == oracle pca_batch on stack[:, b, :counts[b]] alone.  The two round the mean differently (fp64
    sum rounded once against torch's fp32 mean: up to an fp32 ulp of the data, 6e-8 relative), which moves a component by
    about that over the relative gap of its singular value (1/2 here): the limits are those of the GPU comparison."""
    rng = np.random.default_rng(10 * K + n)
    counts = [1, 63, 64, 65, 130]
    Nmax = max(counts)
    stack = np.zeros((K, len(counts), Nmax), dtype=np.float32)
    for b, c in enumerate(counts):
        stack[:, b, :c] = separated_stack(rng, K, c)
    comps, scaled, weights, mean, svals = R.pca_ragged(stack, counts, n)
    for b, c in enumerate(counts):
        q = min(n, c)                                      # the SVD of a K x c matrix has min(K, c) pairs: 1 for c = 1
        o = [t.numpy() for t in O.pca_batch(torch.from_numpy(stack[:, b:b + 1, :c]), q)]
        m = min(n, K - 1, c)                               # components with a non-zero singular value have a direction
        assert o[4].shape[1] == q and m == (1 if c == 1 else n)
        assert np.abs(comps[b, :m, :c] - o[0][0, :m]).max() < 5e-6
        assert np.abs(svals[b, :q] - o[4][0]).max() < 1e-6 * o[4].max() and np.abs(svals[b, q:]).sum() < 1e-6 * o[4].max()
        assert np.abs(scaled[b, :q, :c] - o[1][0]).max() < 5e-6 * o[4].max()
        assert np.abs(scaled[b, q:]).sum() < 5e-6 * o[4].max()
        assert np.abs(mean[b, :c] - o[3][0]).max() < 1e-6 * np.abs(o[3]).max() + 1e-7
        assert np.abs(weights[b, :q] - o[2][0]).max() < 1e-6
        assert np.all(comps[b, :, c:] == 0) and np.all(scaled[b, :, c:] == 0) and np.all(mean[b, c:] == 0)


def test_wrappers_refuse_bad_gaps_and_counts_before_asking_for_a_device():
    from nppc_audio.inpainting import mc_baseline as MB
    mask = torch.ones(3, 1, 8, 21)
    mask[0, :, :, 3] = 0
    mask[2, :, :, 5:7] = 0                                                       # item 1 has no gap
    with pytest.raises(ValueError, match="item 1 has no gap"):
        MB.gap_index(mask)
    with pytest.raises(ValueError, match="item 1 has no gap"):
        MB.mc_dropout_samples_ragged(None, mask, mask, 2)
    with pytest.raises(ValueError, match="item 1 has no gap"):
        MB.calculate_unet_baseline_ragged(None, mask, mask, 2, 1)
    stack = torch.zeros(4, 3, 16)
    with pytest.raises(ValueError, match="item 2 has no gap"):
        MB.compute_pca_ragged(stack, torch.tensor([16, 3, 0]), 2)
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        MB.compute_pca_ragged(stack, [16, 3], 2)
    with pytest.raises(ValueError, match=r"counts\[1\] = 17 exceeds the padded width 16"):
        MB.compute_pca_ragged(stack, [16, 17, 1], 2)
    with pytest.raises(ValueError, match="stack"):
        MB.compute_pca_ragged(torch.zeros(4, 16), [16], 2)


def header_functions():
    txt = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): [a for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(nppc_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_new_symbols_are_declared_bound_exported_and_check_their_arguments():
    from nppc_audio import _hip as H
    fns = header_functions()
    for name in ("nppc_gap_count", "nppc_gap_index", "nppc_gap_gather", "nppc_gap_scatter", "nppc_pca_ragged_work_elems",
                 "nppc_pca_ragged"):
        assert name in fns and len(fns[name]) == len(H.SIGS[name]), name
        assert hasattr(H.lib(), name), f"{name} not exported by libnppc_hip.so"
    n = ctypes.c_long()
    H.call("nppc_pca_ragged_work_elems", 50, 16, 130, 5, ctypes.byref(n))
    assert n.value == 16 * (50 * 50 + 5 + 5 * 50 + 3 * (50 * 51 // 2))          # G, eval, evec, 3 chunks of 64 x upper triangle
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_pca_ragged_work_elems", 50, 16, 0, 5, ctypes.byref(n))
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def rc(name, *args):
        fn = getattr(H.lib(), name)
        fn.argtypes, fn.restype = H.SIGS[name], ctypes.c_int
        return fn(*args)
    # refused before any launch: null pointers, empty shapes, more room than elements
    assert rc("nppc_gap_count", null, p, 1, 8, null) == 1 and rc("nppc_gap_count", p, p, 0, 8, null) == 1
    assert rc("nppc_gap_count", p, p, 1, 1 << 31, null) == 1                     # positions are int32
    assert rc("nppc_gap_index", p, null, 1, 8, 4, null) == 1 and rc("nppc_gap_index", p, p, 1, 8, 9, null) == 1
    assert rc("nppc_gap_index", p, p, 1, 8, 0, null) == 1
    assert rc("nppc_gap_gather", p, p, null, 1, 8, 4, null) == 1 and rc("nppc_gap_gather", p, p, p, 1, 8, 9, null) == 1
    assert rc("nppc_gap_scatter", p, p, p, 1, 0, 8, 4, null) == 1 and rc("nppc_gap_scatter", null, p, p, 1, 1, 8, 4, null) == 1
    ok = [p, p, 4, 1, 8, 2, p, p, p, p, p, p, null]                              # X, counts, K, B, Nmax, n, outputs, work
    for i, v in ((0, null), (1, null), (11, null), (3, 0), (4, 0), (5, 0)):
        bad = list(ok)
        bad[i] = v
        assert rc("nppc_pca_ragged", *bad) == 1, i
    for i, v in ((2, 1), (2, 61), (5, 5), (5, 9)):                               # the limits of nppc_pca_batch
        bad = list(ok)
        bad[i] = v
        if (i, v) == (5, 9):
            bad[2] = 20
        assert rc("nppc_pca_ragged", *bad) == 3, (i, v)


def test_keyword_is_off_by_default():
    import inspect
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer
    from nppc_audio.inpainting.validator.validator_nppc_model import NPPCModelValidator
    for fn in (NPPCModelValidator.validate_batch, NPPCModelValidator.validate_dataloader, NPPCAudioInpaintingTrainer.base_step2):
        assert inspect.signature(fn).parameters["ragged_gaps"].default is False
