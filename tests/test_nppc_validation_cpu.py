"""CPU: the host half of the NPPC validation: nppc_direction_scores against a plain-loop restatement, the
new C-ABI symbols in the header and in the ctypes table, the validation bench's host logic, and the loud failure without a
GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from nppc_validation_ref import direction_scores_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"nppc_rawmag_stage_ragged": 10, "nppc_gram_ragged_work_elems": 5, "nppc_gram_ragged": 12,
               "nppc_combine_ragged": 9, "nppc_cirm_build_compress_ragged": 11}


def loss_terms(B, K, seed):
    """per-item loss outputs of random orthogonal directions and a random error, fp64 (trainer.py:259-298 in numpy)"""
    rng = np.random.default_rng(seed)
    N = 40
    en, pm, wn, rec = [], [], [], []
    for _ in range(B):
        q, _ = np.linalg.qr(rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K)))
        w = q.T * rng.uniform(0.1, 3.0, size=(K, 1))                       # orthogonal rows of different norms
        e = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        e_n = np.linalg.norm(e)
        p = np.array([np.vdot(w[k], e) / (np.linalg.norm(w[k]) * e_n) for k in range(K)])
        en.append(e_n), pm.append(np.abs(p)), wn.append(np.linalg.norm(w, axis=1) / e_n), rec.append(1 - (np.abs(p) ** 2).sum())
    return np.array(en), np.array(pm), np.array(wn), np.array(rec), N


@pytest.mark.parametrize("B,K", [(1, 1), (7, 3), (32, 5)])
def test_direction_scores_match_the_restatement_and_the_loss(B, K):
    from nppc_audio.metrics import nppc_direction_scores
    en, pm, wn, rec, N = loss_terms(B, K, 10 * B + K)
    got = nppc_direction_scores(en, pm, wn)
    ref = direction_scores_np(en, pm, wn)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == np.float64
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-13, atol=1e-15, err_msg=k)
    # the identity with the loss: the residual of all K directions IS reconst_err (the loss's normalisation: per |e|^2), and
    # residual * |e|^2 is the squared error left outside the span of the directions
    np.testing.assert_allclose(got["residual"][:, -1], rec, rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["residual_mean"][-1], rec.mean(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["residual_pooled"][-1], (rec * en ** 2).sum() / (en ** 2).sum(), rtol=1e-13)
    assert np.all(np.diff(got["captured"], axis=1) >= 0) and np.all(got["captured"] <= 1 + 1e-12)
    # float32 device outputs, torch tensors and lists are all taken
    g32 = nppc_direction_scores(torch.from_numpy(en).float(), torch.from_numpy(pm).float(), wn.astype(np.float32).tolist())
    np.testing.assert_allclose(g32["calibration"], got["calibration"], rtol=1e-6)


def test_direction_scores_calibration_and_shape_errors():
    from nppc_audio.metrics import nppc_direction_scores
    en, pm, wn, _, _ = loss_terms(6, 2, 3)
    s = nppc_direction_scores(en, pm, pm)                                   # predicted spread = observed: calibrated
    np.testing.assert_allclose(s["calibration"], 1.0, rtol=1e-14)
    np.testing.assert_allclose(nppc_direction_scores(en, pm, 2 * pm)["calibration"], 0.5, rtol=1e-14)
    for bad in ((en[:3], pm, wn), (en, pm[:, :1], wn), (en, pm[0], wn[0]), (en[:0], pm[:0], wn[:0])):
        with pytest.raises(ValueError):
            nppc_direction_scores(*bad)


def header_functions():
    txt = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): [a for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(nppc_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_new_symbols_are_declared_bound_and_exported():
    from nppc_audio import _hip
    fns = header_functions()
    for name, arity in NEW_SYMBOLS.items():
        assert name in fns, f"{name} missing from include/nppc_hip.h"
        assert len(fns[name]) == arity == len(_hip.SIGS[name]), name
        assert hasattr(_hip.lib(), name), f"{name} not exported by libnppc_hip.so"
    import ctypes
    n = ctypes.c_long()
    _hip.call("nppc_gram_ragged_work_elems", 3, 5, 1, 257, ctypes.byref(n))
    assert n.value == 3 * 65 * 21 * 2                                       # B x ceil(F / 4) row groups x 6 * 7 / 2 entries x (re, im)
    with pytest.raises(RuntimeError, match="bad argument"):                 # null pointers are refused before any launch
        _hip.call("nppc_gram_ragged", None, None, None, None, None, 0, None, 1, 1, 1, 1, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_combine_ragged", None, None, None, None, 1, 1, 1, 1, None)


def _tool():
    spec = importlib.util.spec_from_file_location("bench_nppc_validation", os.path.join(ROOT, "tools", "bench_nppc_validation.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_validation_bench_plans_batches_and_needs_a_gpu():
    t = _tool()
    lengths = t.clip_lengths(10, 1.0, 6.0, 0)
    assert lengths == t.clip_lengths(10, 1.0, 6.0, 0) and all(16000 <= n <= 96000 for n in lengths)
    groups, pad = t.plan_batches(lengths, 4, "sorted")
    assert sorted(i for g in groups for i in g) == list(range(10)) and [len(g) for g in groups] == [4, 4, 2]
    assert all(lengths[a] <= lengths[b] for g in groups for a, b in zip(g, g[1:]))
    _, pad_ds = t.plan_batches(lengths, 4, "dataset")
    assert 0 <= pad <= pad_ds < 1
    assert t.plan_batches(lengths, 1, "dataset")[1] == 0.0                  # one clip per batch: nothing is padded
    assert t.plan_batches([2560, 256], 2, "sorted")[1] == pytest.approx(1 - 13 / 22)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            t.main(["--clips", "2", "--batches", "2", "--max-s", "1.0"])


def test_ragged_entry_points_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return
    from nppc_audio import pc_ops
    with pytest.raises(RuntimeError, match="HIP"):
        pc_ops.gram_schmidt_to_crm_ragged(torch.zeros(1, 2, 2, 3, 4), torch.tensor([4], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP"):
        pc_ops.nppc_loss_ragged(torch.zeros(1, 2, 2, 3, 4), torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4),
                                torch.tensor([4], dtype=torch.int32), 1.0)
