"""GPU: the speech-enhancement metric kernels (csrc/se_metrics.hip through nppc_audio.metrics) against the fp64 oracle
(tests/se_metrics_ref.py) and the reference's recorded SI-SDRs: SI-SDR of both definitions, STOI stage by stage on a
ragged batch, garbage in the padding, batch independence and run-to-run bit identity."""
import numpy as np
import pytest
import torch

import se_metrics_ref as R
from test_se_metrics_cpu import golden_pairs

pytestmark = pytest.mark.gpu

# limits: <= 2x the measured worst on the MI355X (profiles/se_metrics_parity_errors.json).  The issue's budgets were 1e-6 dB,
# 2e-6, 1e-5 and 2e-5; everything after the fp32 input is fp64 here, so the kernels agree with the oracle to a few ulps.
GOLDEN_SISDR_DB = 1.9e-12     # measured 9.7e-13 (mean-removed definition)
SISDR_DB = 7.5e-8             # measured 3.8e-8: mean-removed SI-SDR of an exact copy (~140 dB, residual ~1e-7 of the signal)
RESAMPLE_ABS = 6.6e-16        # measured 3.3e-16
TOB_REL = 1.4e-15             # measured 7.3e-16
STOI_ABS = 4.4e-16            # measured 2.2e-16
GARBAGE = 3.0e38


def padded(pairs, garbage=GARBAGE):
    """[B, Lmax] fp32 device rows with the tail past each length filled with +-garbage"""
    lens = [len(r) for r, _ in pairs]
    Lm = max(lens)
    sign = np.where(np.arange(Lm) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(garbage)
    ref = np.tile(sign, (len(pairs), 1))
    est = -ref.copy()
    for b, (r, e) in enumerate(pairs):
        ref[b, :len(r)], est[b, :len(e)] = r, e
    return torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


def batch_pairs():
    clean, est, lens = R.ragged_batch()
    return [(clean[b, :n], est[b, :n]) for b, n in enumerate(lens)]


@pytest.fixture(scope="module")
def oracle_stages():
    return [R.stoi_stages(c, e) for c, e in batch_pairs()]


def check_sisdr(pairs, got, record_err, tag):
    got = got.cpu().numpy()
    worst = [0.0, 0.0]
    for b, (r, e) in enumerate(pairs):
        for col, fn in enumerate((R.si_sdr, R.si_sdr_zero_mean)):
            want = fn(r, e)
            if np.isinf(want):
                assert np.isinf(got[b, col]) and np.sign(got[b, col]) == np.sign(want), (b, col, got[b, col])
            else:
                worst[col] = max(worst[col], abs(got[b, col] - want))
    record_err(f"{tag}_si_sdr_db", worst[0], SISDR_DB)
    record_err(f"{tag}_si_sdr_zero_mean_db", worst[1], SISDR_DB)


def test_si_sdr_matches_reference_goldens(record_err):
    from nppc_audio import metrics as M
    pairs, z = golden_pairs()
    ref, est, lens = padded(pairs)
    got = M.si_sdr_both(ref, est, lengths=lens).cpu().numpy()
    for b in range(len(pairs)):
        if np.isinf(z["si_sdr"][b]):
            assert np.isinf(got[b, 0]) and got[b, 0] > 0
    fin = np.isfinite(z["si_sdr"])
    record_err("golden_si_sdr_db", np.abs(got[fin, 0] - z["si_sdr"][fin]).max(), GOLDEN_SISDR_DB)
    record_err("golden_si_sdr_zero_mean_db", np.abs(got[:, 1] - z["si_sdr_zero_mean"]).max(), GOLDEN_SISDR_DB)
    # the public per-definition functions are the two columns
    assert torch.equal(M.si_sdr(ref, est, lengths=lens).cpu(), torch.from_numpy(got[:, 0]))
    assert torch.equal(M.si_sdr_zero_mean(ref, est, lengths=lens).cpu(), torch.from_numpy(got[:, 1]))


def test_si_sdr_ragged_batch_matches_oracle(record_err):
    from nppc_audio import metrics as M
    pairs = batch_pairs()
    pairs[3] = (pairs[3][0], pairs[3][0].copy())                  # an exact copy: +inf for the audio_zen definition
    ref, est, lens = padded(pairs)
    check_sisdr(pairs, M.si_sdr_both(ref, est, lengths=lens), record_err, "ragged")


def test_stoi_stages_match_oracle(oracle_stages, record_err):
    from nppc_audio import metrics as M
    pairs = batch_pairs()
    ref, est, lens = padded(pairs)
    st = M.stoi_stages(ref, est, lengths=lens)
    got = {k: v.cpu().numpy() for k, v in st.items()}
    w_rs = w_tob = w_stoi = 0.0
    for b, (o, (c, e)) in enumerate(zip(oracle_stages, pairs)):
        n = o["xr"].size
        assert got["lr"][b] == n
        w_rs = max(w_rs, np.abs(got["xr"][b, :n] - o["xr"]).max(), np.abs(got["yr"][b, :n] - o["yr"]).max())
        nf = o["mask"].size
        assert np.abs(o["margin"]).min() > 1e-3, "input frame energy too close to the silence threshold"
        np.testing.assert_array_equal(got["slot"][b, :nf] >= 0, o["mask"])
        assert (got["slot"][b, nf:] == -1).all()
        assert got["K"][b] == o["K"]
        np.testing.assert_array_equal(got["kidx"][b, :o["K"]], np.flatnonzero(o["mask"]))
        T = o["x_tob"].shape[1]
        for g, want in ((got["x_tob"][b, :, :T], o["x_tob"]), (got["y_tob"][b, :, :T], o["y_tob"])):
            w_tob = max(w_tob, np.abs(g - want).max() / np.abs(want).max())
        w_stoi = max(w_stoi, abs(got["stoi"][b] - o["stoi"]))
    assert got["stoi"][0] == 1e-5                                  # 0.3 s: fewer than 30 frames
    assert all(o["stoi"] > 0.5 for o in oracle_stages[1:])
    record_err("resampled_abs", w_rs, RESAMPLE_ABS)
    record_err("band_magnitude_rel", w_tob, TOB_REL)
    record_err("stoi_abs", w_stoi, STOI_ABS)


def test_items_are_independent_of_batch_and_padding():
    from nppc_audio import metrics as M
    pairs = batch_pairs()
    ref, est, lens = padded(pairs)
    s1, d1 = M.stoi(ref, est, lengths=lens), M.si_sdr_both(ref, est, lengths=lens)
    s2, d2 = M.stoi(ref, est, lengths=lens), M.si_sdr_both(ref, est, lengths=lens)
    assert torch.equal(s1, s2) and torch.equal(d1, d2)                      # run to run
    ref0, est0, lens0 = padded(pairs, garbage=0.0)
    assert torch.equal(M.stoi(ref0, est0, lengths=lens0), s1)               # whatever the padding holds
    assert torch.equal(M.si_sdr_both(ref0, est0, lengths=lens0), d1)
    for b, (c, e) in enumerate(pairs):                                      # alone, no padding at all
        x, y = torch.from_numpy(c).cuda(), torch.from_numpy(e).cuda()
        assert torch.equal(M.stoi(x, y), s1[b:b + 1]), b
        assert torch.equal(M.si_sdr_both(x, y), d1[b:b + 1]), b
    assert torch.isfinite(s1).all() and torch.isfinite(d1).all()


def test_stoi_edge_cases():
    from nppc_audio import metrics as M
    x = torch.from_numpy(batch_pairs()[1][0]).cuda()
    one = M.stoi(x, x)
    assert abs(float(one) - 1.0) < 1e-9
    assert abs(float(M.stoi(x, 0.3 * x)) - 1.0) < 1e-7                   # 0.3 x is rounded to fp32
    tiny = torch.zeros(2, 200, device="cuda")                               # no frame at all
    assert M.stoi(tiny, tiny).tolist() == [1e-5, 1e-5]
