"""GPU: the BSS-eval SDR kernels (csrc/bss_eval.hip through nppc_audio.metrics.sdr_stages / sdr / scale_bss_eval) against
the fp64 restatement of their contract (tests/bss_eval_ref.py), stage by stage on ragged batches whose lengths sit on the
kernels' chunk boundaries; independence of the batch and of the padding, run-to-run bit identity, the edge cases, and the
extra_metrics path of ModelValidator.

Limits (none of them comes from what the kernels give):
- r, d: 1e-11 sqrt(r[0] sum e^2), i.e. five times the worst-case bound (M - 1) 2^-53 = 1.8e-12 of an fp64 sum of
  M <= 16511 products in any order;
- c: not compared element-wise (ill-conditioned by nature); its residual |toeplitz(r) c - d| / |d| must not exceed 100
  times the residual of the same recursion in numpy;
- num, den: 1e-9 relative;
- SDR: max(1e-9 dB, 100 x the spread of LU / lstsq / scipy's Levinson on that item);
- an item whose estimate lies in the span exactly (n = 1, or est == ref) has den = rounding noise: +inf or above 250 dB.
Measured on the MI355X: the worst SDR difference is 2.5e-13 dB, est == ref gives +inf (den == 0 exactly) and the
delayed, halved copy 303.8 dB; see DESIGN.md section 7d.
"""
import functools

import numpy as np
import pytest
import torch

import bss_eval_ref as R
from test_bss_eval_cpu import all_cases, exact_in_span

pytestmark = pytest.mark.gpu

CORR_MARGIN = 1e-11
SUMS_REL = 1e-9
SDR_DB = 1e-9
SCALE_DB = 1e-9
KEYS = ("r", "d", "c", "num", "den", "sdr")


def case_id(case):
    lengths, P = case
    return f"P{P}-" + "_".join(str(n) for n in lengths)


CASE_LIST = all_cases()
CASE_IDS = [case_id(c) for c in CASE_LIST]


@functools.lru_cache(maxsize=None)
def oracle(case):
    """per item of the case: the pair, the restatement's stages, the host solvers' spread and the host Levinson residual;
    computed once and shared by every test"""
    lengths, P = case
    out = []
    for (s, e), n in zip(R.make_batch(lengths, seed0=P), lengths):
        st = R.sdr_stages(s, e, P)
        exact = exact_in_span(n, P)
        spread = 0.0 if exact else R.solver_spread(s, e, P)
        lev = R.levinson(st["r"], st["d"])
        out.append(dict(s=s, e=e, n=n, st=st, exact=exact, spread=spread, lev_res=R.residual(st["r"], st["d"], lev)))
    return out


def padded(items, fill=np.nan):
    """[B, Lmax] fp32 device rows, everything past each length = fill"""
    lens = [it["n"] for it in items]
    ref = np.full((len(items), max(lens)), fill, np.float32)
    est = ref.copy()
    for b, it in enumerate(items):
        ref[b, :it["n"]], est[b, :it["n"]] = it["s"], it["e"]
    return torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in KEYS)


def check_item(got, b, it, P, record_err, tag):
    st = it["st"]
    r, d, c = got["r"][b], got["d"][b], got["c"][b]
    e2 = float(np.sum(it["e"].astype(np.float64) ** 2))
    lim = CORR_MARGIN * np.sqrt(st["r"][0] * e2)
    print(f"{tag}: n {it['n']} r err {np.abs(r - st['r']).max():.3e} d err {np.abs(d - st['d']).max():.3e} limit {lim:.3e}")
    record_err(f"{tag}_r_over_limit", np.abs(r - st["r"]).max() / lim, 1.0)
    record_err(f"{tag}_d_over_limit", np.abs(d - st["d"]).max() / lim, 1.0)
    assert got["status"][b] == 0
    res = R.residual(r, d, c)
    print(f"{tag}: residual {res:.3e} host Levinson {it['lev_res']:.3e}")
    record_err(f"{tag}_residual_over_host", res / (100.0 * it["lev_res"]) if it["lev_res"] > 0 else res, 1.0)
    if it["exact"]:
        assert st["sdr"] > 250.0
        assert got["sdr"][b] > 250.0, got["sdr"][b]                 # +inf included
        return
    print(f"{tag}: num rel {abs(got['num'][b] / st['num'] - 1):.3e} den rel {abs(got['den'][b] / st['den'] - 1):.3e} "
          f"sdr diff {abs(got['sdr'][b] - st['sdr']):.3e} dB spread {it['spread']:.3e} dB")
    record_err(f"{tag}_num_rel", abs(got["num"][b] / st["num"] - 1), SUMS_REL)
    record_err(f"{tag}_den_rel", abs(got["den"][b] / st["den"] - 1), SUMS_REL)
    record_err(f"{tag}_sdr_db", abs(got["sdr"][b] - st["sdr"]), max(SDR_DB, 100.0 * it["spread"]))


def to_numpy(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


@pytest.mark.parametrize("case", CASE_LIST, ids=CASE_IDS)
def test_ragged_batch_stages_match_restatement(case, record_err):
    from nppc_audio import metrics as M
    lengths, P = case
    items = oracle(case)
    ref, est, lens = padded(items)
    got = to_numpy(M.sdr_stages(ref, est, lengths=lens, filter_length=P))
    assert got["r"].shape == (len(items), P) and got["sdr"].dtype == np.float64
    for b, it in enumerate(items):
        check_item(got, b, it, P, record_err, f"item{b}")


@pytest.mark.parametrize("case", CASE_LIST, ids=CASE_IDS)
def test_uniform_batch_and_1d_input(case, record_err):
    """lengths=None: every item of the case twice in a uniform [2, n] batch, and alone as a 1-D tensor"""
    from nppc_audio import metrics as M
    lengths, P = case
    for i, it in enumerate(oracle(case)):
        s, e = torch.from_numpy(it["s"]).cuda(), torch.from_numpy(it["e"]).cuda()
        two = M.sdr_stages(torch.stack((s, s)), torch.stack((e, e)), filter_length=P)
        got = to_numpy(two)
        check_item(got, 0, it, P, record_err, f"uniform{i}")
        for k in KEYS:
            assert torch.equal(bits(two[k][0]), bits(two[k][1])), k
        one = M.sdr_stages(s, e, filter_length=P)
        assert one["sdr"].shape == (1,) and one["r"].shape == (1, P)
        for k in KEYS:
            assert torch.equal(bits(one[k][0]), bits(two[k][0])), k


@pytest.mark.parametrize("case", CASE_LIST, ids=CASE_IDS)
def test_items_do_not_depend_on_batch_padding_or_run(case):
    from nppc_audio import metrics as M
    lengths, P = case
    items = oracle(case)
    ref, est, lens = padded(items, fill=np.nan)
    a = M.sdr_stages(ref, est, lengths=lens, filter_length=P)
    b = M.sdr_stages(ref, est, lengths=lens, filter_length=P)
    assert same_bits(a, b)                                                    # run to run
    ref0, est0, lens0 = padded(items, fill=0.25)
    assert same_bits(a, M.sdr_stages(ref0, est0, lengths=lens0, filter_length=P))      # whatever the padding holds
    assert not torch.isnan(a["r"]).any() and not torch.isnan(a["c"]).any() and not torch.isnan(a["sdr"]).any()
    for i, it in enumerate(items):                                            # alone, no padding at all
        s, e = torch.from_numpy(it["s"]).cuda(), torch.from_numpy(it["e"]).cuda()
        one = M.sdr_stages(s, e, filter_length=P)
        for k in KEYS:
            assert torch.equal(bits(one[k][0]), bits(a[k][i])), (i, k)
    # in another order, with a host list of lengths
    perm = list(range(len(items)))[::-1]
    c = M.sdr_stages(ref[perm], est[perm], lengths=[items[p]["n"] for p in perm], filter_length=P)
    for k in KEYS:
        assert torch.equal(bits(c[k]), bits(a[k][perm])), k
    assert torch.equal(bits(M.sdr(ref, est, lengths=lens, filter_length=P)), bits(a["sdr"]))


def test_default_filter_length_and_registered_metric():
    from nppc_audio import metrics as M
    case = CASE_LIST[2]
    assert case[1] == 512
    items = oracle(case)
    ref, est, lens = padded(items)
    want = M.sdr(ref, est, lengths=lens, filter_length=512)
    assert torch.equal(bits(M.sdr(ref, est, lengths=lens)), bits(want))
    assert torch.equal(bits(M.REGISTERED_METRICS["SDR"](ref, est, sr=16000, lengths=lens)), bits(want))


def test_delay_and_gain_are_forgiven():
    from nppc_audio import metrics as M
    s, _ = R.make_pair(11, 4000)
    s[-3:] = 0.0
    e = np.concatenate((np.zeros(3, np.float32), 0.5 * s[:-3]))
    x, y = torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda()
    got = float(M.sdr(x, y, filter_length=64))
    print(f"delayed and scaled copy: SDR {got} dB, SI-SDR {float(M.si_sdr(x, y))} dB")
    assert got > 200.0
    assert float(M.si_sdr(x, y)) < 10.0
    c = M.sdr_stages(x, y, filter_length=64)["c"][0].cpu().numpy()
    assert abs(c[3] - 0.5) < 1e-9 and np.abs(np.delete(c, 3)).max() < 1e-9


def test_edge_cases():
    from nppc_audio import metrics as M
    items = [dict(it) for it in oracle(CASE_LIST[0])[:3]]
    items[1]["s"] = np.zeros_like(items[1]["s"])                  # an all-zero reference
    items[2]["e"] = items[2]["s"].copy()                          # an exact copy
    ref, est, lens = padded(items)
    st = M.sdr_stages(ref, est, lengths=lens, filter_length=8)
    got = st["sdr"].cpu().numpy()
    want0 = oracle(CASE_LIST[0])[0]["st"]["sdr"]
    assert abs(got[0] - want0) < SDR_DB
    assert np.isnan(got[1]) and st["status"].tolist() == [0, 1, 0]
    assert np.isnan(st["num"][1].item()) and np.isnan(st["den"][1].item())
    print(f"est == ref: SDR {got[2]} dB")
    assert got[2] > 250.0                                         # +inf or finite: both are what the explicit residual permits
    # an all-zero estimate: proj = 0, num = den = 0 -> +inf by the contract's den == 0 rule
    z = M.sdr(ref[:1], torch.zeros_like(est[:1]), lengths=lens[:1], filter_length=8)
    assert torch.isinf(z).all() and (z > 0).all()
    with pytest.raises(ValueError):
        M.sdr(ref, est[:, :-1], lengths=lens)
    with pytest.raises(ValueError):
        M.sdr(ref, est, lengths=[1, 2])


def scale_pairs():
    pairs = [R.make_pair(40 + i, n) for i, n in enumerate((3000, 257, 1025, 2))]
    rng = np.random.default_rng(9)
    ac = rng.standard_normal(2000)
    s = (100.0 + ac).astype(np.float32)                           # a DC offset 100 x the AC level
    e = (100.0 + 0.9 * ac + 0.1 * rng.standard_normal(2000)).astype(np.float32)
    pairs.append((s, e))
    return pairs


def test_scale_bss_eval_matches_restatement(record_err):
    from nppc_audio import metrics as M
    pairs = scale_pairs()
    items = [dict(s=s, e=e, n=len(s)) for s, e in pairs]
    ref, est, lens = padded(items)
    got = M.scale_bss_eval(ref, est, lengths=lens, return_sums=True)
    assert set(got) == {"si_sdr", "sd_sdr", "snr", "srr", "sums"}
    again = M.scale_bss_eval(ref, est, lengths=lens)
    assert set(again) == {"si_sdr", "sd_sdr", "snr", "srr"}
    for k in again:
        assert again[k].shape == (len(pairs),) and again[k].dtype == torch.float64
        assert torch.equal(bits(again[k]), bits(got[k]))
    worst = {k: 0.0 for k in again}
    for b, (s, e) in enumerate(pairs):
        want = R.scale_bss_eval(s, e)
        for k in worst:
            worst[k] = max(worst[k], abs(float(got[k][b]) - want[k]))
        one = M.scale_bss_eval(torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda())
        for k in worst:
            assert torch.equal(bits(one[k]), bits(got[k][b:b + 1])), (b, k)
        s64, e64 = s.astype(np.float64), e.astype(np.float64)
        sums = got["sums"][b].cpu().numpy()
        np.testing.assert_allclose(sums[:3], [np.sum(s64 ** 2), np.dot(s64, e64), np.sum((e64 - s64) ** 2)], rtol=1e-12)
    for k, v in worst.items():
        print(f"scale_bss_eval {k}: worst {v:.3e} dB")
        record_err(f"{k}_db", v, SCALE_DB)
    # the si_sdr of _scale_bss_eval is audio_zen's SI_SDR
    assert float((got["si_sdr"] - M.si_sdr(ref, est, lengths=lens)).abs().max()) < SCALE_DB


def test_model_validator_extra_metrics(tmp_path):
    from nppc_audio import metrics as M
    from test_model_validator_gpu import make_validator
    mv = make_validator(tmp_path)
    items = oracle(CASE_LIST[1])
    ref, est, lens = padded(items, fill=0.0)
    base = mv.calculate_metrics_batch(ref, est, lengths=lens)
    assert set(base) == {"STOI", "SI_SDR"}
    m = mv.calculate_metrics_batch(ref, est, lengths=lens, extra_metrics=("SDR",))
    assert set(m) == {"STOI", "SI_SDR", "SDR"}
    assert torch.equal(bits(m["SDR"]), bits(M.sdr(ref, est, lengths=lens)))
    assert torch.equal(bits(m["STOI"]), bits(base["STOI"])) and torch.equal(bits(m["SI_SDR"]), bits(base["SI_SDR"]))
    one = mv.calculate_metrics(items[0]["s"], items[0]["e"], extra_metrics=("SDR",))
    assert set(one) == {"STOI", "SI_SDR", "SDR"} and one["SDR"] == float(m["SDR"][0])
    assert set(mv.calculate_metrics(items[0]["s"], items[0]["e"])) == {"STOI", "SI_SDR"}
    with pytest.raises(ValueError, match="MOSNET"):
        mv.calculate_metrics_batch(ref, est, lengths=lens, extra_metrics=("MOSNET",))
