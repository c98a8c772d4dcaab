"""CPU: the FLAC encoder's predictor "lpc".  The restatement tests/flac_lpc_ref.py writes streams that decode to the samples;
the serial host encoder (csrc/flac_enc_core.h through nppc_flac_encode_host_lpc and flac.encode_pcm(backend="host")) gives
its bytes; no stream is longer than the fixed predictors' stream of the same input, and the voiced one is shorter and made
of LPC subframes; the default predictor's bytes are what they were; refusals come before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flac_enc_cases as K
import flac_lpc_cases as C
import flac_lpc_ref as L
import flac_ref as R
from nppc_audio import _hip as H
from nppc_audio import flac
from test_flac_encode_cpu import check_stream

ALL = [(b, c.name) for b in (16, 24) for c in C.cases(b)]
IDS = [f"{b}-{n}" for b, n in ALL]


def encode_host_raw(pcm, bps, rate, block_size, max_order):
    """straight through the C entry point"""
    pcm = np.ascontiguousarray(pcm, np.int32)
    cap, frames = ctypes.c_long(), ctypes.c_long()
    H.call("nppc_flac_enc_bound", pcm.shape[1], pcm.shape[0], bps, block_size, ctypes.byref(cap), ctypes.byref(frames))
    out = np.full(cap.value, 0xA5, np.uint8)
    n = ctypes.c_long()
    H.call("nppc_flac_encode_host_lpc", pcm.ctypes.data, pcm.shape[1], pcm.shape[0], bps, rate, block_size, max_order,
           out.ctypes.data, cap.value, ctypes.byref(n))
    assert 0 < n.value <= cap.value
    return out[:n.value].tobytes()


def frame_lengths(data):
    info = R.probe(data)
    off, count, sizes = info["first_frame"], 0, []
    while count < info["total_samples"]:
        hdr = R.parse_header(data, off, info)
        _, end = R.decode_frame(data, off, info, hdr)
        sizes.append(end - off)
        count, off = count + hdr["bs"], end
    return sizes


@pytest.mark.parametrize("bps,name", ALL, ids=IDS)
def test_the_restatement_decodes_and_the_host_encoder_equals_it(bps, name):
    case = C.case(bps, name)
    want, _ = C.reference(bps, name)
    check_stream(want, case)                                          # flac_ref.decode, the host decoder, STREAMINFO, the MD5
    got = encode_host_raw(case.pcm, bps, case.rate, case.block_size, case.max_order)
    assert got == want
    assert flac.encode_pcm([torch.from_numpy(case.pcm)], bps, case.rate, case.block_size, backend="host", predictor="lpc",
                           max_lpc_order=case.max_order) == [want]


@pytest.mark.parametrize("bps,name", ALL, ids=IDS)
def test_no_frame_is_longer_than_the_fixed_predictors_frame(bps, name):
    lpc, fixed = C.reference(bps, name)[0], C.fixed_reference(bps, name)
    assert len(lpc) <= len(fixed)
    assert all(a <= b for a, b in zip(frame_lengths(lpc), frame_lengths(fixed)))


def subframes(bps, name):
    return [s for f in C.reference(bps, name)[1] for s in f["subframes"]]


def test_the_plans_take_every_path():
    for bps in (16, 24):
        voiced = subframes(bps, "voiced_m8")
        assert all(s["type"] == "lpc" and s["precision"] == L.precision(bps) for s in voiced)
        assert max(s["order"] for s in voiced) > 4                    # not the fixed predictors under another name
        assert len(C.reference(bps, "voiced_m8")[0]) < 0.8 * len(C.fixed_reference(bps, "voiced_m8"))
        assert C.reference(bps, "voiced_m1")[0] == C.fixed_reference(bps, "voiced_m1")          # order 1 loses to fixed 4
        assert {s["type"] for s in subframes(bps, "main")} == {"lpc", "constant", "verbatim"}
        assert [s["type"] for s in subframes(bps, "ramp")] == ["fixed"]                          # fixed must still win
        assert {f["assign"] for f in C.reference(bps, "stereo")[1]} == {0, 1, 2, 3}
        assert [s["type"] for s in subframes(bps, "edge1")] == ["fixed", "constant"]              # r_0 = 0: no LPC candidates
        assert C.reference(bps, "edge1")[0] == C.fixed_reference(bps, "edge1")
        assert {(s["type"], s["order"]) for s in subframes(bps, "alternating")} == {("lpc", 1)}
        for n in (1, 2, 13, 16, 17):
            assert C.reference(bps, f"n{n}")[0] == C.fixed_reference(bps, f"n{n}")              # costed, never cheaper
    assert max(s["order"] for s in subframes(16, "voiced_m12")) > 8
    assert any(s["type"] == "lpc" and s["porder"] > 0 for s in subframes(16, "voiced_m8"))       # partitioned LPC residuals
    assert {s["order"] for s in subframes(16, "bs192") if s["type"] == "lpc"} == {7}
    side = subframes(24, "square_stereo")
    assert [s["type"] for s in side[:2]] == ["constant", "fixed"]     # mid is zero, the side channel runs at 25 bits


def test_the_pieces_of_the_rule():
    bs = 4096
    w = L.window(bs)
    assert w.min() == w[0] == w[-1] == (1 << 15) * 4 * bs // (bs + 1) ** 2 and w.max() < 1 << 15 and (w == w[::-1]).all()
    assert L.window(4607).max() == 1 << 15                            # an odd block: d = 0 in the middle
    edge = np.zeros(bs, np.int64)
    edge[0] = 1
    assert L.autocorrelation(edge)[0] == 0 and L.lpc_candidates(edge, 8, 12) == []
    full = np.where(np.arange(4608) % 2, -(1 << 24), (1 << 24) - 1).astype(np.int64)           # a 25-bit side channel
    assert 0 < L.autocorrelation(full)[0] < 1 << 61
    alt = np.asarray(C.case(16, "alternating").pcm[0, :bs], np.int64)
    r = L.autocorrelation(alt, rectangular=True)                      # the sums have bs - l terms: |k_1| = (bs - 1) / bs < 1
    assert r[1] * bs == -r[0] * (bs - 1) and len(L.levinson(r, 8)) == 8 and len(L.levinson(L.autocorrelation(alt), 8)) >= 1
    assert L.levinson([4, 4, 4], 2) == [] and L.levinson([4, 2, 4], 2) == [[0.5]]              # |k| = 1 at orders 1 and 2
    assert L.quantise([0.5, -1.9990234375], 12) == ([512, -2047], 10)
    assert L.quantise([1.9995], 12) == ([2047], 10) and L.quantise([1.99999], 12) == ([1024], 9)
    assert L.quantise([-2048.0], 12) is None and L.quantise([-2047.0], 12) == ([-2047], 0)
    assert L.quantise([2047.5], 12) is None and L.quantise([2047.4], 12) == ([2047], 0)
    assert L.quantise([1e-9], 12) == ([0], 15)


def test_the_default_is_the_fixed_predictor_and_its_bytes_did_not_change():
    for bps in (16, 24):
        for name in ("main", "stereo"):
            c = {c.name: c for c in K.cases(bps)}[name]
            pcm = [torch.from_numpy(c.pcm)]
            want = K.reference(bps, name)[0]
            assert flac.encode_pcm(pcm, bps, c.rate, c.block_size, backend="host") == [want]
            assert flac.encode_pcm(pcm, bps, c.rate, c.block_size, backend="host", predictor="fixed", max_lpc_order=3) == [want]
    x = torch.from_numpy(C.voiced(5000, 16, 4).astype(np.float32) / 32768)[None]
    assert flac.encode_waves(x, backend="host") == flac.encode_waves(x, backend="host", predictor="fixed")
    assert len(flac.encode_waves(x, backend="host", predictor="lpc")[0]) < len(flac.encode_waves(x, backend="host")[0])


def test_refusals_come_before_any_launch(tmp_path):
    ok = torch.zeros(1, 100, dtype=torch.int32)
    for kw in (dict(predictor="tukey"), dict(predictor=None), dict(predictor="lpc", max_lpc_order=0),
               dict(predictor="lpc", max_lpc_order=13), dict(predictor="lpc", max_lpc_order=8.0),
               dict(predictor="fixed", max_lpc_order=33)):
        for backend in ("host", "hip"):                               # refused before the backend is looked at
            with pytest.raises(ValueError, match="predictor|max_lpc_order"):
                flac.encode_pcm([ok], 16, backend=backend, **kw)
            with pytest.raises(ValueError, match="predictor|max_lpc_order"):
                flac.encode_waves(ok.float(), backend=backend, **kw)
        with pytest.raises(ValueError, match="predictor|max_lpc_order"):
            flac.write_waves([tmp_path / "x.flac"], ok.float(), backend="host", **kw)
        with pytest.raises(ValueError, match="predictor|max_lpc_order"):
            flac.write_waves([tmp_path / "x.wav"], ok.float(), fmt="wav", **kw)
    assert not list(tmp_path.iterdir())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            flac.encode_pcm([ok], 16, backend="hip", predictor="lpc")
    flac.write_waves([tmp_path / "y.flac"], torch.from_numpy(C.voiced(3000, 16, 5).astype(np.float32) / 32768)[None],
                     backend="host", predictor="lpc")
    assert R.decode((tmp_path / "y.flac").read_bytes())[1] == [C.voiced(3000, 16, 5).tolist()]


def test_c_entry_points_check_their_arguments():
    pcm = np.zeros((1, 64), np.int32)
    out = np.zeros(4096, np.uint8)
    n = ctypes.c_long()
    good = [pcm.ctypes.data, 64, 1, 16, 16000, 4096, 8, out.ctypes.data, out.size, ctypes.byref(n)]

    def host(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        H.call("nppc_flac_encode_host_lpc", *a)

    host()
    for bad in (dict(a0=None), dict(a1=0), dict(a2=0), dict(a2=9), dict(a4=0), dict(a4=1 << 20), dict(a6=0), dict(a6=13),
                dict(a7=None), dict(a8=100)):
        with pytest.raises(RuntimeError, match="bad argument"):
            host(**bad)
    for bad in (dict(a3=17), dict(a3=32), dict(a5=15), dict(a5=4609)):
        with pytest.raises(RuntimeError, match="unsupported"):
            host(**bad)
    pcm[0, 3] = 40000
    with pytest.raises(RuntimeError, match="bad argument"):
        host()
    # the device entry points reject null pointers, empty batches, order limits and unsupported formats before any launch
    p = ctypes.c_void_p(64)                                          # never dereferenced: the checks come first
    for name, args, code in (
            ("nppc_flac_enc_plan_lpc", [None, 1, p, 1, p, 1, 16, 4096, 8, p, None], "bad argument"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 0, p, 1, 16, 4096, 8, p, None], "bad argument"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 1, p, 1, 16, 4096, 8, None, None], "bad argument"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 1, p, 1, 16, 4096, 0, p, None], "bad argument"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 1, p, 1, 16, 4096, 13, p, None], "bad argument"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 1, p, 1, 17, 4096, 8, p, None], "unsupported"),
            ("nppc_flac_enc_plan_lpc", [p, 1, p, 1, p, 1, 16, 8, 8, p, None], "unsupported"),
            ("nppc_flac_enc_scan_stride", [p, 34, None, 1, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_scan_stride", [p, 34, p, 0, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_scan_stride", [p, 0, p, 1, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_scan_stride", [p, 1025, p, 1, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_write_lpc", [p, 1, p, 1, p, 1, 16, 16000, 4096, p, p, p, p, None, 1, None], "bad argument"),
            ("nppc_flac_enc_write_lpc", [p, 1, p, 1, p, 1, 16, 0, 4096, p, p, p, p, p, 1, None], "bad argument"),
            ("nppc_flac_enc_write_lpc", [p, 1, p, 0, p, 1, 16, 16000, 4096, p, p, p, p, p, 1, None], "bad argument"),
            ("nppc_flac_enc_write_lpc", [p, 1, p, 1, p, 1, 24, 16000, 5000, p, p, p, p, p, 1, None], "unsupported")):
        with pytest.raises(RuntimeError, match=code):
            H.call(name, *args)
    assert flac.PLAN_LPC_INTS == 34 and flac.ENC_MAX_LPC_ORDER == 12
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nppc_hip.h")).read()
    assert "#define NPPC_FLAC_ENC_PLAN_LPC 34" in header and "#define NPPC_FLAC_ENC_MAX_LPC 12" in header
