"""CPU: the serial FLAC encoder (csrc/flac_enc_core.h through nppc_flac_encode_host and flac.encode_pcm(backend="host")) gives
byte for byte what the restatement tests/flac_enc_ref.py gives, and both decoders give the samples back."""
import ctypes

import numpy as np
import pytest
import torch

import flac_enc_cases as K
import flac_enc_ref as E
import flac_ref as R
from nppc_audio import _hip as H
from nppc_audio import flac

ALL = [(16, c.name, True) for c in K.cases(16)] + [(b, c.name, False) for b in (8, 12, 20, 24) for c in K.cases(b, False)]


def encode_host_raw(pcm, bps, rate, block_size):
    """straight through the C entry point"""
    pcm = np.ascontiguousarray(pcm, np.int32)
    cap, frames = ctypes.c_long(), ctypes.c_long()
    H.call("nppc_flac_enc_bound", pcm.shape[1], pcm.shape[0], bps, block_size, ctypes.byref(cap), ctypes.byref(frames))
    assert frames.value == -(-pcm.shape[1] // block_size)
    out = np.full(cap.value, 0xA5, np.uint8)
    n = ctypes.c_long()
    H.call("nppc_flac_encode_host", pcm.ctypes.data, pcm.shape[1], pcm.shape[0], bps, rate, block_size, out.ctypes.data, cap.value,
           ctypes.byref(n))
    assert 0 < n.value <= cap.value
    return out[:n.value].tobytes()


def frame_sizes(data):
    info = R.probe(data)
    off, count, sizes = info["first_frame"], 0, []
    while count < info["total_samples"]:
        hdr = R.parse_header(data, off, info)
        _, end = R.decode_frame(data, off, info, hdr)
        sizes.append(end - off)
        count, off = count + hdr["bs"], end
    assert off == len(data)
    return sizes


def check_stream(data, case):
    """what every encoded stream has to be, whoever wrote it"""
    pcm = case.pcm
    info, back = R.decode(data)
    assert np.array_equal(np.asarray(back, np.int64), pcm)
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"], info["total_samples"]) == \
        (case.rate, pcm.shape[0], case.bps, pcm.shape[1])
    assert info["min_blocksize"] == info["max_blocksize"] == case.block_size
    sizes = frame_sizes(data)
    assert (info["min_frame"], info["max_frame"]) == (min(sizes), max(sizes))
    (host,), (hinfo,) = flac.decode_files([data], out="pcm", backend="host", verify_md5=True)
    assert np.array_equal(host.numpy(), pcm) and hinfo.sample_rate == case.rate
    md5 = flac.stream_md5(data)
    assert md5 is not None and md5 == flac.pcm_md5(torch.from_numpy(pcm), case.bps, backend="host")[0] == E.pcm_md5(pcm, case.bps)


@pytest.mark.parametrize("bps,name,full_set", ALL, ids=[f"{b}-{n}" for b, n, _ in ALL])
def test_host_encoder_equals_the_restatement(bps, name, full_set):
    case = {c.name: c for c in K.cases(bps, full_set)}[name]
    want, _ = K.reference(bps, name, full_set)
    got = encode_host_raw(case.pcm, case.bps, case.rate, case.block_size)
    assert got == want
    assert flac.encode_pcm([torch.from_numpy(case.pcm)], case.bps, case.rate, case.block_size, backend="host") == [want]
    check_stream(got, case)


def subframes(bps, name):
    return [(f["assign"], [s["type"] for s in f["subframes"]], f["subframes"]) for f in K.reference(bps, name)[1]]


def test_the_plans_take_every_path():
    main = subframes(16, "main")
    assert [t for _, t, _ in main] == [["fixed"], ["constant"], ["verbatim"], ["fixed"]]
    assert {s[0]["order"] for _, t, s in main if t == ["fixed"]} <= {1, 2, 3, 4}
    spike = subframes(16, "spike")[-1][2][0]
    assert (spike["type"], spike["order"], spike["porder"]) == ("fixed", 0, 0) and spike["params"][0] in (5, 6)
    assert 30000 * 2 >> spike["params"][0] > 900                     # a unary run of tens of words
    assert {a for a, _, _ in subframes(16, "stereo")} == {0, 1, 2, 3}
    assert {a for a, _, _ in subframes(24, "stereo")} == {0, 1, 2, 3}
    ramp = subframes(16, "ramp")[0][2][0]
    assert (ramp["type"], ramp["order"], ramp["porder"]) == ("fixed", 2, 0)      # orders 3 and 4 tie on the residual: lower o
    assert {s[0]["porder"] for _, t, s in main if t == ["fixed"]} - {0}          # partitioned residuals
    assert {f["subframes"][0]["porder"] for f in K.reference(16, "p8")[1]} == {8}
    assert K.reference(24, "main")[1][0]["subframes"][0]["method"] == 1


def test_more_than_two_channels_on_the_host():
    pcm = np.stack([K.speech(3000, 16, s) for s in (1, 2, 3)])
    c = K.Case("three", pcm, 16, 16000, 1024)
    got = encode_host_raw(pcm, 16, 16000, 1024)
    assert got == E.encode(pcm, 16, 16000, 1024)
    check_stream(got, c)


def test_encode_pcm_rejects_before_any_launch():
    ok = torch.zeros(1, 100, dtype=torch.int32)
    for kw, pcm in ((dict(bits_per_sample=16), [torch.zeros(1, 0, dtype=torch.int32)]),
                    (dict(bits_per_sample=15), [ok]), (dict(bits_per_sample=32), [ok]),
                    (dict(bits_per_sample=16, block_size=15), [ok]), (dict(bits_per_sample=16, block_size=4609), [ok]),
                    (dict(bits_per_sample=16, backend="cpu"), [ok]),
                    (dict(bits_per_sample=16), [torch.full((1, 5), 32768, dtype=torch.int32)]),
                    (dict(bits_per_sample=8), [torch.full((1, 5), -129, dtype=torch.int32)]),
                    (dict(bits_per_sample=16), [ok.float()]), (dict(bits_per_sample=16), [torch.zeros(9, 4, dtype=torch.int32)])):
        kw.setdefault("backend", "host")
        with pytest.raises(ValueError):
            flac.encode_pcm(pcm, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            flac.encode_pcm([ok], 16, backend="hip")
    assert flac.encode_pcm([], 16, backend="host") == []
    edge = torch.tensor([[-32768, 32767]], dtype=torch.int32)
    assert R.decode(flac.encode_pcm([edge], 16, backend="host")[0])[1] == [[-32768, 32767]]


def test_c_entry_points_check_their_arguments():
    pcm = np.zeros((1, 64), np.int32)
    out = np.zeros(4096, np.uint8)
    n, m = ctypes.c_long(), ctypes.c_long()
    good = [pcm.ctypes.data, 64, 1, 16, 16000, 4096, out.ctypes.data, out.size, ctypes.byref(n)]

    def host(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        H.call("nppc_flac_encode_host", *a)

    host()
    for bad in (dict(a0=None), dict(a1=0), dict(a2=0), dict(a2=9), dict(a4=0), dict(a4=1 << 20), dict(a6=None), dict(a7=100)):
        with pytest.raises(RuntimeError, match="bad argument"):
            host(**bad)
    for bad in (dict(a3=17), dict(a3=32), dict(a5=15), dict(a5=4609)):
        with pytest.raises(RuntimeError, match="unsupported"):
            host(**bad)
    pcm[0, 3] = 40000
    with pytest.raises(RuntimeError, match="bad argument"):
        host()
    with pytest.raises(RuntimeError, match="bad argument"):
        H.call("nppc_flac_enc_bound", 0, 1, 16, 4096, ctypes.byref(n), ctypes.byref(m))
    with pytest.raises(RuntimeError, match="unsupported"):
        H.call("nppc_flac_enc_bound", 10, 1, 18, 4096, ctypes.byref(n), ctypes.byref(m))
    # the device entry points reject null pointers, empty batches and unsupported formats before any launch
    p = ctypes.c_void_p(64)                                          # never dereferenced: the checks come first
    for name, args, code in (
            ("nppc_flac_enc_plan", [None, 1, p, 1, p, 1, 16, 4096, p, None], "bad argument"),
            ("nppc_flac_enc_plan", [p, 1, p, 0, p, 1, 16, 4096, p, None], "bad argument"),
            ("nppc_flac_enc_plan", [p, 1, p, 1, p, 1, 17, 4096, p, None], "unsupported"),
            ("nppc_flac_enc_plan", [p, 1, p, 1, p, 1, 16, 8, p, None], "unsupported"),
            ("nppc_flac_enc_scan", [p, None, 1, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_scan", [p, p, 0, 1, p, p, None], "bad argument"),
            ("nppc_flac_enc_write", [p, 1, p, 1, p, 1, 16, 16000, 4096, p, p, p, p, None, 1, None], "bad argument"),
            ("nppc_flac_enc_write", [p, 1, p, 1, p, 1, 16, 0, 4096, p, p, p, p, p, 1, None], "bad argument"),
            ("nppc_flac_enc_write", [p, 1, p, 1, p, 1, 24, 16000, 5000, p, p, p, p, p, 1, None], "unsupported"),
            ("nppc_pcm_quantize", [None, 1, None, 1, 16, p, p, 1, None], "bad argument"),
            ("nppc_pcm_quantize", [p, 1, None, 0, 16, p, p, 1, None], "bad argument"),
            ("nppc_pcm_quantize", [p, 1, None, 1, 13, p, p, 1, None], "unsupported")):
        with pytest.raises(RuntimeError, match=code):
            H.call(name, *args)


def test_the_quantiser_formula():
    """quantize_waves_host is the formula of the issue, clip(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1) with halves to
    even, worked out here in Python integers and fractions; the device kernel is compared with it on the GPU"""
    from fractions import Fraction
    for bits in (8, 16, 24):
        full = 1 << (bits - 1)
        eps = float(np.spacing(np.float32(1.0)))
        xs = [1.0, -1.0, 1.0 - eps / 2, -1.0 - eps, 1.0 + eps, (full - 1) / full, (full - 0.5) / full, -(full - 0.5) / full,
              0.5 / full, 1.5 / full, 2.5 / full, -0.5 / full, -1.5 / full, -2.5 / full, 0.0, 3.0, -3.0, 0.49999 / full]
        x = np.array(xs, np.float32)
        want = []
        for v in x:
            y = Fraction(float(v)) * full
            r = int(y // 1)
            frac = y - r
            r = r + 1 if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and r % 2) else r
            want.append(max(-full, min(full - 1, r)))
        got = flac.quantize_waves_host(x, bits)
        assert got.dtype == np.int32 and got.tolist() == want, (bits, got.tolist(), want)
    streams = flac.encode_waves(torch.tensor([[0.25, -0.5, 1.0, -1.0], [0.0, 0.5 / 32768, 1.5 / 32768, 9.0]]), lengths=[4, 3],
                                backend="host")
    assert [R.decode(s)[1] for s in streams] == [[[8192, -16384, 32767, -32768]], [[0, 0, 2]]]
