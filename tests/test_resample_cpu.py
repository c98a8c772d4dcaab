"""CPU: nppc_audio.resample without a device: the compressed table against the full bank, the host
backend against the fp64 restatement (tests/resample_ref.py), output lengths, gap mapping against brute force, the refusals,
the native-rate gap arithmetic of RecordingRestorer, data._to_rate's keyword and the C ABI's host half.

Bound (host backend): every output is a sum of n = Klen products in fp32, in whatever order conv1d takes; any order obeys
|y - ref| <= gamma_n sum_k |h_k x_k|, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability, section 3.1),
with ref the fp64 sum over the same fp32 taps.  1e-12 covers the reference's own fp64 rounding.  No slack is added."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def RS():
    from nppc_audio import resample
    return resample


def signal(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.3 * np.sin(0.05 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


# ---- table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_compressed_table_scatters_back_to_the_full_bank(orig, new):
    t = RS().sinc_table(orig, new)
    kern, clamped, width = R.full_bank(orig, new)
    k32 = kern.astype(np.float32)
    assert (t.orig, t.new, t.width, t.klen) == (orig, new, width, 2 * width + orig)
    assert t.stride == (2 + t.maxcount) | 1 and t.stride % 2 == 1 and tuple(t.packed.shape) == (new, t.stride)
    packed = t.packed.numpy()
    taps = np.ascontiguousarray(packed[:, 2:]).view(np.float32)
    back = np.zeros_like(k32)
    inside = np.zeros(k32.shape, dtype=bool)
    for p in range(new):
        k0, cnt = int(packed[p, 0]), int(packed[p, 1])
        assert (k0, cnt) == (int(t.k0[p]), int(t.count[p])) and 0 < cnt <= t.maxcount and k0 + cnt <= t.klen
        back[p, k0:k0 + cnt] = taps[p, :cnt]
        inside[p, k0:k0 + cnt] = True
        assert not taps[p, cnt:].any()                                     # the row's padding
    assert np.array_equal(back, k32)                                       # exactly, tap by tap
    assert not k32[~inside].any()                                          # every tap outside the rows is 0.0f
    assert not k32[clamped].any()                                          # every clamped tap is 0.0f after the cast
    for p in range(new):                                                   # the live taps of a phase: one contiguous run
        live = np.flatnonzero(~clamped[p])
        assert live.size and np.array_equal(live, np.arange(live[0], live[-1] + 1))
        assert live[0] <= int(t.k0[p]) and int(t.k0[p] + t.count[p]) <= live[-1] + 1
    assert t.tile in RS().TILES and t.lds_bytes <= 65536


def test_the_runs_the_design_quotes():
    t = RS().sinc_table(44100, 16000)
    assert (t.orig, t.new, t.klen) == (441, 160, 475) and (int(t.count.min()), int(t.count.max())) == (33, 34)
    t = RS().sinc_table(16000, 44100)
    assert t.klen == 174 and (int(t.count.min()), int(t.count.max())) == (12, 13)
    t = RS().sinc_table(48000, 16000)
    assert t.klen == 41 and (int(t.count.min()), int(t.count.max())) == (37, 37)
    assert RS().sinc_table(44100, 16000) is RS().sinc_table(441, 160)      # cached by reduced ratio


# ---- host backend ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_host_backend_within_the_derived_bound(orig, new, record_err):
    t = RS().sinc_table(orig, new)
    x = signal(2 * orig + 1237, seed=orig + new)
    y = RS().resample(torch.from_numpy(x), orig, new, backend="host")
    ref, mag = R.resample(x, orig, new)
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
    err = np.abs(y.numpy().astype(np.float64) - ref)
    lim = R.gamma(t.klen) * mag + 1e-12
    print(f"{orig}->{new}: worst error / bound {float((err / lim).max()):.4f}")
    record_err(f"host_{orig}_{new}", float((err / lim).max()), 1.0)


def test_host_backend_ragged_batch_and_module():
    x = np.zeros((3, 1500), dtype=np.float32)
    lens = [1500, 0, 777]
    for b, n in enumerate(lens):
        x[b, :n] = signal(n, seed=b)
        x[b, n:] = np.nan                                                  # never read
    y, out = RS().resample(torch.from_numpy(x), 441, 160, lengths=lens, backend="host")
    assert out.tolist() == [R.out_length(n, 441, 160) for n in lens] and y.shape == (3, int(out.max()))
    for b, n in enumerate(lens):
        alone = RS().resample(torch.from_numpy(x[b, :n].copy()), 441, 160, backend="host")
        assert torch.equal(y[b, :int(out[b])], alone) and not y[b, int(out[b]):].any()
    m = RS().Resample(44100, 16000, backend="host")
    z = m(torch.from_numpy(x[:1, :1500]))
    assert torch.equal(z[0], y[0, :int(out[0])])
    same = torch.from_numpy(x[0])
    assert RS().resample(same, 16000, 16000) is same                       # equal rates: the input itself
    assert RS().Resample(8000, 8000)(same) is same


# ---- lengths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(441, 160), (160, 441), (3, 1), (1, 3), (7, 5)])
def test_output_lengths(orig, new):
    for n in (0, 1, orig - 1, orig, orig + 1, 3000, 4001):
        if n < 0:
            continue
        want = -(-new * n // orig)
        assert RS().out_length(n, orig, new) == want == R.out_length(n, orig, new)
        y = RS().resample(torch.from_numpy(signal(n)), orig, new, backend="host")
        assert y.shape == (want,)
    assert RS().out_length(44100, 44100, 16000) == 16000


# ---- gap mapping -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(441, 160), (160, 441), (3, 1), (1, 3), (2, 1), (1, 2), (7, 5)])
def test_map_gap_equals_brute_force(orig, new):
    t = RS().sinc_table(orig, new)
    n = 3 * orig + 1000
    n_out = R.out_length(n, orig, new)
    for j in (0, 1, new - 1, new, n_out - 1):
        assert RS().support(j, t) == R.support(j, orig, new)
    gaps = [(0, 5), (0, 1), (n - 7, n), (n - 1, n), (n // 2, n // 2 + 1), (700, 1300), (0, n)]
    for s, e in gaps:
        got = RS().map_gap(s, e, t, out_len=n_out)
        want = R.map_gap(s, e, n, orig, new)
        assert got == want, (s, e, got, want)
    assert RS().map_gap(0, n, t, out_len=n_out) == (0, n_out)
    with pytest.raises(ValueError, match="empty"):
        RS().map_gap(5, 5, t)


def test_outputs_outside_the_mapped_gap_do_not_depend_on_the_gap():
    x = signal(5000, 3)
    s, e = 2000, 2300
    z = x.copy()
    z[s:e] = 7.0
    for orig, new in [(441, 160), (160, 441)]:
        t = RS().sinc_table(orig, new)
        a, b = RS().map_gap(s, e, t, out_len=R.out_length(5000, orig, new))
        y0 = RS().resample(torch.from_numpy(x), orig, new, backend="host")
        y1 = RS().resample(torch.from_numpy(z), orig, new, backend="host")
        r0, _ = R.resample(x, orig, new)
        r1, _ = R.resample(z, orig, new)
        assert np.array_equal(r0[:a], r1[:a]) and np.array_equal(r0[b:], r1[b:])      # exactly, in the restatement
        assert float((y0 - y1)[a:b].abs().max()) > 1.0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong():
    x = torch.zeros(100)
    with pytest.raises(ValueError, match="sinc_interp_kaiser"):
        RS().resample(x, 44100, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError, match="sinc_interp_kaiser"):
        RS().Resample(44100, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError, match="16000/44101"):
        RS().resample(x, 16000, 44101, backend="host")
    with pytest.raises(ValueError, match="16000/44101"):
        RS().Resample(16000, 44101)
    for o, n in [(0, 16000), (16000, 0), (-1, 3), (3, -2), (2.5, 1)]:
        with pytest.raises(ValueError, match="rates"):
            RS().resample(x, o, n)
    with pytest.raises(ValueError, match="lengths"):
        RS().resample(torch.zeros(2, 10), 2, 1, lengths=[10, 11], backend="host")
    with pytest.raises(ValueError, match="backend"):
        RS().resample(x, 2, 1, backend="eager")
    with pytest.raises(ValueError, match="resampler"):
        from nppc_audio.data import _to_rate
        _to_rate(np.zeros(10, np.float32), 8000, 16000, resampler="torchaudio")


# ---- native-rate gap arithmetic of RecordingRestorer -----------------------------------------------------------------------
def test_native_crossfade_and_gap_merging():
    from nppc_audio.inpainting.restore import merge_native_gaps, native_crossfade
    assert native_crossfade(64, 44100, 16000) == 177 == R.native_crossfade(64, 44100, 16000)      # ceil(176.4)
    assert native_crossfade(64, 48000, 16000) == 192 and native_crossfade(64, 8000, 16000) == 32
    assert native_crossfade(0, 44100, 16000) == 0 and native_crossfade(1, 44100, 16000) == 3
    xf = 177
    cases = [[(1000, 2000), (2000 + 2 * xf - 1, 3000)], [(1000, 2000), (2000 + 2 * xf, 3000)],
             [(5000, 6000), (1000, 2000), (1500, 1700)], [(10, 20)], [(0, 5), (6, 9), (400, 500), (853, 900)]]
    for gaps in cases:
        assert merge_native_gaps(gaps, xf) == R.merge_gaps(gaps, xf)
    assert merge_native_gaps(cases[0], xf) == [(1000, 3000)]
    assert merge_native_gaps(cases[1], xf) == [(1000, 2000), (2000 + 2 * xf, 3000)]
    assert merge_native_gaps(cases[2], xf) == [(1000, 2000), (5000, 6000)]
    merged = merge_native_gaps(cases[4], xf)
    for (_, e0), (s1, _) in zip(merged, merged[1:]):                       # the blended regions never overlap
        assert e0 + xf <= s1 - xf


def test_restore_validates_native_gaps_before_anything_else():
    from nppc_audio.inpainting.restore import RecordingRestorer, RecordingRestorerConfig
    r = RecordingRestorer.__new__(RecordingRestorer)
    r.config = RecordingRestorerConfig.model_construct(sample_rate=16000, crossfade_samples=64)
    r.device = torch.device("cpu")
    x = torch.zeros(1000)
    with pytest.raises(ValueError, match=r"gap \(900, 1001\) is empty, negative or outside the recording's 1000 samples"):
        r.restore(x, [(900, 1001)], sample_rate=44100)
    with pytest.raises(ValueError, match=r"gap \(5, 5\)"):
        r.restore(x, [(5, 5)], sample_rate=44100)
    with pytest.raises(ValueError, match="44101/16000"):                   # a rate the resampler cannot hold
        r.restore(x, [(5, 50)], sample_rate=44101)
    out = r.restore(x, [], sample_rate=44100)                              # no gaps: the input itself, nothing launched
    assert out["restored"] is x and out["sample_rate"] == 44100 and out["gaps_merged"] == [] and out["windows"] == []


# ---- datasets --------------------------------------------------------------------------------------------------------------
def test_to_rate_keyword_keeps_the_scipy_path(tmp_path):
    from scipy.io import wavfile
    from nppc_audio.data import _decode_wav, _to_rate, _to_rate_batch
    a = signal(2205, 9)
    assert np.array_equal(_to_rate(a, 22050, 16000), _to_rate(a, 22050, 16000, resampler="scipy"))
    assert _to_rate(a, 16000, 16000, resampler="sinc_hann") is a
    pcm = np.rint(a.astype(np.float64) * 32768).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), 22050, pcm)
    assert torch.equal(_decode_wav(tmp_path / "a.wav", 16000), _decode_wav(tmp_path / "a.wav", 16000, "scipy"))
    clips = [torch.from_numpy(signal(n, n)) for n in (500, 0, 441)]
    got = _to_rate_batch(clips, [22050, 16000, 22050], 16000, "scipy")
    for c, g, r in zip(clips, got, [22050, 16000, 22050]):
        assert np.array_equal(g.numpy(), _to_rate(c.numpy(), r, 16000))


def test_audio_dataset_takes_the_reference_resampler(tmp_path):
    from scipy.io import wavfile
    from nppc_audio.data import AudioDataset, AudioDataSetConfig
    for sub, seed in (("clean", 1), ("noise", 2)):
        (tmp_path / sub).mkdir()
        pcm = np.rint(signal(3000, seed).astype(np.float64) * 32768).astype(np.int16)
        wavfile.write(str(tmp_path / sub / "a.wav"), 8000, pcm)
    cfg = AudioDataSetConfig(clean_path=str(tmp_path / "clean"), noisy_path=str(tmp_path / "noise"),
                             sub_sample_length_seconds=0.25)
    ds = AudioDataset(cfg, resampler="sinc_hann", seed=0)
    pcm = wavfile.read(str(tmp_path / "clean" / "a.wav"))[1].astype(np.float32) / 32768.0
    want = RS().resample(torch.from_numpy(pcm), 8000, 16000).cpu()         # "auto", as the dataset takes it
    assert ds.clean[0].shape == (6000,) and torch.equal(ds.clean[0], want)
    old = AudioDataset(cfg, seed=0)
    assert old.clean[0].shape == (6000,) and not torch.equal(old.clean[0], want)       # scipy's filter is another one
    assert torch.equal(old.clean[0], AudioDataset(cfg, resampler="scipy", seed=0).clean[0])
    with pytest.raises(ValueError, match="resampler"):
        AudioDataset(cfg, resampler="kaiser")


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_shape_answers_without_a_gpu_and_the_launcher_refuses_bad_arguments():
    from nppc_audio import _hip as H
    hdr = open(os.path.join(ROOT, "include", "nppc_hip.h")).read()
    for name in ("nppc_resample_sinc_shape", "nppc_resample_sinc"):
        assert f"int {name}(" in hdr and name in H.SIGS and hasattr(H.lib(), name)
    sh = RS().shape(441, 160, 17, 34, 1024)
    blocks = (1024 - 1) // 160 + 2
    assert sh == {"stride": 37, "table_bytes": 160 * 37 * 4, "span_elems": (blocks - 1) * 441 + 475,
                  "lds_bytes": 160 * 37 * 4 + 4 * ((blocks - 1) * 441 + 475), "fits": True}
    assert not RS().shape(16000, 44101, 7, 13, 64)["fits"]                 # the table alone is 2.6 MB
    assert not RS().shape(441, 1, 2673, 5347, 1024)["fits"] and RS().shape(441, 1, 2673, 5347, 8)["fits"]
    for bad in [(0, 160, 17, 34, 1024), (441, 0, 17, 34, 1024), (441, 160, 0, 34, 1024), (441, 160, 17, 0, 1024),
                (441, 160, 17, 34, 0), (441, 160, 17, 476, 1024)]:
        with pytest.raises(RuntimeError, match="bad argument"):
            RS().shape(*bad)
    fn = getattr(H.lib(), "nppc_resample_sinc")
    fn.argtypes, fn.restype = H.SIGS["nppc_resample_sinc"], ctypes.c_int
    buf = (ctypes.c_float * 16)()
    p, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    good = [p, 16, nul, 1, p, 441, 160, 17, 34, 1024, p, 16, nul]
    for i, v in [(0, nul), (4, nul), (10, nul), (1, 0), (1, -1), (3, 0), (3, -2), (11, 0), (11, -5), (5, -441), (9, -1)]:
        args = list(good)
        args[i] = v
        assert fn(*args) == 1, (i, v)                                      # NPPC_EBADARG, before anything is launched
    args = list(good)
    args[5:9] = [16000, 44101, 7, 13]
    assert fn(*args) == 3                                                  # NPPC_EUNSUPPORTED: the table does not fit
