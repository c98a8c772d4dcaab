"""GPU: RecordingRestorer.restore(..., sample_rate=44100) and restore_file(keep_rate=True) against
the composition of the public pieces -- resample down, restore at 16 kHz, resample up -- and the fp64 native-rate splice of
tests/resample_ref.py.

Shapes: the random-weight checkpoint and the 8192-sample window of tests/test_restore_gpu.py; a 44.1 kHz recording of 22600
samples (8200 at 16 kHz: one window); two gaps 300 samples apart, closer than twice the native crossfade of
ceil(64 * 441 / 160) = 177, so they are merged; a second run with one gap near the end.

Tolerances
  outside the merged, crossfaded native ranges: the input's bits.
  inside: with `up` the fp64 restatement's upsampling of the 16 kHz restoration (same fp32 taps) and want = the fp64 splice of
  it, |got - want| <= gamma_n sum_k |h_k x_k| + 1e-12 (the last resample: an fp32 fma chain over n live taps, times a blend
  weight of at most one) + 2^-24 |want| (the splice blends in fp64 and rounds to fp32 once) + 1e-14 (the fp64 blend itself).
"""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

import resample_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
RATE, MODEL_RATE, N, WIN, XF, NFFT, HOP, K = 44100, 16000, 22600, 8192, 64, 255, 128, 3
XFN = 177
GAPS = [(9000, 10200), (10500, 11000)]
MERGED = [(9000, 11000)]
GAPS_END = [(20000, 21500)]
ALPHAS = [-1.0, 0.5]


def recording(n=N, seed=0):
    t = np.arange(n) / float(RATE)
    rng = np.random.default_rng(seed)
    x = 0.05 * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 330 * t + 1) + 0.3 * np.sin(2 * np.pi * 12000 * t))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.005 * rng.standard_normal(n)).astype(np.float32)


def with_gaps(x, gaps):
    y = x.copy()
    for s, e in gaps:
        y[s:e] = 0.0
    return y


def bits(t):
    return t.contiguous().view(torch.int32)


def region(n, gaps, xf):
    m = np.zeros(n, dtype=bool)
    for s, e in gaps:
        m[max(s - xf, 0):min(e + xf, n)] = True
    return m


@pytest.fixture(scope="module")
def restorer(tmp_path_factory):
    from nppc_audio.inpainting import restore as RS
    tmp = tmp_path_factory.mktemp("restore_native")
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(K), 41).items()}
    pre = "pretrained_restoration_model.net."
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, tmp / "restorer.pt")
    torch.save({"model_state_dict": wts}, tmp / "nppc.pt")
    mc = dict(pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
              pretrained_restoration_model_path=str(tmp / "restorer.pt"),
              audio_pc_wrapper_configuration=dict(n_dirs=K, model_configuration=dict(in_channels=2, out_channels=K,
                                                                                     precision="fp32")),
              device="cuda")
    return RS.RecordingRestorer(RS.RecordingRestorerConfig(checkpoint_path=str(tmp / "nppc.pt"), model_configuration=mc,
                                                           window_samples=WIN, n_fft=NFFT, hop_length=HOP, gl_iters=4,
                                                           crossfade_samples=XF))


def check_against_the_composition(restorer, x, gaps, merged, out, record_err, name):
    from nppc_audio import resample as RSM
    xt = torch.from_numpy(x)
    down = RSM.sinc_table(RATE, MODEL_RATE)
    n16 = R.out_length(N, RATE, MODEL_RATE)
    mapped = [RSM.map_gap(s, e, down, out_len=n16) for s, e in gaps]
    assert mapped == [R.map_gap(s, e, N, RATE, MODEL_RATE) for s, e in gaps]
    assert out["sample_rate"] == RATE and out["gaps_model_rate"] == mapped and out["gaps_merged"] == merged
    low = RSM.resample(xt.cuda(), RATE, MODEL_RATE)
    assert low.shape == (n16,) and n16 >= WIN
    inner = restorer.restore(low, mapped)
    assert torch.equal(bits(out["restored_model_rate"]), bits(inner["restored"]))
    assert [p["gap"] for p in out["windows"]] == [p["gap"] for p in inner["windows"]]
    got = out["restored"]
    assert got.shape == (N,) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    reg = region(N, merged, XFN)
    keep = torch.from_numpy(~reg)
    assert torch.equal(bits(got.cpu()[keep]), bits(xt[keep]))              # the input's own samples, bit for bit
    up, mag = R.resample(inner["restored"].cpu().numpy(), MODEL_RATE, RATE)
    assert up.size >= N
    want, touched = R.splice_native(x, up[:N], merged, XFN)
    assert np.array_equal(touched, reg)
    count = RSM.sinc_table(MODEL_RATE, RATE).count.numpy()
    lim = R.gamma(count[np.arange(N) % 441]) * mag[:N] + 1e-12 + 2.0 ** -24 * np.abs(want) + 1e-14
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    worst = float((err[reg] / lim[reg]).max())
    print(f"{name}: worst error / bound inside the spliced ranges {worst:.4f}")
    record_err(name, worst, 1.0)
    for s, e in merged:
        assert float(got[s:e].abs().max()) > 0
    return mapped, low


def test_two_merged_gaps_equal_the_composition(restorer, record_err):
    x = with_gaps(recording(), GAPS)
    out = restorer.restore(torch.from_numpy(x), GAPS, sample_rate=RATE)
    assert {"restored", "windows", "gain", "inconsistency", "target_norm", "status", "sample_rate", "restored_model_rate",
            "gaps_model_rate", "gaps_merged"} == set(out)
    mapped, low = check_against_the_composition(restorer, x, GAPS, MERGED, out, record_err, "native_two_gaps")
    again = restorer.restore(torch.from_numpy(x), GAPS, sample_rate=RATE)
    assert torch.equal(bits(again["restored"]), bits(out["restored"]))
    # garbage inside the gaps changes nothing: the mapped gaps cover the filter's reach
    noisy = x.copy()
    for s, e in GAPS:
        noisy[s:e] = 3.0
    other = restorer.restore(torch.from_numpy(noisy), GAPS, sample_rate=RATE)
    assert torch.equal(bits(other["restored"]), bits(out["restored"]))
    # the model's own rate, named or not, is the existing path
    a = restorer.restore(low, mapped, alphas=ALPHAS)
    b = restorer.restore(low, mapped, alphas=ALPHAS, sample_rate=MODEL_RATE)
    assert set(a) == set(b) and "sample_rate" not in b
    assert torch.equal(bits(a["restored"]), bits(b["restored"]))
    assert torch.equal(bits(a["variation_windows"]), bits(b["variation_windows"]))
    assert torch.equal(a["gain"], b["gain"]) and torch.equal(a["inconsistency"], b["inconsistency"])


def test_a_gap_near_the_end(restorer, record_err):
    x = with_gaps(recording(seed=3), GAPS_END)
    out = restorer.restore(torch.from_numpy(x).cuda(), GAPS_END, sample_rate=RATE)
    check_against_the_composition(restorer, x, GAPS_END, GAPS_END, out, record_err, "native_end_gap")


def test_full_variations_keep_the_input_outside(restorer):
    x = with_gaps(recording(), GAPS)
    xt = torch.from_numpy(x)
    out = restorer.restore(xt, GAPS, alphas=ALPHAS, variations="full", sample_rate=RATE)
    A = len(ALPHAS)
    assert out["variations"].shape == (K, A, N) and out["restored"].shape == (N,) and "variation_windows" not in out
    keep = torch.from_numpy(~region(N, MERGED, XFN))
    v = out["variations"].reshape(K * A, N).cpu()
    assert torch.equal(bits(v[:, keep]), bits(xt[keep].expand(K * A, -1)))
    assert torch.equal(bits(out["restored"].cpu()[keep]), bits(xt[keep]))
    assert not torch.equal(v[0, 9000:11000], v[1, 9000:11000])             # the variations differ inside
    win = restorer.restore(xt, GAPS, alphas=ALPHAS, sample_rate=RATE)      # 'windows': at the model's rate
    assert win["variation_windows"].shape == (1, K, A, WIN)
    assert torch.equal(bits(win["restored"]), bits(out["restored"]))


def test_restore_file_keeps_the_rate_and_the_known_pcm(restorer, tmp_path):
    from nppc_audio.data import _decode_wav
    pcm = np.rint(recording(seed=7).astype(np.float64) * 32768).astype(np.int16)
    for s, e in GAPS:
        pcm[s:e] = 0
    wavfile.write(str(tmp_path / "in.wav"), RATE, pcm)
    assert restorer.detect_gaps(_decode_wav(tmp_path / "in.wav", RATE)) == GAPS          # the dropouts as written
    out = restorer.restore_file(tmp_path / "in.wav", tmp_path / "out.wav", keep_rate=True)
    assert out["sample_rate"] == RATE and out["gaps_merged"] == MERGED
    sr, back = wavfile.read(str(tmp_path / "out.wav"))
    assert sr == RATE and back.dtype == np.int16 and back.shape == pcm.shape
    reg = region(N, MERGED, XFN)
    assert np.array_equal(back[~reg], pcm[~reg])                           # the known PCM, exactly
    assert np.abs(back[9000:10200]).max() > 0 and np.abs(back[10500:11000]).max() > 0
    plain = restorer.restore_file(tmp_path / "in.wav", tmp_path / "out16.wav", gaps=out["gaps_model_rate"])
    sr16, back16 = wavfile.read(str(tmp_path / "out16.wav"))
    assert sr16 == MODEL_RATE and back16.shape == (R.out_length(N, RATE, MODEL_RATE),) and "sample_rate" not in plain
