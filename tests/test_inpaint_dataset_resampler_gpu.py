"""GPU: AudioInpaintingDataset(..., resampler=) on folders at 22.05 kHz: "sinc_hann" is the
reference's torchaudio filter through nppc_audio.resample -- clip by clip for a wav folder, one ragged batch per source rate
for a flac folder -- and "scipy" stays what it was.

Bound for "sinc_hann": the one of tests/test_resample_gpu.py, |y - ref| <= gamma_n sum_k |h_k x_k| + 1e-12 with n the live
taps of the output's phase and ref the fp64 restatement (tests/resample_ref.py) over the same fp32 taps; lengths are
ceil(len * 320 / 441).  Everything else is equality."""
import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as F
import resample_ref as R
from test_flac_cpu import data_config

pytestmark = pytest.mark.gpu
RATE, SR = 22050, 16000
LENS = [12000, 12500, 3000, 13500]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """the same PCM as flac and as wav: four mono recordings at 22.05 kHz (one too short for a clip), and in the flac
    folder a fifth at 16 kHz, a second source rate"""
    tmp = tmp_path_factory.mktemp("resampler")
    sub = dict(subframes=F.lpc([1638, -819], 12, 10))
    (tmp / "flac").mkdir()
    (tmp / "wav").mkdir()
    (tmp / "mixed").mkdir()
    pcm = []
    for i, n in enumerate(LENS):
        p = C.walk(n, 16, 700 + i) // 2
        sizes = [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
        c = C.make([p], 16, rate=RATE, blocksizes=sizes, frames=sub)
        (tmp / "flac" / f"clip{i}.flac").write_bytes(c.data)
        (tmp / "mixed" / f"clip{i}.flac").write_bytes(c.data)
        C.write_wav(tmp / "wav" / f"clip{i}.wav", c)
        pcm.append((p.astype(np.float32) / 32768.0).astype(np.float32))
    p = C.walk(9000, 16, 799) // 2
    c = C.make([p], 16, rate=SR, blocksizes=[4096, 4096, 808], frames=sub)
    (tmp / "mixed" / "clip9.flac").write_bytes(c.data)
    pcm.append((p.astype(np.float32) / 32768.0).astype(np.float32))
    return tmp, pcm


def dataset(path, **kw):
    from nppc_audio.inpainting.data import AudioInpaintingDataset
    return AudioInpaintingDataset(data_config(clean_path=str(path), seed=11), **kw)


def test_sinc_hann_wav_folder_within_the_bound_and_flac_folder_bit_equal(folders, record_err):
    from nppc_audio import resample as RSM
    tmp, pcm = folders
    wav = dataset(tmp / "wav", resampler="sinc_hann")
    count = RSM.sinc_table(RATE, SR).count.numpy()
    assert len(wav) == 4
    worst = 0.0
    for clip, x, n in zip(wav.clean, pcm, LENS):
        m = -(-n * 320 // 441)
        assert clip.shape == (m,) and clip.dtype == torch.float32 and not clip.is_cuda
        ref, mag = R.resample(x, RATE, SR)
        lim = R.gamma(count[np.arange(m) % 320]) * mag + 1e-12
        worst = max(worst, float((np.abs(clip.numpy().astype(np.float64) - ref) / lim).max()))
    print(f"sinc_hann 22050 -> 16000: worst error / bound {worst:.4f}")
    record_err("dataset_sinc_hann", worst, 1.0)
    flac = dataset(tmp / "flac", resampler="sinc_hann")                    # one ragged batch: the same bits
    assert len(flac) == 4 and flac.file_of == wav.file_of and torch.equal(flac.gain, wav.gain)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(flac.clean, wav.clean))
    mixed = dataset(tmp / "mixed", resampler="sinc_hann")                  # two source rates: two groups, one a no-op
    assert len(mixed) == 5
    assert all(torch.equal(a, b) for a, b in zip(mixed.clean[:4], wav.clean))
    assert np.array_equal(mixed.clean[4].numpy(), pcm[4])                  # the 16 kHz file is its PCM, untouched
    it = wav[0]                                                            # and the dataset serves items from it
    assert it[0].is_cuda and bool(torch.isfinite(it[0]).all())


def test_scipy_stays_what_it_was(folders):
    from scipy.signal import resample_poly
    tmp, pcm = folders
    plain = dataset(tmp / "wav")
    named = dataset(tmp / "wav", resampler="scipy")
    flac = dataset(tmp / "flac", resampler="scipy")
    for a, b, c, x in zip(plain.clean, named.clean, flac.clean, pcm):
        want = resample_poly(x.astype(np.float64), 320, 441).astype(np.float32)
        assert np.array_equal(a.numpy(), want) and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError, match="resampler"):
        dataset(tmp / "wav", resampler="kaiser")
