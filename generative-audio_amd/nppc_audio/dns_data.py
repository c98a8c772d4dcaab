"""The data that FullSubNet_plus/config/train.toml selects: `[train_dataset]` = the DNS dynamic mixer
(fullsubnet_plus/dataset/dataset_train.py, identical to fullsubnet/dataset/dataset_train.py), with the reverberation and the
mixing done on the HIP device.

`DNSDatasetConfig` holds the `[train_dataset.args]` keys.  `DynamicMixDataset` mirrors dataset_train.py:12-207 on
PRE-DECODED clips (files are decoded once at construction): a random crop of the clean clip, noise assembled from random
files with silence gaps, an integer SNR, a room impulse response (RIR) for `reverb_proportion` of the items, an integer
output level.  `dataset[i]` returns the reference's (noisy [L], clean [L]) as numpy float32, computed on the host like the
reference (scipy's fftconvolve, snr_mix line by line).  The training loop does not come through there:
`DeviceReverbMixLoader` draws the same random decisions, uploads the un-mixed ingredients and makes two launches per
minibatch, nppc_rir_convolve (fftconvolve(clean, rir)[:L], direct form in fp64) and nppc_dns_snr_mix (snr_mix :153-182).
"""
import os
import random
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import pydantic
import torch

__all__ = ["DNSDatasetConfig", "DynamicMixDataset", "DeviceReverbMixLoader", "MixIngredients", "rir_convolve_on_device",
           "snr_mix_on_device", "snr_mix_host"]

EPS = 1e-6


class DNSDatasetConfig(pydantic.BaseModel):
    """`[train_dataset.args]` of train.toml, same names, the file's values as defaults.  The three *_dataset entries are
    text files with one audio path per line (`~` is expanded); `sub_sample_length` is in seconds.  pre_load_* and
    num_workers are accepted and ignored: every file is decoded once at construction."""
    clean_dataset: str = "train_data_DNS_2021_16k/clean_book.txt"
    clean_dataset_limit: Union[bool, int] = False
    clean_dataset_offset: int = 0
    noise_dataset: str = "train_data_DNS_2021_16k/noise.txt"
    noise_dataset_limit: Union[bool, int] = False
    noise_dataset_offset: int = 0
    rir_dataset: str = "train_data_DNS_2021_16k/rir.txt"
    rir_dataset_limit: Union[bool, int] = False
    rir_dataset_offset: int = 0
    snr_range: Tuple[int, int] = (-5, 20)
    reverb_proportion: float = 0.75
    silence_length: float = 0.2
    target_dB_FS: int = -25
    target_dB_FS_floating_value: int = 10
    sub_sample_length: float = 3.072
    sr: int = 16000
    pre_load_clean_dataset: bool = False
    pre_load_noise: bool = False
    pre_load_rir: bool = False
    num_workers: int = 36

    @pydantic.model_validator(mode='after')
    def check_like_the_reference(self) -> 'DNSDatasetConfig':
        # dataset_train.py:84, base_dataset.py:17-18
        assert 0 <= self.reverb_proportion <= 1, "reverberation proportion should be in [0, 1]"
        assert self.snr_range[0] <= self.snr_range[-1], "The low SNR should not larger than high SNR."
        return self

    @property
    def crop_length(self) -> int:
        return int(self.sub_sample_length * self.sr)                                  # :187

    @property
    def snr_list(self):
        return list(range(self.snr_range[0], self.snr_range[1] + 1))                  # base_dataset.py:20-25


class MixIngredients(NamedTuple):
    """the un-mixed ingredients of one item: everything random has been drawn, no per-sample arithmetic has been done"""
    clean: np.ndarray            # [L] float32, cropped or zero-padded
    noise: np.ndarray            # [L] float32
    snr: int                     # dB
    rir: Optional[np.ndarray]    # [n] float32 (one channel), None for a dry item
    level: int                   # dBFS of the mixture (noisy_target_dB_FS)


def _decode_audio(path, sr):
    """one wav file -> float32 [n] (mono) or [C, n] at `sr`, channels KEPT like the reference's librosa.load(mono=False)
    (feature.py:116-120).  scipy decodes; another rate goes through scipy's polyphase filter, which is not bit-identical to
    librosa's resampler (the caveat of data._decode_wav)."""
    from scipy.io import wavfile
    rate, a = wavfile.read(os.path.abspath(os.path.expanduser(str(path))))
    if a.dtype.kind == "i":
        a = a.astype(np.float32) / float(1 << (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == "u":
        a = (a.astype(np.float32) - 128.0) / 128.0
    else:
        a = a.astype(np.float32)
    if rate != sr and a.size:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(rate), int(sr))
        a = resample_poly(a.astype(np.float64), sr // g, rate // g, axis=0).astype(np.float32)
    return np.ascontiguousarray(a.T)


def _read_list(path, offset, limit):
    with open(os.path.abspath(os.path.expanduser(str(path))), "r") as f:
        lines = [line.rstrip("\n") for line in f]
    lines = lines[offset:]                                                            # base_dataset.py:9-13
    if limit:
        lines = lines[:limit]
    return lines


def snr_mix_host(clean_y, noise_y, snr, target_dB_FS, noisy_target_dB_FS, rir=None, eps=EPS):
    """Dataset.snr_mix (dataset_train.py:130-182) with its two random draws (RIR channel, output level) already made:
    numpy float32 arithmetic in the reference's order -> (noisy, clean)"""
    if rir is not None:
        from scipy import signal
        clean_y = signal.fftconvolve(clean_y, rir)[:len(clean_y)]

    def tailor(y, target):                                                            # feature.py:105-109
        rms = np.sqrt(np.mean(y ** 2))
        scalar = 10 ** (target / 20) / (rms + eps)
        y *= scalar
        return y, scalar

    clean_y = clean_y / (np.max(np.abs(clean_y)) + eps)                               # norm_amplitude, feature.py:98-102
    clean_y, _ = tailor(clean_y, target_dB_FS)
    clean_rms = (clean_y ** 2).mean() ** 0.5
    noise_y = noise_y / (np.max(np.abs(noise_y)) + eps)
    noise_y, _ = tailor(noise_y, target_dB_FS)
    noise_rms = (noise_y ** 2).mean() ** 0.5
    snr_scalar = clean_rms / (10 ** (snr / 20)) / (noise_rms + eps)
    noise_y *= snr_scalar
    noisy_y = clean_y + noise_y
    noisy_y, noisy_scalar = tailor(noisy_y, noisy_target_dB_FS)
    clean_y *= noisy_scalar
    if np.any(np.abs(noisy_y) > 0.999):                                               # is_clipped, feature.py:112-113
        noisy_y_scalar = np.max(np.abs(noisy_y)) / (0.99 - eps)
        noisy_y = noisy_y / noisy_y_scalar
        clean_y = clean_y / noisy_y_scalar
    return noisy_y.astype(np.float32), clean_y.astype(np.float32)


class DynamicMixDataset(torch.utils.data.Dataset):
    """dataset_train.py:12-207 on pre-decoded clips.

    DynamicMixDataset(config)                  reads the three path lists and decodes every file ONCE
    DynamicMixDataset(config, clean_clips=[...], noise_clips=[...], rir_clips=[...])   array-backed: 1-D float arrays at
                                               config.sr; a RIR clip may be [C, n] (the reference draws one channel)
    seed: None = entropy-seeded; an int seeds both generators.  The reference draws from BOTH global streams, Python's
    `random` (file choices, SNR) and numpy's legacy `np.random` (crop starts, reverb flag, RIR channel, output level); this
    class owns one of each, `self.rng = random.Random(seed)` and `self.np_rng = np.random.RandomState(seed)`, and draws
    in the reference's order, so with the two in the state of the reference's globals `draw(i)` yields the reference's
    ingredients and `dataset[i]` its item.

    With target_dB_FS_floating_value = 0 the reference's np.random.randint(t, t) raises ValueError("low >= high") at the
    first item; here the same ValueError is raised at construction."""

    def __init__(self, config: DNSDatasetConfig, clean_clips=None, noise_clips=None, rir_clips=None, seed=None):
        self.config = config
        lo = config.target_dB_FS - config.target_dB_FS_floating_value
        hi = config.target_dB_FS + config.target_dB_FS_floating_value
        if lo >= hi:
            raise ValueError(f"low >= high: the output level is drawn by randint({lo}, {hi}); "
                             "target_dB_FS_floating_value must be at least 1")
        self._level_range = (lo, hi)
        if clean_clips is None:
            c = config
            clean_clips = [_decode_audio(p, c.sr) for p in _read_list(c.clean_dataset, c.clean_dataset_offset, c.clean_dataset_limit)]
            noise_clips = [_decode_audio(p, c.sr) for p in _read_list(c.noise_dataset, c.noise_dataset_offset, c.noise_dataset_limit)]
            rir_clips = [_decode_audio(p, c.sr) for p in _read_list(c.rir_dataset, c.rir_dataset_offset, c.rir_dataset_limit)]
        if noise_clips is None:
            raise ValueError("array-backed construction needs clean_clips and noise_clips")
        self.clean = [self._mono(c, "clean") for c in clean_clips]
        self.noise = [self._mono(c, "noise") for c in noise_clips]
        self.rir = [np.ascontiguousarray(np.asarray(r, dtype=np.float32)) for r in (rir_clips or [])]
        if not self.clean or not self.noise:
            raise ValueError("the clean or the noise list is empty")
        if any(n.size == 0 for n in self.noise):
            raise ValueError("an empty noise clip would never fill an item")
        if any(r.ndim not in (1, 2) or r.shape[-1] == 0 for r in self.rir):
            raise ValueError("a RIR clip is [n] or [C, n] with n > 0")
        if config.reverb_proportion > 0 and not self.rir:
            raise ValueError("reverb_proportion > 0 needs at least one RIR clip")
        self.rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed)

    @staticmethod
    def _mono(c, what):
        c = np.asarray(c, dtype=np.float32)
        if c.ndim != 1:                                                               # subsample asserts, feature.py:161
            raise ValueError(f"Only support 1D data ({what} clip). The dim is {c.ndim}")
        return np.ascontiguousarray(c)

    def __len__(self) -> int:
        return len(self.clean)

    def _select_noise(self, target_length):                                           # :106-127
        c = self.config
        parts, silence, remaining = [], int(c.sr * c.silence_length), target_length
        while remaining > 0:
            new = self.rng.choice(self.noise)
            parts.append(new)
            remaining -= len(new)
            if remaining > 0:
                n = min(remaining, silence)
                parts.append(np.zeros(n, dtype=np.float32))
                remaining -= n
        noise = np.concatenate(parts)
        if len(noise) > target_length:
            start = self.np_rng.randint(len(noise) - target_length)
            noise = noise[start:start + target_length]
        return noise

    def draw(self, idx) -> MixIngredients:
        """the random decisions of item idx in the reference's order (crop start, noise files and start, SNR, reverb flag,
        RIR file, RIR channel, output level) and the crops they select: host copies only"""
        c = self.config
        L = c.crop_length
        clean = self.clean[idx]
        if len(clean) > L:                                                            # subsample, feature.py:164-170
            start = self.np_rng.randint(len(clean) - L)
            clean = clean[start:start + L]
        elif len(clean) < L:
            clean = np.append(clean, np.zeros(L - len(clean), dtype=np.float32))
        noise = self._select_noise(L)
        snr = self.rng.choice(c.snr_list)
        rir = None
        if bool(self.np_rng.random_sample(1) < c.reverb_proportion):                  # :193
            rir = self.rng.choice(self.rir)
            if rir.ndim > 1:                                                          # :147-149
                rir = rir[self.np_rng.randint(0, rir.shape[0]), :]
        level = int(self.np_rng.randint(*self._level_range))                          # :166-169
        return MixIngredients(clean, noise, int(snr), rir, level)

    def __getitem__(self, idx: int):
        """(noisy [L], clean [L]) numpy float32 on the host, like the reference's item"""
        it = self.draw(idx)
        return snr_mix_host(it.clean, it.noise, it.snr, self.config.target_dB_FS, it.level, rir=it.rir)


def _check_bl(name, t, B=None, L=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the HIP device")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if B is not None and tuple(t.shape) != ((B,) if L is None else (B, L)):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {(B,) if L is None else (B, L)}")
    return t.contiguous()


def rir_convolve_on_device(clean, rir, rir_len, check_lengths=True):
    """fftconvolve(clean[b], rir[b, :rir_len[b]])[:L] for a batch, on the HIP device: clean [B, L] fp32, rir [B, ldr] fp32,
    rir_len [B] int32 -> [B, L] fp32.  rir_len[b] == 0 copies clean[b] bit for bit; taps at or beyond L do not contribute;
    nothing at or past rir[b, rir_len[b]] is read.  One launch.  check_lengths reads rir_len back to verify
    0 <= rir_len <= ldr (a host synchronisation; the loader, which built rir_len itself, skips it)."""
    from . import _hip as H
    H.require_gpu()
    if clean.dim() != 2 or rir.dim() != 2:
        raise ValueError(f"clean is [B, L] and rir [B, ldr], got {tuple(clean.shape)} and {tuple(rir.shape)}")
    B, L = clean.shape
    ldr = rir.shape[1]
    if B < 1 or L < 1 or ldr < 1 or rir.shape[0] != B:
        raise ValueError(f"clean {tuple(clean.shape)} and rir {tuple(rir.shape)} need the same B >= 1 and L, ldr >= 1")
    clean, rir = _check_bl("clean", clean), _check_bl("rir", rir)
    rir_len = _check_bl("rir_len", rir_len, B, dtype=torch.int32)
    if check_lengths and (int(rir_len.min()) < 0 or int(rir_len.max()) > ldr):
        raise ValueError(f"rir_len must lie in [0, ldr = {ldr}]")
    out = torch.empty_like(clean)
    H.call("nppc_rir_convolve", clean, rir, rir_len, out, B, L, ldr, H.stream())
    return out


def snr_mix_on_device(clean, noise, snr_db, noisy_target_dbfs, target_dB_FS=-25):
    """Dataset.snr_mix after the convolution (dataset_train.py:153-182) for a batch, on the HIP device: clean (possibly
    reverberant), noise [B, L] fp32, snr_db, noisy_target_dbfs [B] fp32 -> (noisy [B, L], clean [B, L]).  One launch."""
    from . import _hip as H
    H.require_gpu()
    if clean.dim() != 2:
        raise ValueError(f"clean is [B, L], got {tuple(clean.shape)}")
    B, L = clean.shape
    if B < 1 or L < 1:
        raise ValueError("an empty batch cannot be mixed")
    clean, noise = _check_bl("clean", clean), _check_bl("noise", noise, B, L)
    snr_db, level = _check_bl("snr_db", snr_db, B), _check_bl("noisy_target_dbfs", noisy_target_dbfs, B)
    noisy_out, clean_out = torch.empty_like(clean), torch.empty_like(clean)
    H.call("nppc_dns_snr_mix", clean, noise, snr_db, level, float(target_dB_FS), noisy_out, clean_out, B, L, H.stream())
    return noisy_out, clean_out


class DeviceReverbMixLoader:
    """Minibatches of a `DynamicMixDataset` reverberated and mixed ON the HIP device.  Per batch the host draws each item's
    random decisions and gathers the un-mixed crops (memcpy-sized work) and uploads clean, noise, the RIRs (zero-padded to
    the longest of the batch, truncated to L), their lengths (0 = dry) and two scalars per item; then two launches,
    nppc_rir_convolve and nppc_dns_snr_mix, with no host synchronisation between them.  Iterates like `DeviceMixLoader`:
    yields (noisy [B, L], clean [B, L]) device tensors; `batch_sampler` yields index lists."""

    def __init__(self, dataset: DynamicMixDataset, batch_sampler, device="cuda", pin_memory=True):
        self.dataset, self.batch_sampler, self.device, self.pin = dataset, batch_sampler, device, pin_memory

    def __len__(self):
        return len(self.batch_sampler)

    def gather(self, idxs):
        """host tensors of one batch: clean, noise [B, L], rir [B, ldr], rir_len [B] int32, meta [B, 2] = (snr, level)"""
        items = [self.dataset.draw(i) for i in idxs]
        L = self.dataset.config.crop_length
        clean = torch.from_numpy(np.stack([it.clean for it in items]))
        noise = torch.from_numpy(np.stack([it.noise for it in items]))
        lens = [0 if it.rir is None else min(len(it.rir), L) for it in items]
        rir = torch.zeros(len(items), max(max(lens), 1), dtype=torch.float32)
        for b, (it, n) in enumerate(zip(items, lens)):
            if n:
                rir[b, :n] = torch.from_numpy(it.rir[:n])
        rir_len = torch.tensor(lens, dtype=torch.int32)
        meta = torch.tensor([[it.snr, it.level] for it in items], dtype=torch.float32)
        return clean, noise, rir, rir_len, meta

    def upload(self, host):
        if self.pin:
            host = tuple(t.pin_memory() for t in host)
        return tuple(t.to(self.device, non_blocking=True) for t in host)

    def __iter__(self):
        target = self.dataset.config.target_dB_FS
        for idxs in self.batch_sampler:
            clean, noise, rir, rir_len, meta = self.upload(self.gather(idxs))
            rev = rir_convolve_on_device(clean, rir, rir_len, check_lengths=False)
            yield snr_mix_on_device(rev, noise, meta[:, 0].contiguous(), meta[:, 1].contiguous(), target)
