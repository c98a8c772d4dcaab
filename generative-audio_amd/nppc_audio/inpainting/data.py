"""On-device batch synthesis for the inpainting step: what
AudioInpaintingDataset.__getitem__ (dataset/audio_dataset_inpainting.py:254-327) computes per clip on the CPU
(dBFS normalisation, gap mask, centred STFT, time_to_spec_mask, frame-masked STFT), batched in HBM with three kernels.

`AudioInpaintingDataset` + `InpaintingDeviceLoader` are the dataset itself (:86-333): a folder of recordings decoded once,
kept on the device as one flat buffer, and per minibatch the crop, the whole-file gain, the voice-activity gap placement
(`vad.py`: an energy detector, NOT the reference's silero-vad) and the two STFTs in three launches, with every random
decision drawn on the device from a counter-based generator."""
import os
from pathlib import Path

import torch

from .. import _hip as H
from . import vad as V


def time_to_spec_mask(mask_time, T_frames, waveform_length=None, win_length=255, hop_length=128, center=True):
    """AudioInpaintingDataset.time_to_spec_mask (:223-251) for a batch of sample masks [B, L] (the reference takes
    [1, L]): frame t -> 1.0 iff every sample of its clamped window is 1, 0.0 for an empty window."""
    H.require_gpu()
    mask_time = mask_time.contiguous().float()
    assert mask_time.dim() == 2, "mask_time should be [B, T] shape."
    if waveform_length is not None and int(waveform_length) < mask_time.shape[1]:
        mask_time = mask_time[:, :int(waveform_length)].contiguous()
    B, L = mask_time.shape
    out = torch.empty(B, T_frames, dtype=torch.float32, device=mask_time.device)
    H.call("nppc_time_to_spec_mask", mask_time, out, B, L, win_length, hop_length, int(center), T_frames, H.stream())
    return out


def audio_to_stft(waveform, nfft=255, hop_length=128, win_length=None):
    """utils.audio_to_stft (utils.py:150-175): [B, L] -> [B, 2, F, T] real/imag pair, any nfft = win_length <= 512."""
    H.require_gpu()
    if waveform.dim() == 1:
        waveform = waveform[None]
    if win_length not in (None, nfft):
        raise NotImplementedError("win_length != nfft")
    waveform = waveform.contiguous().float()
    B, L = waveform.shape
    spec = torch.empty(B, 2, nfft // 2 + 1, 1 + L // hop_length, dtype=torch.float32, device=waveform.device)
    H.call("nppc_stft_pair", waveform, None, spec, None, B, L, nfft, hop_length, H.stream())
    return spec


def inpainting_batch_on_device(clean_audio, gap_start, gap_end, nfft=255, hop_length=128, target_dB_FS=-25.0,
                               normalize=True):
    """clean_audio [B, L] (device), gap_start / gap_end [B] int sample indices ->
    (stft_masked [B,2,F,T], mask_frames [B,T], stft_clean [B,2,F,T], masked_audio [B,1,L]): the order of
    AudioInpaintingSample.get_training_tuple (:38-40), ready for NPPCAudioInpaintingTrainer.base_step."""
    H.require_gpu()
    clean_audio = clean_audio.contiguous().float()
    B, L = clean_audio.shape
    dev = clean_audio.device
    g0 = torch.as_tensor(gap_start, dtype=torch.int32, device=dev).contiguous()
    g1 = torch.as_tensor(gap_end, dtype=torch.int32, device=dev).contiguous()
    assert g0.shape == (B,) and g1.shape == (B,)
    T, F = 1 + L // hop_length, nfft // 2 + 1
    s = H.stream()
    audio = torch.empty_like(clean_audio)
    masked_audio = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
    mask_frames = torch.empty(B, T, dtype=torch.float32, device=dev)
    H.call("nppc_inpaint_prepare", clean_audio, g0, g1, int(bool(normalize)), float(target_dB_FS), audio, masked_audio,
           mask_frames, B, L, nfft, hop_length, T, s)
    stft_clean = torch.empty(B, 2, F, T, dtype=torch.float32, device=dev)
    stft_masked = torch.empty_like(stft_clean)
    H.call("nppc_stft_pair", audio, mask_frames, stft_clean, stft_masked, B, L, nfft, hop_length, s)
    return stft_masked, mask_frames, stft_clean, masked_audio


class AudioInpaintingDataset(torch.utils.data.Dataset):
    """dataset/audio_dataset_inpainting.py:86-333 on pre-decoded clips.

    AudioInpaintingDataset(config)                     scans config.clean_path for *.wav and decodes every file ONCE
                                                       (data._decode_wav); flac files next to them stay ignored.  A
                                                       folder with no wav and some *.flac files (LibriSpeech) is decoded
                                                       by nppc_audio.flac.decode_files in batches, on the device when
                                                       there is one; the same PCM as wav and as flac gives the same
                                                       dataset bit for bit.  When the flac decoder rejects every file it
                                                       is a ValueError that says so.  No file written by libFLAC or any
                                                       other encoder was available when the decoder was built: the
                                                       format is pinned by tests/flac_ref.py, written from the
                                                       specification.  verify_flac_md5 (default True): the decoded
                                                       samples of every file whose STREAMINFO states an MD5 are hashed
                                                       (on the device when it decodes there) and a file that decodes to
                                                       other samples than its encoder saw raises flac.FlacError (status
                                                       9) with its name; False loads such a file as it decodes.
                                                       resampler: how files at another rate reach
                                                       config.sample_rate, "scipy" (the default, data._to_rate) or
                                                       "sinc_hann", the reference's torchaudio filter
                                                       (nppc_audio.resample); a flac folder is then grouped by source
                                                       rate and every group resampled as one ragged batch.
    AudioInpaintingDataset(config, clean_clips=[...])  tensor-backed: 1-D float tensors already at config.sample_rate
    `config` is the trainer's AudioInpaintingConfig.  No transcriptions, no torch.hub.

    An index whose file is shorter than sub_sample_length maps to the next usable one, cyclically: `file_of[i]` (the
    reference's recursion :278-280).  Every file keeps the gain of its WHOLE-file normalisation (:154-168, :276), computed
    once here.  config.seed makes item idx always the same item (the reference reseeds with seed + idx, :256-264): the
    device draws use the key config.seed, the file's index and epoch 0, whatever `InpaintingDeviceLoader.set_epoch` says.
    Without config.seed the key is `seed` (None = drawn once from entropy), the counter holds the requested index and
    the loader's epoch.  `vad` overrides config.vad_configuration (default EnergyVadConfig()).

    dataset[i] = (stft_masked [2,F,T], mask_frames [T], stft_clean [2,F,T], masked_audio [1,L]) device tensors: a batch
    of one through `InpaintingDeviceLoader`."""

    def __init__(self, config, clean_clips=None, seed=None, vad=None, verify_flac_md5=True, resampler="scipy"):
        from ..data import RESAMPLERS, _decode_wav
        if resampler not in RESAMPLERS:
            raise ValueError(f"resampler = {resampler!r}: one of {RESAMPLERS}")
        self.resampler = resampler
        self.config = config
        self.verify_flac_md5 = bool(verify_flac_md5)
        sr = int(config.sample_rate)
        self.sub_sample_length = int(config.sub_sample_length_seconds * sr)            # :81-82
        self.missing_length = int(config.missing_length_seconds * sr)
        self.vad = vad or getattr(config, "vad_configuration", None) or V.EnergyVadConfig()
        st = config.stft_configuration
        if st.win_length not in (None, st.nfft):
            raise NotImplementedError("win_length != nfft")
        L, miss = self.sub_sample_length, self.missing_length
        if not 0 < miss <= L:
            raise ValueError(f"missing_length_seconds gives a gap of {miss} samples in a clip of {L}")
        self.missing_start = None
        if config.missing_start_seconds is not None:
            self.missing_start = int(config.missing_start_seconds * sr)                # :177
            if self.missing_start < 0 or self.missing_start + miss > L:
                raise ValueError(f"missing_start_seconds puts the gap at [{self.missing_start}, {self.missing_start + miss}) "
                                 f"of a clip of {L} samples")
        if config.use_vad:
            V.check_windows(L, V.vad_window(sr))
        self.clean_files = None
        if clean_clips is None:
            self.clean_path = Path(config.clean_path).resolve()
            how = ("; put *.wav files there, or pass dataset= (items of (stft_masked [2,F,T], mask_frames [T], "
                   "stft_clean [2,F,T])) or clean_clips=")
            wavs = sorted(self.clean_path.rglob("*.wav")) if self.clean_path.is_dir() else []
            flacs = sorted(self.clean_path.rglob("*.flac")) if self.clean_path.is_dir() and not wavs else []
            if flacs:
                decoded = self._decode_flac_folder(flacs, sr, how)
            elif not wavs:
                raise ValueError(f"No WAV files found in clean directory: {self.clean_path}" + how)
            else:
                decoded = [(f, _decode_wav(f, sr, resampler)) for f in wavs]
            self.clean_files = [f for f, c in decoded if c is not None]
            clean_clips = [c for _, c in decoded if c is not None]
        self.clean = [torch.as_tensor(c, dtype=torch.float32).reshape(-1) for c in clean_clips]
        usable = [i for i, c in enumerate(self.clean) if c.numel() >= L]
        if not usable:
            raise ValueError(f"no clip has the {L} samples of sub_sample_length_seconds = {config.sub_sample_length_seconds} "
                             "(pass dataset= or longer recordings)")
        n = len(self.clean)
        self.file_of, nxt = [0] * n, usable[0]                                          # past the last usable file: the first
        for i in range(n - 1, -1, -1):
            if self.clean[i].numel() >= L:
                nxt = i
            self.file_of[i] = nxt
        # _normalize_audio (:164-168) of every WHOLE file at target_dB_FS, once, in the reference's fp32 arithmetic
        self.gain = torch.stack([10 ** ((config.target_dB_FS - 20 * torch.log10(c.pow(2).mean().sqrt() + 1e-8)) / 20)
                                 if c.numel() else torch.tensor(1.0) for c in self.clean]).float()
        self.fixed_items = config.seed is not None
        if self.fixed_items:
            self.seed = int(config.seed) & V.SEED_MASK
        else:
            self.seed = (int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)) & V.SEED_MASK
        self._single = None

    def _decode_flac_folder(self, flacs, sr, how):
        """[(file, mono float32 clip at sr)] of a folder of flac files: every file is probed on the host first (a file the
        probe rejects is skipped with a warning; when it rejects all of them that is the ValueError), the rest are decoded
        by flac.decode_files in batches -- on the device when there is one -- and brought to `sr` like a wav"""
        import warnings
        import numpy as np
        from ..data import _to_rate, _to_rate_batch
        from ..flac import FlacError, decode_files, probe
        good, first = [], None
        for f in flacs:
            try:
                probe(f)
                good.append(f)
            except FlacError as e:
                first = first or e
                warnings.warn(f"skipping {e}")
        if not good:
            raise ValueError(f"{self.clean_path} holds {len(flacs)} FLAC files and no WAV file, and the flac decoder rejects "
                             f"every one of them (the first: {first})" + how)
        clips, infos = decode_files(good, out="mono", verify_md5=self.verify_flac_md5)
        if self.resampler != "scipy":
            return list(zip(good, _to_rate_batch(clips, [i.sample_rate for i in infos], sr, self.resampler)))
        return [(f, torch.from_numpy(np.ascontiguousarray(_to_rate(c.numpy(), i.sample_rate, sr))))
                for f, c, i in zip(good, clips, infos)]

    def __len__(self) -> int:
        return len(self.clean)

    def __getitem__(self, idx: int):
        if self._single is None:
            self._single = InpaintingDeviceLoader(self, None)
        out = self._single.batch([int(idx)])
        return tuple(t[0] for t in out[:4])


class InpaintingDeviceLoader:
    """Minibatches of an `AudioInpaintingDataset` assembled ON the HIP device.  Construction uploads the corpus once: every
    clip back to back in one flat fp32 buffer, the clip offsets and the whole-file gains.  A batch is three launches with no
    host synchronisation: nppc_inpaint_vad_batch (crop, gain, voice-activity segments, gap), nppc_inpaint_prepare (gap
    mask, frame mask; do_norm = 0) and nppc_stft_pair.  The only per-batch upload is the index list (2 x B int32); nothing
    is drawn on the host.

    Iterates like the DataLoader it replaces; `batch_sampler` yields index lists.  Every `iter(loader)` is one pass over
    the data: it draws with the current epoch and advances it, so without config.seed the next pass cuts other crops and
    places other gaps, as the reference's unseeded __getitem__ does on every visit (`set_epoch(e)` sets the epoch of the
    next pass; `batch(idxs)` draws with the current epoch and leaves it alone).  Yields
    (stft_masked [B,2,F,T], mask_frames [B,T], stft_clean [B,2,F,T], masked_audio [B,1,L], meta), the order of
    AudioInpaintingSample.get_training_tuple, with meta a dict of device tensors: gap_start, gap_end, used_fallback,
    crop_start, file_index (int32 [B]), n_segments [B], segments [B,S,2] and clean_audio [B,L].
    VAD-placed gaps cover 17 or 18 frames at nfft 255 / hop 128, depending on where they start: the validator takes such
    batches with ragged_gaps=True."""

    def __init__(self, dataset: AudioInpaintingDataset, batch_sampler, device="cuda"):
        H.require_gpu()
        self.dataset, self.batch_sampler = dataset, batch_sampler
        self.device = torch.device(device)
        lens = [c.numel() for c in dataset.clean]
        if max(lens) >= 2 ** 31:
            raise ValueError("a clip of 2^31 samples or more does not fit the int32 crop arithmetic")
        self.corpus = torch.cat(dataset.clean).to(self.device)
        self.offsets = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(self.device)
        self.gains = dataset.gain.to(self.device).contiguous()
        self.epoch = 0

    def __len__(self):
        return len(self.batch_sampler)

    def set_epoch(self, epoch: int):
        """the epoch of the next pass: another epoch, other crops and gaps -- unless config.seed pins the items"""
        self.epoch = int(epoch)

    def batch(self, idxs, epoch=None):
        ds, cfg = self.dataset, self.dataset.config
        epoch = self.epoch if epoch is None else int(epoch)
        n = len(ds)
        if not len(idxs) or any(not 0 <= int(i) < n for i in idxs):
            raise IndexError(f"item indices must lie in [0, {n}), got {list(idxs)}")
        files = [ds.file_of[int(i)] for i in idxs]
        items = files if ds.fixed_items else [int(i) for i in idxs]
        index = torch.tensor([files, items], dtype=torch.int32).to(self.device, non_blocking=True)
        B, L, dev = len(files), ds.sub_sample_length, self.device
        win = V.vad_window(cfg.sample_rate) if cfg.use_vad else 512
        S = V.max_segments(L, win) if cfg.use_vad else 1
        clean = torch.empty(B, L, dtype=torch.float32, device=dev)
        crop, g0, g1, nseg, fb = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(5))
        segments = torch.empty(B, S, 2, dtype=torch.int32, device=dev)
        vad, s = ds.vad, H.stream()
        H.call("nppc_inpaint_vad_batch", self.corpus, self.corpus.numel(), self.offsets, self.gains, n, index[0], index[1],
               B, L, win, ds.missing_length, -1 if ds.missing_start is None else ds.missing_start, int(bool(cfg.use_vad)),
               int(bool(cfg.is_random_sub_sample)), ds.seed, 0 if ds.fixed_items else epoch,
               float(cfg.target_dB_FS_floating_value), vad.on_db, vad.range_db, vad.hysteresis_db, vad.floor_percentile,
               vad.min_silence_samples(cfg.sample_rate), S, clean, crop, g0, g1, segments, nseg, fb, s)
        st = cfg.stft_configuration
        T, F = 1 + L // st.hop_length, st.nfft // 2 + 1
        masked_audio = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
        mask_frames = torch.empty(B, T, dtype=torch.float32, device=dev)
        H.call("nppc_inpaint_prepare", clean, g0, g1, 0, float(cfg.target_dB_FS), None, masked_audio, mask_frames, B, L,
               st.nfft, st.hop_length, T, s)
        stft_clean = torch.empty(B, 2, F, T, dtype=torch.float32, device=dev)
        stft_masked = torch.empty_like(stft_clean)
        H.call("nppc_stft_pair", clean, mask_frames, stft_clean, stft_masked, B, L, st.nfft, st.hop_length, s)
        meta = dict(gap_start=g0, gap_end=g1, used_fallback=fb, crop_start=crop, file_index=index[0], n_segments=nseg,
                    segments=segments, clean_audio=clean)
        return stft_masked, mask_frames, stft_clean, masked_audio, meta

    def __iter__(self):
        epoch = self.epoch
        self.epoch = epoch + 1                       # the next pass, whether or not this one is read to its end
        for idxs in self.batch_sampler:
            yield self.batch(idxs, epoch)
