"""Reference surface use_pre_trained_model/model_validator/model_validator.py on the HIP kernels: score a pretrained
FullSubNet+ restorer over a dataloader of (noisy, clean) clips.

The reference enhances and scores one clip at a time on the host (pesq, pystoi, numpy).  Here a whole batch is enhanced
at once (ops.stft, the FullSubNet_Plus inference forward, ops.model_outputs_to_waveforms) and scored on the device
(nppc_audio.metrics: STOI and the mean-removed SI-SDR of calculate_metrics); the per-item scores stay on the device until
the end of `validate_dataloader`, which copies them to the host once.  PESQ is not part of this build, so the metrics are
{"STOI", "SI_SDR"}; `extra_metrics=("SDR",)` adds the BSS-eval SDR of audio_zen/metrics.py:56-58 (metrics.sdr).
"""
import json
from typing import Dict, Literal

import pydantic
import torch

from . import _hip as H
from . import metrics
from . import ops
from .data import RaggedBatch
from .fullsubnet import FullSubNetPlusConfig
from .nppc_model import StftConfig, load_pretrained_model

__all__ = ["AudioConfig", "ModelValidatorConfig", "ModelValidator", "EXTRA_METRICS"]

EXTRA_METRICS = ("SDR",)        # names calculate_metrics_batch can add to {"STOI", "SI_SDR"}


class AudioConfig(pydantic.BaseModel):      # utils.py:20-22
    sr: int = 16000
    stft_configuration: StftConfig = pydantic.Field(default_factory=StftConfig)


class ModelValidatorConfig(pydantic.BaseModel):
    model_path: str
    model_configuration: FullSubNetPlusConfig
    device: Literal['cpu', 'cuda'] = 'cuda'
    audio_config: AudioConfig = pydantic.Field(default_factory=AudioConfig)


class ModelValidator:
    def __init__(self, config: ModelValidatorConfig):
        self.config = config
        st = config.audio_config.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        self.model = load_pretrained_model(config.model_path, config.model_configuration)
        self.device = config.device
        if config.device == 'cuda':
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.model.to(self.device)
        self.model.eval()

    def enhance_audio(self, noisy: torch.Tensor, clean: torch.Tensor = None, lengths=None) -> torch.Tensor:
        """noisy [B, L] or [L] -> enhanced waveforms [B, L] on the device (model_validator.py:79-130, batched): the
        compressed cIRM of the inference forward, decompressed and applied to the noisy STFT (true complex product),
        inverse STFT with length L.  `clean` is accepted for the reference's signature; the enhancement does not use it.

        lengths [B] (clips of different lengths padded to L, data.pad_collate): item b is enhanced as the clip
        noisy[b, :lengths[b]] alone would be; its samples past lengths[b] are 0 and its padding is never read."""
        H.require_gpu()
        st = self.config.audio_config.stft_configuration
        noisy = noisy.to(self.device)
        if noisy.dim() == 1:
            noisy = noisy[None]
        if lengths is not None:
            lengths = torch.as_tensor(lengths).reshape(-1).cpu()
            with torch.no_grad():
                mag, re, im = ops.stft(noisy, st.nfft, st.hop_length, lengths=lengths)
                crm = self.model(mag[:, None], re[:, None], im[:, None], frames=ops.stft_frames(lengths, st.hop_length))
                return ops.model_outputs_to_waveforms(crm, re[:, None], im[:, None], noisy.shape[-1], st.nfft, st.hop_length,
                                                      lengths=lengths)
        with torch.no_grad():
            mag, re, im = ops.stft(noisy, st.nfft, st.hop_length)
            crm = self.model(mag[:, None], re[:, None], im[:, None])
            return ops.model_outputs_to_waveforms(crm, re[:, None], im[:, None], noisy.shape[-1], st.nfft, st.hop_length)

    def _check_sr(self, sr):
        if sr != metrics.SR:
            raise ValueError(f"sr = {sr}: the metrics are built for 16000 Hz audio")

    @staticmethod
    def _check_extra(extra_metrics):
        extra = tuple(extra_metrics)
        for name in extra:
            if name not in EXTRA_METRICS:
                raise ValueError(f"extra metric {name!r}: only {sorted(EXTRA_METRICS)} can be added")
        return extra

    def calculate_metrics_batch(self, clean: torch.Tensor, enhanced: torch.Tensor, sr: int = 16000, lengths=None,
                                extra_metrics=()):
        """per-item device scores {"STOI": [B], "SI_SDR": [B]} float64 (no host synchronisation); every name of
        extra_metrics (only "SDR": metrics.sdr) adds a key of the same kind"""
        self._check_sr(sr)
        extra = self._check_extra(extra_metrics)
        clean, enhanced = clean.to(self.device), enhanced.to(self.device)
        m = {"STOI": metrics.stoi(clean, enhanced, sr=sr, lengths=lengths),
             "SI_SDR": metrics.si_sdr_zero_mean(clean, enhanced, lengths=lengths)}
        for name in extra:
            m[name] = metrics.REGISTERED_METRICS[name](clean, enhanced, sr=sr, lengths=lengths)
        return m

    def calculate_metrics(self, clean, enhanced, sr: int = 16000, extra_metrics=()) -> Dict[str, float]:
        """model_validator.py:34-77 for one clip: {"STOI", "SI_SDR"} (the mean-removed SI-SDR of the reference), and the
        extra_metrics of calculate_metrics_batch"""
        clean = torch.as_tensor(clean).reshape(-1)
        enhanced = torch.as_tensor(enhanced).reshape(-1)
        m = self.calculate_metrics_batch(clean[None], enhanced[None], sr, extra_metrics=extra_metrics)
        return {k: float(v[0]) for k, v in m.items()}

    def validate_dataloader(self, dataloader, extra_metrics=()) -> Dict[str, float]:
        """mean over all items of every metric (model_validator.py:132-170); one batched launch sequence per batch and one
        device-to-host copy at the end.  A `data.RaggedBatch` batch is enhanced and scored per item over its own length.
        extra_metrics as in calculate_metrics_batch: their means follow "STOI" and "SI_SDR" in the result."""
        extra = self._check_extra(extra_metrics)
        stoi_all, sdr_all = [], []
        extra_all = {name: [] for name in extra}
        for batch in dataloader:
            lengths = batch.lengths if isinstance(batch, RaggedBatch) else None    # by type: a plain tuple has no lengths
            noisy, clean = batch[0].to(self.device), batch[1].to(self.device)
            if noisy.dim() == 1:
                noisy, clean = noisy[None], clean[None]
            enhanced = self.enhance_audio(noisy, lengths=lengths)
            if lengths is not None:
                lengths = torch.as_tensor(lengths).to(self.device, torch.int32)
            m = self.calculate_metrics_batch(clean, enhanced, sr=self.config.audio_config.sr, lengths=lengths,
                                             extra_metrics=extra)
            stoi_all.append(m["STOI"])
            sdr_all.append(m["SI_SDR"])
            for name in extra:
                extra_all[name].append(m[name])
        if not stoi_all:
            raise ValueError("the dataloader yields no batch")
        means = torch.stack([torch.cat(stoi_all).mean(), torch.cat(sdr_all).mean()]
                            + [torch.cat(extra_all[name]).mean() for name in extra]).cpu()
        avg = {"STOI": float(means[0]), "SI_SDR": float(means[1])}
        for i, name in enumerate(extra):
            avg[name] = float(means[2 + i])
        print("\nValidation Results:")
        for metric, value in avg.items():
            print(f"{metric}: {value:.4f}")
        return avg

    def save_metrics(self, metrics_dict: Dict[str, float], save_path: str):
        """model_validator.py:172-175"""
        with open(save_path, 'w') as f:
            json.dump(metrics_dict, f, indent=4)
