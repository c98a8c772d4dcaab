"""Speech-enhancement restorer trainer on the MI355X kernels: the FullSubNet+ fine-tuning loop that
FullSubNet_plus/config/train.toml selects (`trainer.path = Trainer_Finetune`,
fullsubnet_plus/trainer/trainer.py:308-353; checkpoint layout audio_zen/trainer/base_trainer.py:160-201).

Per step: STFT of noisy and clean (512 / 256 / 512), the compressed cIRM target with drop-band, the train-mode forward
of `FullSubNet_Plus` (ONE autograd function whose backward is the engine's), mean-squared error, backward,
clip_grad_norm_(10) and Adam(1e-3, (0.9, 0.999)).  The target + loss and its gradient are HIP kernels (nppc_crm_mse /
_bwd); with Adam the clip + update is the fused clipped Adam over the flat parameter buffer (the clip coefficient stays
on the device).  The checkpoint is what `nppc_model.preload_model` reads, so the trained restorer goes straight into
`NPPCModelConfig.pretrained_restoration_model_path`.

Differences, deliberately: no AMP (train.toml has use_amp = false, the scaler is an identity), no TensorBoard, no toml
loader, no resume, one GPU.  The data: train.toml's `[train_dataset]`, the DNS dynamic mixer with reverberation, is
`dns_data.DynamicMixDataset` (pass one, or set `train_dataset_configuration`), reverberated and mixed on the device by
`DeviceReverbMixLoader` with drop_last = true (train.toml:59); the NPPC-side wav-folder `AudioDataset` (no reverberation)
keeps its `DeviceMixLoader` route.  `validate`
reports the mean loss; `validate_metrics` follows _validation_epoch (trainer.py:366-446) and scores the enhanced
waveforms with STOI and SI-SDR on the device (nppc_audio.metrics); PESQ is not part of this build, so the epoch score that
picks best_model.tar is the mean enhanced STOI.
"""
import os
from typing import List, Optional, Tuple

import pydantic
import torch
import torch.nn as nn

from . import _hip as H
from . import metrics
from . import ops
from . import ops_lstm
from .data import AudioDataset, DataConfig, DataLoaderConfig, DeviceMixLoader, RaggedBatch
from .dns_data import DeviceReverbMixLoader, DNSDatasetConfig, DynamicMixDataset
from .fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
from .nppc_model import StftConfig
from .trainer import ClippedFlatStep, HipAdam, LoopLoader, OptimizerConfig, make_optimizer

__all__ = ["FullSubNetPlusTrainerConfig", "FullSubNetPlusTrainer", "CrmMSE", "crm_mse"]


def _toml_optimizer():
    return OptimizerConfig(type="Adam", args=dict(lr=1e-3, betas=(0.9, 0.999)))     # train.toml [optimizer]


class FullSubNetPlusTrainerConfig(pydantic.BaseModel):
    """Configuration of the FullSubNet+ restorer trainer (train.toml's [model], [optimizer], [trainer] and the
    acoustics / dataset sections this build implements)"""
    model_configuration: FullSubNetPlusConfig
    data_configuration: Optional[DataConfig] = None       # wav folders; not needed when a dataset is passed
    # train.toml [train_dataset.args] (DNS dynamic mixing); used when no dataset is passed
    train_dataset_configuration: Optional[DNSDatasetConfig] = None
    dataloader_configuration: DataLoaderConfig = pydantic.Field(default_factory=DataLoaderConfig)
    optimizer_configuration: OptimizerConfig = pydantic.Field(default_factory=_toml_optimizer)
    stft_configuration: StftConfig = pydantic.Field(default_factory=StftConfig)
    clip_grad_norm_value: float = 10.0
    device: str = "cuda"


class CrmMSE(torch.autograd.Function):
    """mse_loss(gt, cRM) (trainer.py:343) with gt = drop_band(compressed cIRM(noisy, clean), G) built inside the kernel.
    crm [B,2,F',T] in drop-band order; noisy / clean STFT [B,F,T].  Returns (loss, gt); gt is not differentiable."""

    @staticmethod
    def forward(ctx, crm, n_re, n_im, c_re, c_im, groups):
        B, F, T = n_re.shape
        work = torch.empty(H.crm_mse_work_elems(), dtype=torch.float64, device=crm.device)
        loss = torch.empty((), dtype=torch.float32, device=crm.device)
        gt = torch.empty_like(crm)
        H.call("nppc_crm_mse", n_re, n_im, c_re, c_im, crm, gt, B, F, T, groups, ops.EPS32, work, loss, H.stream())
        ctx.save_for_backward(crm, n_re, n_im, c_re, c_im)
        ctx.groups = groups
        ctx.mark_non_differentiable(gt)
        return loss, gt

    @staticmethod
    def backward(ctx, g, _g_gt):
        crm, n_re, n_im, c_re, c_im = ctx.saved_tensors
        B, F, T = n_re.shape
        dcrm = torch.empty_like(crm)
        H.call("nppc_crm_mse_bwd", n_re, n_im, c_re, c_im, crm, g.float().contiguous(), dcrm, B, F, T, ctx.groups, ops.EPS32,
               H.stream())
        return dcrm, None, None, None, None, None


def crm_mse(crm, n_re, n_im, c_re, c_im, groups):
    """(loss, gt): loss = mean (gt - crm)^2, gt = drop_band(compressed cIRM, groups) [B,2,F',T]"""
    H.require_gpu()
    B, F, T = n_re.shape
    Fo = F if groups <= 1 else (F - F % groups) // groups
    if tuple(crm.shape) != (B, 2, Fo, T) or any(tuple(t.shape) != (B, F, T) for t in (n_im, c_re, c_im)):
        raise ValueError(f"crm_mse: crm {tuple(crm.shape)} needs [{B}, 2, {Fo}, {T}] for STFTs of {(B, F, T)}, groups {groups}")
    n_re, n_im, c_re, c_im = (ops._f32c(t) for t in (n_re, n_im, c_re, c_im))
    return CrmMSE.apply(crm.contiguous().float(), n_re, n_im, c_re, c_im, int(groups))


class FullSubNetPlusTrainer(nn.Module):
    def __init__(self, config: FullSubNetPlusTrainerConfig, dataset=None):
        super().__init__()
        self.config = config
        st = config.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        if st.nfft // 2 + 1 != config.model_configuration.num_freqs:
            raise ValueError(f"nfft {st.nfft} gives {st.nfft // 2 + 1} bins, the model has num_freqs = "
                             f"{config.model_configuration.num_freqs}")
        bs, G = config.dataloader_configuration.batch_size, config.model_configuration.num_groups_in_drop_band
        if bs <= G:
            # drop_band asserts batch_size > num_groups on the target of every training batch (feature.py:263)
            raise ValueError(f"Batch size = {bs}, num_groups = {G}. The batch size should larger than the num_groups.")
        self.model = FullSubNet_Plus(config.model_configuration)       # raises for the configurations not built here
        self.device = config.device
        if config.device == "cuda":
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.model.to(self.device)
        self.model.train()

        self.optimizer = make_optimizer(self.model.parameters(), config.optimizer_configuration)

        if dataset is None:
            if config.train_dataset_configuration is not None:
                dataset = DynamicMixDataset(config.train_dataset_configuration)
            elif config.data_configuration is None:
                raise ValueError("pass a dataset or a data_configuration (wav folders of clean speech and noise)")
            else:
                dataset = AudioDataset(config.data_configuration.dataset)
        self.dataset = dataset
        self.dataloader = self.make_loader(dataset, config.dataloader_configuration)
        self.step = 0
        self.epoch = 0
        self.loss_history: List[float] = []
        self._clip_step = ClippedFlatStep()
        self.best_score = float("-inf")
        self.val_history: List[dict] = []

    def make_loader(self, dataset, lc):
        """(noisy [B,L], clean [B,L]) batches: an AudioDataset on a HIP device is mixed there (DeviceMixLoader), a
        DynamicMixDataset is reverberated and mixed there (DeviceReverbMixLoader; drop_last like train.toml:59, a last
        partial batch of <= num_groups items would trip drop-band's assertion)"""
        if isinstance(dataset, DynamicMixDataset) and str(self.device).startswith("cuda"):
            base = (torch.utils.data.RandomSampler if lc.shuffle else torch.utils.data.SequentialSampler)(dataset)
            return DeviceReverbMixLoader(dataset, torch.utils.data.BatchSampler(base, lc.batch_size, drop_last=True),
                                         device=self.device, pin_memory=lc.pin_memory)
        if isinstance(dataset, AudioDataset) and str(self.device).startswith("cuda"):
            base = (torch.utils.data.RandomSampler if lc.shuffle else torch.utils.data.SequentialSampler)(dataset)
            return DeviceMixLoader(dataset, torch.utils.data.BatchSampler(base, lc.batch_size, drop_last=False),
                                   device=self.device, pin_memory=lc.pin_memory)
        return torch.utils.data.DataLoader(dataset, batch_size=lc.batch_size, shuffle=lc.shuffle, num_workers=lc.num_workers,
                                           pin_memory=lc.pin_memory)

    # ---------------------------------------------------------------------------------- reference API
    def base_step(self, batch) -> Tuple[torch.Tensor, dict]:
        """(noisy [B,L], clean [B,L]) -> (loss, log): trainer.py:328-343 (drop-band only when B > 1, like the forward)"""
        noisy, clean = batch[0], batch[1]
        st = self.config.stft_configuration
        mag, n_re, n_im = ops.stft(noisy, st.nfft, st.hop_length)
        _, c_re, c_im = ops.stft(clean, st.nfft, st.hop_length, want_mag=False)
        B = n_re.shape[0]
        G = self.config.model_configuration.num_groups_in_drop_band if B > 1 else 1
        crm = self.model(mag[:, None], n_re[:, None], n_im[:, None])          # [B, 2, F', T]
        loss, gt = crm_mse(crm, n_re, n_im, c_re, c_im, G)
        log = {"cRM": crm.detach(), "gt": gt, "loss": loss.detach()}
        return loss, log

    def validate(self, loader):
        """mean loss over the loader, no gradients (the inference launch sequence)"""
        losses = []
        with torch.no_grad():
            for batch in loader:
                loss, _ = self.base_step(self._to_device(batch))
                losses.append(loss.item())
        if not losses:
            raise ValueError("the validation loader yields no batch")
        return sum(losses) / len(losses)

    def full_band_output(self, mag, n_re, n_im):
        """compressed cIRM [B,2,F,T] of the inference forward WITHOUT drop-band.  The forward drop-bands any batch of
        B > 1 when num_groups_in_drop_band > 1 (fullsubnet_plus.py:212-214); the reference validates with batch size 1,
        so such a batch runs one clip at a time here."""
        B = mag.shape[0]
        with torch.no_grad():
            if B > 1 and self.config.model_configuration.num_groups_in_drop_band > 1:
                return torch.cat([self.model(mag[b:b + 1, None], n_re[b:b + 1, None], n_im[b:b + 1, None])
                                  for b in range(B)])
            return self.model(mag[:, None], n_re[:, None], n_im[:, None])

    def validate_metrics(self, loader):
        """Trainer_Finetune._validation_epoch (trainer.py:366-446) + metrics_visualization (base_trainer.py:264-303) on
        (noisy [B,L], clean [B,L]) batches: the loss on the cIRM WITHOUT drop-band (full_band_output, crm_mse with one
        group), the enhanced waveform (decompressed mask applied to the noisy STFT, inverse STFT), and STOI and audio_zen's
        SI-SDR of the noisy and of the enhanced waveform against the clean one.  Returns {"loss", "STOI_noisy", "STOI",
        "SI_SDR_noisy", "SI_SDR", "score"}: loss = mean of the batch losses (the reference's per-clip mean at batch size
        1), the metrics = means over items.  The reference's score is (STOI + (WB_PESQ + 0.5) / 5) / 2; without PESQ it is
        the mean enhanced STOI here.  Everything stays on the device until one host copy at the end.

        A `data.RaggedBatch` (clips of different lengths, data.pad_collate) runs the ragged forward: every item is scored
        as if run alone, and its cIRM MSE over its own frames counts as one clip of the loss mean."""
        st = self.config.stft_configuration
        losses, scores = [], {k: [] for k in ("STOI_noisy", "STOI", "SI_SDR_noisy", "SI_SDR")}
        with torch.no_grad():
            for batch in loader:
                if isinstance(batch, RaggedBatch):
                    loss, sc = self._ragged_metrics(batch)
                    losses.append(loss)
                    for k in scores:
                        scores[k].append(sc[k])
                    continue
                noisy, clean = self._to_device(batch)
                mag, n_re, n_im = ops.stft(noisy, st.nfft, st.hop_length)
                _, c_re, c_im = ops.stft(clean, st.nfft, st.hop_length, want_mag=False)
                crm = self.full_band_output(mag, n_re, n_im)
                loss, _ = crm_mse(crm, n_re, n_im, c_re, c_im, 1)
                enhanced = ops.model_outputs_to_waveforms(crm, n_re[:, None], n_im[:, None], noisy.shape[-1], st.nfft,
                                                          st.hop_length)
                losses.append(loss.double().reshape(1))
                scores["STOI_noisy"].append(metrics.stoi(clean, noisy))
                scores["STOI"].append(metrics.stoi(clean, enhanced))
                scores["SI_SDR_noisy"].append(metrics.si_sdr(clean, noisy))
                scores["SI_SDR"].append(metrics.si_sdr(clean, enhanced))
        if not losses:
            raise ValueError("the validation loader yields no batch")
        names = ["loss"] + list(scores)
        vals = torch.stack([torch.cat(losses).mean()] + [torch.cat(v).mean() for v in scores.values()]).cpu().tolist()
        out = dict(zip(names, vals))
        out["score"] = out["STOI"]
        return out

    def _ragged_metrics(self, batch):
        """validate_metrics of one RaggedBatch: (per-item cIRM MSE [B] fp64, per-item scores)"""
        st = self.config.stft_configuration
        noisy, clean = (x.to(self.device, non_blocking=True) for x in batch[:2])
        lengths = batch.lengths
        mag, n_re, n_im = ops.stft(noisy, st.nfft, st.hop_length, lengths=lengths)
        _, c_re, c_im = ops.stft(clean, st.nfft, st.hop_length, want_mag=False, lengths=lengths)
        frames = ops.stft_frames(torch.as_tensor(lengths, dtype=torch.int64).cpu(), st.hop_length)
        crm = self.model(mag[:, None], n_re[:, None], n_im[:, None], frames=frames)     # [B, 2, F, T], no drop-band
        dl = torch.as_tensor(lengths).to(self.device, torch.int32)
        loss = ops.crm_mse_ragged(n_re, n_im, c_re, c_im, crm, frames.to(self.device, torch.int32))
        enhanced = ops.model_outputs_to_waveforms(crm, n_re[:, None], n_im[:, None], noisy.shape[-1], st.nfft, st.hop_length,
                                                  lengths=lengths)
        sc = {"STOI_noisy": metrics.stoi(clean, noisy, lengths=dl), "STOI": metrics.stoi(clean, enhanced, lengths=dl),
              "SI_SDR_noisy": metrics.si_sdr(clean, noisy, lengths=dl), "SI_SDR": metrics.si_sdr(clean, enhanced, lengths=dl)}
        return loss, sc

    # ---------------------------------------------------------------------------------- one optimisation step
    def train_step(self, batch):
        """zero_grad + forward + backward + clip_grad_norm_(clip_grad_norm_value) + optimizer step (trainer.py:325-349).
        log['grad_norm'] is the total gradient norm before clipping (a device tensor).
        The clipped Adam does not read the hand-off time-out counters of the cooperative LSTM kernels, so every step ends
        with ops_lstm.check_coop_timeouts: a timed-out hand-off raises here instead of training on wrong numbers (the check
        reads the counters on the host, i.e. it waits for the step)."""
        net = self.model
        fast = isinstance(self.optimizer, HipAdam)
        net.flat_grad_only = fast
        try:
            self.optimizer.zero_grad()
            loss, log = self.base_step(batch)
            loss.backward()
        finally:
            net.flat_grad_only = False
        if fast:
            log["grad_norm"] = self._clip_step(self.optimizer, net.engine(), self.config.clip_grad_norm_value)
        else:
            log["grad_norm"] = torch.nn.utils.clip_grad_norm_(net.parameters(), self.config.clip_grad_norm_value)
            self.optimizer.step()
        self.step += 1
        ops_lstm.check_coop_timeouts(f"step {self.step}")
        return loss, log

    def _to_device(self, batch):
        return tuple(x.to(self.device, non_blocking=True) for x in batch[:2])

    def train(self, n_steps=None, n_epochs=None, checkpoint_dir="checkpoints", save_flag=True, val_loader=None):
        """training loop (the name shadows nn.Module.train like the NPPC trainers; mode changes go through self.model).
        Writes <checkpoint_dir>/latest_model.tar at the end when save_flag.  Returns the per-step loss history.
        With a val_loader, every completed epoch ends with validate_metrics (train.toml validation_interval = 1; the
        results go to self.val_history) and, when its score >= the best so far (save_max_metric_score = true),
        <checkpoint_dir>/best_model.tar in the layout of save_checkpoint with that best_score (base_trainer.py:160-215)."""
        assert n_steps is not None or n_epochs is not None, "Must specify either n_steps or n_epochs"
        loop_loader = LoopLoader(dataloader=self.dataloader, n_steps=n_steps, n_epochs=n_epochs)
        if len(loop_loader) == 0:
            raise ValueError("the data loader yields no minibatch")
        per_epoch = max(len(self.dataloader), 1)
        history: List[float] = []
        for it, batch in enumerate(loop_loader):
            loss, _ = self.train_step(self._to_device(batch))
            history.append(loss.item())
            if (it + 1) % per_epoch == 0:
                self.epoch += 1
                if val_loader is not None:
                    self._validate_epoch(val_loader, checkpoint_dir)
        self.loss_history.extend(history)
        if history:
            print(f"step {self.step}: Loss: {history[-1]:.4f}")
        if save_flag:
            os.makedirs(checkpoint_dir, exist_ok=True)
            self.save_checkpoint(os.path.join(checkpoint_dir, "latest_model.tar"))
        return history

    def _validate_epoch(self, val_loader, checkpoint_dir):
        m = self.validate_metrics(val_loader)
        m["epoch"] = self.epoch
        self.val_history.append(m)
        print(f"epoch {self.epoch}: validation loss {m['loss']:.4f}, STOI {m['STOI']:.4f} (noisy {m['STOI_noisy']:.4f}), "
              f"SI-SDR {m['SI_SDR']:.2f} dB (noisy {m['SI_SDR_noisy']:.2f} dB)")
        if m["score"] >= self.best_score:
            self.best_score = m["score"]
            self.save_checkpoint(os.path.join(checkpoint_dir, "best_model.tar"), best_score=m["score"])
        return m

    def save_checkpoint(self, path, best_score=None):
        """base_trainer.py:173-184 layout: {"epoch", "best_score", "optimizer", "scaler", "model"} (+ "step");
        "model" loads strictly into FullSubNet_Plus and is what nppc_model.preload_model reads"""
        checkpoint = {
            "epoch": self.epoch,
            "step": self.step,
            "best_score": float("-inf") if best_score is None else best_score,
            "optimizer": self.optimizer.state_dict(),
            "scaler": {},                     # use_amp = false: the reference's disabled GradScaler has an empty state
            "model": self.model.state_dict(),
        }
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        torch.save(checkpoint, path)
        print(f"Checkpoint saved to {path}")
        return path
