"""Inpainting restorer trainer on the MI355X kernels: mirrors nppc_audio/inpainting/trainer/restoration_trainer.py
(OptimizerConfig :19-21, InpaintingTrainerConfig :24-35, InpaintingTrainer.__init__ :39-80, train :104-176,
base_step :178-200, validate :202-222, save_checkpoint :260-284, _get_and_save_metrics :286-327).

It trains the restorer the inpainting NPPC model loads frozen (`RestorationWrapper(UNet(1 -> 1, dropout 0.2))`): the
U-Net runs in train mode (batch-statistics BatchNorm, running-buffer update) with its four nn.Dropout layers active,
the masked spectral MSE and its gradient are HIP kernels, and with Adam the clip_grad_norm_ + update is the fused
clipped Adam over the flat parameter buffer (the clip coefficient stays on the device).

Differences, deliberately: wandb logging and matplotlib plotting are not built (`use_wandb=True` raises
NotImplementedError); without a `dataset=` the data come from `data.AudioInpaintingDataset` + `data.InpaintingDeviceLoader`
(a wav folder, minibatches assembled on the device, gaps placed by the energy voice-activity detector of `vad.py` where the
reference uses silero-vad); `max_grad_norm` is a config field (the reference hard-codes 5); the step's loss history is kept
on the trainer (`loss_history`) and returned by `train`.
"""
import json
import os
from datetime import datetime
from typing import List, Optional

import pydantic
import torch
import torch.nn as nn

from ... import _hip as H
from ...data import DataLoaderConfig
from ...trainer import ClippedFlatStep, HipAdam, LoopLoader, OptimizerConfig, make_optimizer
from ..networks.unet import RestorationWrapper, UNet, UNetConfig
from ..utils import preprocess_data
from .nppc_trainer import AudioInpaintingConfig, build_device_loader

__all__ = ["OptimizerConfig", "InpaintingTrainerConfig", "InpaintingTrainer", "MaskedSpectralMSE", "masked_spectral_mse"]


class InpaintingTrainerConfig(pydantic.BaseModel):
    """Configuration for Inpainting trainer"""
    model_configuration: UNetConfig
    data_configuration: AudioInpaintingConfig
    dataloader_configuration: DataLoaderConfig
    optimizer_configuration: OptimizerConfig
    device: str = "cuda"
    use_wandb: bool = False
    wandb_project_name: Optional[str] = "generative-audio"
    wandb_run_name: Optional[str] = None
    wandb_tags: Optional[List[str]] = None
    wandb_artifact_name: str = "restoration_model"
    max_grad_norm: float = 5.0


class MaskedSpectralMSE(torch.autograd.Function):
    """loss = sum (out - clean)^2 (1 - m) / (F sum (1 - m) + 1e-6)  (restoration_trainer.py:189-191): out, clean [B,1,F,T]
    fp32, m [B,T] broadcast over F.  nppc_masked_mse reduces in fp64 without float atomics (bit-identical on repeat);
    nppc_masked_mse_bwd reads the incoming gradient from the device."""

    @staticmethod
    def forward(ctx, out, clean, mask_frames):
        B, _, F, T = out.shape
        work = torch.empty(H.masked_mse_work_elems(), dtype=torch.float64, device=out.device)
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        H.call("nppc_masked_mse", out, clean, mask_frames, B, F, T, work, loss, H.stream())
        ctx.save_for_backward(out, clean, mask_frames, work)
        return loss

    @staticmethod
    def backward(ctx, g):
        out, clean, mask_frames, work = ctx.saved_tensors
        B, _, F, T = out.shape
        dout = torch.empty_like(out)
        H.call("nppc_masked_mse_bwd", out, clean, mask_frames, g.float().contiguous(), work, dout, B, F, T, H.stream())
        return dout, None, None


def masked_spectral_mse(output, clean_spec_mag_norm_log, mask_frames):
    """[B,1,F,T] x 2, frame mask [B,T] (1 = known) -> scalar loss over the gap"""
    H.require_gpu()
    B, C, F, T = output.shape
    if C != 1 or clean_spec_mag_norm_log.shape != output.shape or tuple(mask_frames.shape) != (B, T):
        raise ValueError(f"masked_spectral_mse: output {tuple(output.shape)}, clean {tuple(clean_spec_mag_norm_log.shape)}, "
                         f"mask {tuple(mask_frames.shape)}")
    return MaskedSpectralMSE.apply(output.contiguous().float(), clean_spec_mag_norm_log.contiguous().float(),
                                   mask_frames.contiguous().float())


class InpaintingTrainer(nn.Module):
    def __init__(self, config: InpaintingTrainerConfig, dataset=None):
        super().__init__()
        self.config = config
        if config.use_wandb:
            raise NotImplementedError("wandb logging is outside the MI355X hot path build (no network)")
        self.dataloader = None
        if dataset is None:                                          # the wav folder of data_configuration, before the model
            dataset, self.dataloader = build_device_loader(config.data_configuration, config.dataloader_configuration,
                                                           config.device)

        base_network = UNet(self.config.model_configuration)
        self.model = RestorationWrapper(base_network)
        self.device = config.device
        if config.device == 'cuda':
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.model.to(self.device)

        self.optimizer = make_optimizer(self.model.parameters(), config.optimizer_configuration)

        print(f"Total sample pairs in dataset: {len(dataset)}")
        if self.dataloader is None:
            dl = config.dataloader_configuration
            self.dataloader = torch.utils.data.DataLoader(dataset, batch_size=dl.batch_size, shuffle=dl.shuffle,
                                                          num_workers=dl.num_workers, pin_memory=dl.pin_memory)
        self.step = 0
        self.loss_history: List[float] = []
        self._clip_step = ClippedFlatStep()

    # ---------------------------------------------------------------------------------- reference API
    def base_step(self, batch):
        """(masked_spec [B,2,F,T], mask_frames [B,T], clean_spec [B,2,F,T][, masked_audio]) -> (loss, log)"""
        masked_spec, mask_frames, clean_spec = batch[:3]
        clean_spec_mag_norm_log, mask, masked_spec_mag_log = preprocess_data(clean_spec, masked_spec, mask_frames)
        output = self.model(masked_spec_mag_log, mask)
        loss = masked_spectral_mse(output, clean_spec_mag_norm_log, mask_frames)
        log = {
            'clean_spec': clean_spec.detach(),
            'output': output.detach(),
            'loss': loss.detach(),
        }
        if len(batch) > 3 and isinstance(batch[3], torch.Tensor):
            log['masked_audio'] = batch[3].detach()
        return loss, log

    def validate(self, val_dataloader):
        """mean loss over the loader with the restorer in eval mode (folded BatchNorm, no dropout), then back to train mode"""
        self.model.eval()
        val_losses = []
        try:
            with torch.no_grad():
                for batch in val_dataloader:
                    loss, _ = self.base_step(self._to_device(batch))
                    val_losses.append(loss.item())
        finally:
            self.model.train()
        return sum(val_losses) / len(val_losses)

    # ---------------------------------------------------------------------------------- one optimisation step
    def train_step(self, batch):
        """base_step + zero_grad + backward + clip_grad_norm_(max_grad_norm) + optimizer step (restoration_trainer.py:132-136).
        log['grad_norm'] is the total gradient norm before clipping (a device tensor: no host round trip)."""
        net = self.model.net
        fast = isinstance(self.optimizer, HipAdam)
        net.flat_grad_only = fast
        try:
            loss, log = self.base_step(batch)
            self.optimizer.zero_grad()
            loss.backward()
        finally:
            net.flat_grad_only = False
        if fast:
            log['grad_norm'] = self._clip_step(self.optimizer, net.engine(), self.config.max_grad_norm)
        else:
            log['grad_norm'] = torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=self.config.max_grad_norm)
            self.optimizer.step()
        self.step += 1
        return loss, log

    def _to_device(self, batch):
        masked_spec, mask_frames, clean_spec = batch[:3]
        return (masked_spec.to(self.device), mask_frames.to(self.device), clean_spec.to(self.device))

    def train(self, n_steps=None, n_epochs=None, checkpoint_dir="checkpoints", save_flag=False, val_dataloader=None):
        """training loop (the name shadows nn.Module.train exactly like the reference, restoration_trainer.py:104);
        model mode changes go through self.model.  Returns the per-step loss history."""
        assert n_steps is not None or n_epochs is not None, "Must specify either n_steps or n_epochs"
        os.makedirs(checkpoint_dir, exist_ok=True)
        loss_history: List[float] = []
        val_loss_history: List[float] = []
        loop_loader = LoopLoader(dataloader=self.dataloader, n_steps=n_steps, n_epochs=n_epochs)
        log_dict = None
        for batch in loop_loader:
            loss, log_dict = self.train_step(self._to_device(batch))
            loss_history.append(loss.item())
        self.loss_history.extend(loss_history)
        if loss_history:
            print(f'step {self.step}: Loss: {loss_history[-1]:.4f}')
        if val_dataloader:
            val_loss = self.validate(val_dataloader)
            val_loss_history.append(val_loss)
            print(f"Final Validation Loss: {val_loss:.4f}")
        if save_flag:
            timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
            final_checkpoint_path = os.path.join(checkpoint_dir, f"checkpoint_final_{timestamp}.pt")
            self._get_and_save_metrics(checkpoint_dir, log_dict, n_epochs, n_steps, timestamp)
            self.save_checkpoint(final_checkpoint_path)
        return loss_history

    def save_checkpoint(self, checkpoint_path):
        """{'model_state_dict': UNet state dict (what NPPCModel(pretrained_restoration_model_path=...) loads strictly),
        'optimizer_state_dict', 'step', 'config'}"""
        checkpoint = {
            'model_state_dict': self.model.net.state_dict(),
            'optimizer_state_dict': self.optimizer.state_dict(),
            'step': self.step,
            'config': self.config.model_dump(mode="json"),
        }
        os.makedirs(os.path.dirname(checkpoint_path) or ".", exist_ok=True)
        torch.save(checkpoint, checkpoint_path)
        print(f"Checkpoint saved to {checkpoint_path}")

    def _get_and_save_metrics(self, checkpoint_dir, log_dict, n_epochs, n_steps, timestamp):
        """metrics_final_<timestamp>.json with the reference's fields"""
        dc = self.config.data_configuration
        final_metrics = {
            'timestamp': timestamp,
            'total_steps': self.step,
            'final_loss': log_dict['loss'].item() if log_dict is not None else None,
            'training_config': {
                'n_steps': n_steps,
                'n_epochs': n_epochs,
                'learning_rate': self.config.optimizer_configuration.args.get('lr'),
                'device': self.config.device,
                'batch_size': self.config.dataloader_configuration.batch_size,
                'audio_len': dc.sub_sample_length_seconds,
                'missing_length_seconds': dc.missing_length_seconds,
                'missing_start_seconds': dc.missing_start_seconds,
                'length_audio_seconds': dc.sub_sample_length_seconds,
                'nfft': dc.stft_configuration.nfft,
            }
        }
        metrics_path = os.path.join(checkpoint_dir, f"metrics_final_{timestamp}.json")
        with open(metrics_path, 'w') as f:
            json.dump(final_metrics, f, indent=4)
        return metrics_path
