"""Inpainting NPPC trainer on the MI355X kernels: mirrors nppc_audio/inpainting/trainer/nppc_trainer.py
(NPPCAudioInpaintingTrainerConfig :28-46, NPPCAudioInpaintingTrainer.__init__ :49-93, train :115-166,
base_step :338-385, save_checkpoint :604-618, _calculate_final_objective :680-687).

Differences, deliberately: the frozen restorer runs once per step (the reference runs it twice on the same input);
clip_grad_norm_ + Adam run as sum-of-squares + ONE fused kernel over the flat gradient with the clip coefficient
computed on the device (no host round trip); wandb logging and plotting are not built.  Without a
`dataset=` the trainer builds `data.AudioInpaintingDataset` + `data.InpaintingDeviceLoader` from its data_configuration:
a wav folder decoded once and minibatches assembled on the device, with the gap placed by an energy voice-activity
detector (`vad.py`) where the reference uses silero-vad.
"""
import os
from datetime import datetime
from pathlib import Path
from typing import List, Optional, Union

import pydantic
import torch
import torch.nn as nn

from ...data import DataLoaderConfig
from ...nppc_model import StftConfig
from ...pc_ops import NPPCLoss, planes, second_moment_weight
from ...trainer import ClippedFlatStep, HipAdam, LoopLoader, OptimizerConfig, make_optimizer
from ..nppc.nppc_model import NPPCModel, NPPCModelConfig
from ..utils import preprocess_data
from ..vad import EnergyVadConfig


class AudioInpaintingConfig(pydantic.BaseModel):
    """dataset/audio_dataset_inpainting.py:60-83 (the fields).  vad_configuration (not in the reference): the constants of
    the energy voice-activity detector that use_vad selects here; None = EnergyVadConfig()'s defaults."""
    clean_path: Union[str, Path]
    sample_rate: int = 16000
    missing_length_seconds: float = 0.128
    missing_start_seconds: Optional[float] = None
    missing_end_seconds: Optional[float] = None
    sub_sample_length_seconds: float = 3.0
    target_dB_FS: float = -25.0
    target_dB_FS_floating_value: float = 0.0
    stft_configuration: StftConfig
    use_vad: bool = False
    seed: Optional[int] = None
    is_random_sub_sample: bool = True
    vad_configuration: Optional[EnergyVadConfig] = None


def build_device_loader(data_configuration, dataloader_configuration, device):
    """the stock data path of both inpainting trainers: (AudioInpaintingDataset, InpaintingDeviceLoader) from the parsed
    configuration.  The dataset is built first and raises ValueError (naming the dataset= way in) for a missing or empty
    folder before anything touches the device.  Of dataloader_configuration only batch_size and shuffle apply (the last
    batch is kept): num_workers and pin_memory have no meaning for a loader that assembles its batches on the device and
    are ignored.  Both trainers set up their data before their model, with or without dataset=, so a data error comes
    before a model or checkpoint error."""
    from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
    from ..data import AudioInpaintingDataset, InpaintingDeviceLoader
    dataset = AudioInpaintingDataset(data_configuration)
    dl = dataloader_configuration
    sampler = RandomSampler(dataset) if dl.shuffle else SequentialSampler(dataset)
    return dataset, InpaintingDeviceLoader(dataset, BatchSampler(sampler, dl.batch_size, drop_last=False), device=device)


class NPPCAudioInpaintingTrainerConfig(pydantic.BaseModel):
    nppc_model_configuration: NPPCModelConfig
    data_configuration: AudioInpaintingConfig
    dataloader_configuration: DataLoaderConfig
    optimizer_configuration: OptimizerConfig
    device: str = "cuda"
    save_interval: int = 10
    log_interval: int = 100
    second_moment_loss_lambda: float = 1.0
    second_moment_loss_grace: int = 500
    max_grad_norm: float = 1.0
    use_wandb: bool = False
    wandb_project_name: Optional[str] = "generative-audio"
    wandb_run_name: Optional[str] = None
    wandb_tags: Optional[List[str]] = None
    wandb_artifact_name: str = "nppc_inpainting_model"


def inpainting_base_step(model, batch, step, grace, lam_cfg):
    """nppc_trainer.py:338-385: (masked_spec [B,2,F,T], mask [B,T], clean_spec [B,2,F,T]) ->
    (reconst_err [B], objective [], log)."""
    masked_spec, mask, clean_spec = batch
    clean_norm, mask4, masked_norm = preprocess_data(clean_spec, masked_spec, mask)
    w_mat = model(masked_norm, mask4)                                   # [B, n_dirs, F, T]
    pred = model.get_pred_spec_mag_norm(masked_norm, mask4)             # memoised: the restorer ran inside model()
    B, K, F, T = w_mat.shape
    lam = second_moment_weight(step, grace, lam_cfg)
    # real vectors = complex vectors with a zero imaginary plane; eps 1e-6 inside the norms (:355,:363)
    reconst_err, objective, err_norm, pr, _, _, w_norms, sm = NPPCLoss.apply(
        planes(w_mat), planes(clean_norm).view(B, 2, F, T), planes(pred).view(B, 2, F, T), lam, 1e-6, 1)
    log = {
        'w_mat': w_mat.detach(),
        'err_norm': err_norm.detach(),
        'err_proj': pr.detach(),
        'w_norms': w_norms.detach(),
        'reconst_err': reconst_err.detach(),
        'second_moment_mse': sm.detach(),
        'objective': objective.detach(),
    }
    return reconst_err, objective, log


class NPPCAudioInpaintingTrainer(nn.Module):
    def __init__(self, config: NPPCAudioInpaintingTrainerConfig, dataset=None):
        super().__init__()
        self.config = config
        if config.use_wandb:
            raise NotImplementedError("wandb logging is outside the MI355X hot path build (no network)")
        self.device = self.config.device
        if dataset is None:                                          # the wav folder of data_configuration, before the model
            dataset, self.dataloader = build_device_loader(config.data_configuration, config.dataloader_configuration,
                                                           self.device)
        else:
            dl = config.dataloader_configuration
            self.dataloader = torch.utils.data.DataLoader(dataset, batch_size=dl.batch_size, shuffle=dl.shuffle,
                                                          num_workers=dl.num_workers, pin_memory=dl.pin_memory)
        print(f"Total sample pairs in dataset: {len(dataset)}")
        self.nppc_model = NPPCModel(self.config.nppc_model_configuration)
        self.step = 0
        self.optimizer = make_optimizer(self.nppc_model.parameters(), config.optimizer_configuration)
        self._clip_step = ClippedFlatStep()
        self.val_loss_history = []
        self.val_reconst_err_history = []

    # ---------------------------------------------------------------------------------- reference API
    def base_step(self, batch):
        return inpainting_base_step(self.nppc_model, batch, self.step, self.config.second_moment_loss_grace,
                                    self.config.second_moment_loss_lambda)

    def base_step2(self, batch, n_mc_samples=50, ragged_gaps=False):
        """nppc_trainer.py:244-336: the alternative target -- the NPPC directions are fitted to the MC-dropout + PCA
        components of the restorer (50 stochastic passes with the WHOLE restorer in train mode, as the reference's
        `restoration_model.train()` does: BatchNorm uses batch statistics and its running buffers move).
        ragged_gaps=True accepts a batch whose items have different numbers of gap frames
        (mc_baseline.calculate_unet_baseline_ragged); the default raises ValueError for one, as before."""
        from ..mc_baseline import PairProjectionLoss, calculate_unet_baseline, calculate_unet_baseline_ragged
        masked_spec, mask, clean_spec = batch
        clean_norm, mask4, masked_norm = preprocess_data(clean_spec, masked_spec, mask)
        w_mat = self.nppc_model(masked_norm, mask4)                      # [B, n_dirs, F, T]
        restoration_model = self.nppc_model.pretrained_restoration_model
        restoration_model.train()
        try:
            baseline = calculate_unet_baseline_ragged if ragged_gaps else calculate_unet_baseline
            mc = baseline(restoration_model, masked_norm, mask4, n_mc_samples=n_mc_samples, n_components=w_mat.shape[1])
        finally:
            restoration_model.eval()
        w_mc, singular_values = mc['scaled_principal_components'], mc['singular_vals']
        lam = second_moment_weight(self.step, self.config.second_moment_loss_grace, self.config.second_moment_loss_lambda)
        reconst_err, objective, proj, w_norms, second_moment_mse = PairProjectionLoss.apply(w_mat, w_mc, singular_values, lam)
        log = {
            'w_mat': w_mat.detach(),
            'w_mc': w_mc.detach(),
            'proj_W_mc_on_W_nppc': proj.detach(),
            'w_norms': w_norms.detach(),
            'reconst_err': reconst_err.detach(),
            'second_moment_mse': second_moment_mse.detach(),
            'objective': objective.detach(),
        }
        return reconst_err, objective, log

    def _calculate_final_objective(self, reconst_err, second_moment_mse):
        lam = second_moment_weight(self.step, self.config.second_moment_loss_grace, self.config.second_moment_loss_lambda)
        return reconst_err.mean() + lam * second_moment_mse.mean()

    # ---------------------------------------------------------------------------------- one optimisation step
    def train_step(self, batch):
        """forward + loss + backward + clip_grad_norm_(max_grad_norm) + optimizer step (nppc_trainer.py:145-154)"""
        net = self.nppc_model.pc_wrapper.net
        fast = isinstance(self.optimizer, HipAdam)
        net.flat_grad_only = fast
        try:
            reconst_err, objective, log = self.base_step(batch)
            self.optimizer.zero_grad()
            objective.backward()
        finally:
            net.flat_grad_only = False
        if fast:
            self._clip_step(self.optimizer, net.engine(), self.config.max_grad_norm)
        else:
            torch.nn.utils.clip_grad_norm_(self.nppc_model.parameters(), max_norm=self.config.max_grad_norm)
            self.optimizer.step()
        self.step += 1
        return reconst_err, objective, log

    def train(self, n_steps=None, n_epochs=None, checkpoint_dir="checkpoints", save_flag=True, val_dataloader=None,
              log_every=None):
        """training loop (the name shadows nn.Module.train exactly like the reference, nppc_trainer.py:115).
        val_dataloader: validated whenever the step counter, read before the step, is a multiple of log_interval
        (:170-176); the results are appended to self.val_loss_history / self.val_reconst_err_history, which belong to the
        trainer and keep growing over successive train() calls (the reference keeps them in locals and drops them)."""
        os.makedirs(checkpoint_dir, exist_ok=True)
        loop_loader = LoopLoader(dataloader=self.dataloader, n_steps=n_steps, n_epochs=n_epochs)
        log_every = log_every or self.config.log_interval
        for it, batch in enumerate(loop_loader):
            masked_spec, mask_frames, clean_spec = batch[:3]
            batch = (masked_spec.to(self.device), mask_frames.to(self.device), clean_spec.to(self.device))
            step_before = self.step                                   # the reference tests its counter before advancing it
            reconst_err, objective, log_dict = self.train_step(batch)
            if it % log_every == 0 or it + 1 == len(loop_loader):
                print(f'step {self.step}: Objective: {objective.item():.4f} | '
                      f'Second Moment MSE: {log_dict["second_moment_mse"].mean().item():.4f} | '
                      f'Reconstract Error: {reconst_err.mean().item():.4f}')
            if val_dataloader is not None and step_before % self.config.log_interval == 0:      # nppc_trainer.py:170-176
                val_loss, val_reconst_err = self.validate(val_dataloader)
                self.val_loss_history.append(val_loss)
                self.val_reconst_err_history.append(val_reconst_err)
                print(f" | Validation objective at Step {step_before}: {val_loss:.4f}")
                print(f" | Validation Reconstract Error at Step {step_before}: {val_reconst_err:.4f}")
        if save_flag:
            timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
            self.save_checkpoint(os.path.join(checkpoint_dir, f"checkpoint_final_{timestamp}.pt"))

    def validate(self, val_dataloader):
        """nppc_trainer.py:689-706: mean objective and mean reconstruction error of base_step over a held-out loader, in
        eval mode under no_grad -> (avg_objective, avg_reconst_err).  Batches are (masked_spec, mask, clean_spec) or the
        five-tuple of the reference's collate_fn (the first three are used).  Nothing the optimiser or a later training
        step sees changes: no gradient, no BatchNorm running-buffer update, and the training flags are put back as they
        were (the reference ends with .train(); the frozen restorer stays in eval mode either way)."""
        model = self.nppc_model
        was_training = {m: m.training for m in model.modules()}
        model.eval()
        val_losses, val_reconst_err = [], []
        try:
            with torch.no_grad():
                for batch in val_dataloader:
                    masked_spec, mask, clean_spec = (x.to(self.device) for x in batch[:3])
                    reconst_err, objective, _ = self.base_step((masked_spec, mask, clean_spec))
                    val_losses.append(objective.item())
                    val_reconst_err.append(reconst_err.mean().item())
        finally:
            for m, flag in was_training.items():
                m.training = flag
            model._memo = None                                    # the memoised restorer output belongs to a held-out batch
        if not val_losses:
            raise ValueError("the validation dataloader yielded no batches")
        return sum(val_losses) / len(val_losses), sum(val_reconst_err) / len(val_reconst_err)

    def save_checkpoint(self, checkpoint_path):
        checkpoint = {
            'model_state_dict': self.nppc_model.state_dict(),
            'optimizer_state_dict': self.optimizer.state_dict(),
            'step': self.step,
        }
        os.makedirs(os.path.dirname(checkpoint_path) or ".", exist_ok=True)
        torch.save(checkpoint, checkpoint_path)
        print(f"Checkpoint saved to {checkpoint_path}")
