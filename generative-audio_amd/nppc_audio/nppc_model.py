"""Reference surface nppc_audio/nppc_model.py:13-132 on the HIP kernels.

NPPCModel = frozen FullSubNet+ restorer + AudioPCWrapper.  The reference executes the restorer twice
and the noisy STFT three times per train step (nppc_model.py:88,95,122,129; trainer.py:354); both are
deterministic, so this build memoises them per input tensor: `forward` stores the compressed cIRM and
`get_pred_crm` on the same waveform returns it without re-running the kernels.
"""
from pathlib import Path
from typing import Literal, Union

import pydantic
import torch
import torch.nn as nn

from . import _hip as H
from . import ops
from .fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig, check_frames
from .pc_wrapper import AudioPCWrapper, AudioPCWrapperConfig


class StftConfig(pydantic.BaseModel):      # utils.py:14-17
    nfft: int = 512
    hop_length: int = 256
    win_length: int = 512


def preload_model(model_path: Union[Path, str], model: FullSubNet_Plus) -> FullSubNet_Plus:
    """utils.py:82-98: '*.tar' checkpoint = {"model": state_dict}, loaded strict=False."""
    model_path = Path(model_path).expanduser().absolute()
    assert model_path.exists(), f"The file {model_path.as_posix()} is not exist. please check path."
    ck = torch.load(model_path.as_posix(), map_location="cpu")
    model.load_state_dict(ck["model"], strict=False)
    return model


def load_pretrained_model(model_path, model_config: FullSubNetPlusConfig) -> FullSubNet_Plus:
    return preload_model(model_path, FullSubNet_Plus(model_config))


class NPPCModelConfig(pydantic.BaseModel):
    pretrained_restoration_model_configuration: FullSubNetPlusConfig
    pretrained_restoration_model_path: str
    audio_pc_wrapper_configuration: AudioPCWrapperConfig
    stft_configuration: StftConfig
    device: Literal['cpu', 'cuda'] = 'cuda'

    def make_instance(self):
        return NPPCModel(self)


class NPPCModel(nn.Module):
    def __init__(self, config: NPPCModelConfig):
        super().__init__()
        self.config = config
        self.pretrained_restoration_model = load_pretrained_model(config.pretrained_restoration_model_path,
                                                                  config.pretrained_restoration_model_configuration)
        self.device = config.device
        if config.device == 'cuda':
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.pretrained_restoration_model.to(self.device)
        self.pretrained_restoration_model.eval()
        self.audio_pc_wrapper = AudioPCWrapper(config.audio_pc_wrapper_configuration)
        self.audio_pc_wrapper.to(self.device)
        self._memo = None

    # -- shared front end ------------------------------------------------------------------------
    def _front(self, noisy_waveform, reuse=True, lengths=None):
        """STFT + frozen restorer.  `forward` always recomputes (reuse=False) and leaves the result for the
        `get_pred_crm` / gt-mask calls that follow on the SAME tensor within the step.

        lengths [B] (host ints; a ragged batch padded to noisy_waveform's width): the ragged STFT and the ragged restorer
        forward; the result also carries `frames` (device int32 [B]) and `lengths` (host list)."""
        H.require_gpu()
        # the memo holds the input tensor itself: identity + version (+ the lengths) is then a safe key (an address alone
        # could be recycled by the caching allocator for the next batch)
        m = self._memo
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            raise ValueError("lengths must live on the host (a list, or a CPU tensor such as RaggedBatch.lengths): they are "
                             "checked item by item, and a device tensor would have to be read back")
        lkey = None if lengths is None else tuple(int(n) for n in torch.as_tensor(lengths).reshape(-1).tolist())
        if reuse and m is not None and m[0] is noisy_waveform and m[1] == noisy_waveform._version and m[3] == lkey:
            return m[2]
        st = self.config.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        if lkey is None:
            mag, re, im = ops.stft(noisy_waveform, st.nfft, st.hop_length)
            with torch.no_grad():
                pred_crm = self.pretrained_restoration_model(mag[:, None], re[:, None], im[:, None])
            out = dict(mag=mag, re=re, im=im, pred_crm=pred_crm)
        else:
            B = noisy_waveform.shape[0] if noisy_waveform.dim() > 1 else 1
            ops.ragged_lengths(lkey, B, noisy_waveform.shape[-1], st.nfft // 2, "cpu")      # ValueError names the item
            tb = ops.stft_frames(list(lkey), st.hop_length)
            check_frames(tb, B, 1 + noisy_waveform.shape[-1] // st.hop_length, self.pretrained_restoration_model.kersize)
            check_frames(tb, B, 1 + noisy_waveform.shape[-1] // st.hop_length, self.audio_pc_wrapper.net.kersize)
            mag, re, im = ops.stft(noisy_waveform, st.nfft, st.hop_length, lengths=list(lkey))
            frames = torch.tensor(tb, dtype=torch.int32).to(mag.device)
            with torch.no_grad():
                pred_crm = self.pretrained_restoration_model(mag[:, None], re[:, None], im[:, None], frames=frames)
            out = dict(mag=mag, re=re, im=im, pred_crm=pred_crm, frames=frames, lengths=list(lkey))
        self._memo = (noisy_waveform, noisy_waveform._version, out, lkey)
        return out

    def forward(self, noisy_waveform: torch.Tensor, lengths=None) -> torch.Tensor:
        """[B, L] -> w_mat [B, n_dirs, 2, F', T] (nppc_model.py:58-115)

        lengths [B] (extension, inference only, under torch.no_grad()): a ragged batch.  Item b's directions are those of
        its first L_b samples run alone: all F bins (no drop-band), 0 at frames t >= 1 + L_b // hop; samples at or past
        L_b are never read."""
        f = self._front(noisy_waveform, reuse=False, lengths=lengths)
        # decompress + the reference's swapped mask application (conj(mask) * noisy), utils.py:241-249
        # (ragged: the restorer's mask and the noisy STFT are 0 from T_b on, and so are the enhanced maps)
        _, emag, ere, eim = ops.cirm_decompress_apply_conj(f["pred_crm"], f["re"], f["im"])
        if lengths is not None:
            return self.audio_pc_wrapper(f["mag"][:, None], f["re"][:, None], f["im"][:, None],
                                         emag[:, None], ere[:, None], eim[:, None], frames=f["frames"])
        return self.audio_pc_wrapper(f["mag"][:, None], f["re"][:, None], f["im"][:, None],
                                     emag[:, None], ere[:, None], eim[:, None])

    def get_pred_crm(self, noisy_waveform: torch.Tensor, lengths=None) -> torch.Tensor:
        """compressed, un-drop-banded restorer output [B,2,F,T] (nppc_model.py:117-132); lengths: see forward"""
        return self._front(noisy_waveform, lengths=lengths)["pred_crm"]
