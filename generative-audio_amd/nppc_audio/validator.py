"""Speech-enhancement NPPC validator on the MI355X kernels: mirrors nppc_audio/validator.py (NPPCAudioValidatorConfig :17-21,
NPPCAudioValidator :24-314).

`visualize_pc_spectrograms` writes what the reference writes for a noisy clip: under <save_dir>/audio/ the peak-normalised
noisy, clean and enhanced waveforms and every `enhanced + alpha * PC_k` (alphas = linspace(-3, 3, 6)), all K * 6 + 1 inverse
STFTs as one batched launch (ops.pc_direction_waveforms), and under <save_dir>/spectrograms/ the (1 + K) x 9 sheet
pc_spectrograms_variations.png:
    row 0   noisy, clean, enhanced (autoscaled dB), Error (Enh - Clean) in [-60, 0] dB, five blank cells
    row k   PC k in [-60, 0] dB, then enhanced + alpha * PC k for the six alphas (autoscaled dB), two blank cells
drawn and encoded on the device (nppc_audio/spectrogram_png.py): the complex planes never leave it.  Titles, axes and colour
bars are not drawn and no pixel parity with matplotlib's figure is claimed; the sheet's fixed layout carries what the titles
say.  A batch [B, T] is accepted too: one sheet and one set of wav files per item, under <save_dir>/item_<b>/ when B > 1.
"""
from pathlib import Path
from typing import Literal, Optional

import pydantic
import torch

from . import _hip as H
from . import flac as FL
from . import ops
from . import png as PNG
from .nppc_model import NPPCModel, NPPCModelConfig
from .spectrogram_png import Cell, Sheet, render_indices, render_png

__all__ = ["NPPCAudioValidatorConfig", "NPPCAudioValidator", "pc_variation_sheet", "ALPHAS", "SHEET_COLUMNS"]

ALPHAS = tuple(float(a) for a in torch.linspace(-3, 3, 6))        # validator.py:246
SHEET_COLUMNS = 9                                                  # validator.py:204
DB_RANGE = (-60.0, 0.0)                                            # the two panels the reference gives vmin and vmax
NOISY, CLEAN, ENHANCED, PC = 0, 1, 2, 3                            # planes of the stacked tensor


def pc_variation_sheet(item, K, has_clean, sx=1, sy=1, gutter=4):
    """the (1 + K) x 9 sheet of visualize_pc_spectrograms over the complex planes (noisy, clean, enhanced, pc_1 .. pc_K)"""
    db = dict(g="db")
    fixed = dict(g="db", vmin=DB_RANGE[0], vmax=DB_RANGE[1])
    top = [Cell(p=NOISY, **db), Cell(p=CLEAN, **db) if has_clean else None, Cell(p=ENHANCED, **db),
           Cell(p=ENHANCED, q=CLEAN, alpha=-1.0, **fixed) if has_clean else None]
    rows = [top + [None] * (SHEET_COLUMNS - len(top))]
    for k in range(K):
        row = [Cell(q=PC + k, **fixed)] + [Cell(p=ENHANCED, q=PC + k, alpha=a, **db) for a in ALPHAS]
        rows.append(row + [None] * (SHEET_COLUMNS - len(row)))
    return Sheet(item, rows, sx=sx, sy=sy, gutter=gutter)


def stack_planes(noisy, clean, enhanced, pcs):
    """(re, im) pairs [B,F,T] (clean may be None: zeros) and the directions ([B,K,F,T], [B,K,F,T]) -> [B, 3 + K, 2, F, T]"""
    n = torch.stack(noisy, dim=1)
    c = torch.stack(clean, dim=1) if clean is not None else torch.zeros_like(n)
    e = torch.stack(enhanced, dim=1)
    d = torch.stack(pcs, dim=2)                                    # [B,K,2,F,T]
    return torch.cat([n[:, None], c[:, None], e[:, None], d], dim=1).float().contiguous()


class NPPCAudioValidatorConfig(pydantic.BaseModel):
    nppc_audio_model_configuration: NPPCModelConfig
    checkpoint_path: str
    metrics_path: Optional[str] = None
    device: Literal["cpu", "cuda"] = "cuda"


class NPPCAudioValidator:
    def __init__(self, config: NPPCAudioValidatorConfig):
        self.config = config
        self.device = torch.device(config.device)
        self.nppc_model = NPPCModel(config.nppc_audio_model_configuration)
        model_path = Path(config.checkpoint_path).expanduser().absolute()
        if not model_path.exists():
            raise FileNotFoundError(f"Model file not found: {model_path}")
        try:
            checkpoint = torch.load(model_path.as_posix(), map_location="cpu")
            self.nppc_model.load_state_dict(checkpoint['model_state_dict'])
        except Exception as e:
            raise RuntimeError(f"Failed to load model: {str(e)}")
        self.nppc_model.to(self.device)
        self.nppc_model.eval()

    # ---- the pieces --------------------------------------------------------------------------------------------------------
    def _stft_config(self):
        st = self.config.nppc_audio_model_configuration.stft_configuration
        if st.win_length != st.nfft:
            raise NotImplementedError("win_length == nfft is the STFT configuration built for MI355X")
        return st

    def _stft_parts(self, audio):
        st = self._stft_config()
        _, re, im = ops.stft(audio.to(self.device).float(), st.nfft, st.hop_length, want_mag=False)
        return re, im

    def audio_to_stft(self, input_audio):
        """complex STFT [B,F,T] of input_audio [B,T] (validator.py:304-314)"""
        H.require_gpu()
        return torch.complex(*self._stft_parts(input_audio))

    def _direction_parts(self, noisy):
        with torch.no_grad():
            w_mat = self.nppc_model(noisy)                          # [B,K,2,F,T] compressed cIRM directions
            re, im = self._stft_parts(noisy)
            return w_mat, ops.crm_directions_to_spectrograms(w_mat, re, im)

    def _crm_directions_to_spectograms(self, noisy_audio):
        """the K directions as complex spectrograms: a list of K tensors [B,F,T] (validator.py:55-102)"""
        H.require_gpu()
        _, (d_re, d_im) = self._direction_parts(noisy_audio.to(self.device).float())
        return [torch.complex(d_re[:, k], d_im[:, k]) for k in range(d_re.shape[1])]

    @staticmethod
    def _normalised(x):
        return x / (x.abs().amax(dim=-1, keepdim=True) + 1e-8)      # validator.py:126

    def save_audio_files(self, audio_dir, noisy_audio, clean_audio, enhanced_complex, stft_config=None, window=None):
        """noisy.wav, clean.wav (when given) and enhanced.wav under audio_dir, each peak-normalised, 16-bit at 16 kHz
        (validator.py:104-146).  noisy_audio, clean_audio [1,T]; enhanced_complex [1,F,T]; `window` is accepted for the
        reference's signature (the kernels' window is the periodic Hann of win_length == nfft)."""
        H.require_gpu()
        st = stft_config or self._stft_config()
        audio_dir = Path(audio_dir)
        e = enhanced_complex.to(self.device)
        enhanced = ops.istft(e.real.float().contiguous(), e.imag.float().contiguous(), st.nfft, st.hop_length, noisy_audio.shape[1])
        names, waves = ["noisy.wav"], [noisy_audio.to(self.device).float()]
        if clean_audio is not None:
            names.append("clean.wav"), waves.append(clean_audio.to(self.device).float())
        names.append("enhanced.wav"), waves.append(enhanced)
        paths = [audio_dir / n for n in names]
        FL.write_waves(paths, self._normalised(torch.cat(waves)), 16000, fmt="wav")
        return paths

    # ---- the sheet ---------------------------------------------------------------------------------------------------------
    def visualize_pc_spectrograms(self, noisy_audio: torch.Tensor, clean_audio: Optional[torch.Tensor] = None, save_dir=None,
                                  sx=1, sy=1, gutter=4, palette="viridis"):
        """noisy_audio [B,T] (the reference takes [1,T]), clean_audio [B,T] or None -> writes the audio files and the sheet
        (module docstring) and returns what the reference returns: (the K directions as complex spectrograms [B,F,T],
        the enhanced spectrogram in dB [B,F,T])."""
        H.require_gpu()
        if noisy_audio.dim() != 2:
            raise ValueError(f"Expected noisy_audio shape [B,T], got {tuple(noisy_audio.shape)}")
        if clean_audio is not None and clean_audio.shape != noisy_audio.shape:
            raise ValueError("Clean and noisy audio must have the same shape")
        if save_dir is None:
            raise ValueError("visualize_pc_spectrograms writes files: pass save_dir")
        st = self._stft_config()
        B, L = noisy_audio.shape
        with torch.no_grad():
            noisy = noisy_audio.to(self.device).float().contiguous()
            clean = clean_audio.to(self.device).float().contiguous() if clean_audio is not None else None
            w_mat, (d_re, d_im) = self._direction_parts(noisy)
            K = w_mat.shape[1]
            n_re, n_im = self._stft_parts(noisy)
            pred_crm = self.nppc_model.get_pred_crm(noisy)
            _, e_re, e_im = ops.cirm_decompress_apply(pred_crm, n_re, n_im)
            enhanced, variants = ops.pc_direction_waveforms(pred_crm, w_mat, ALPHAS, n_re, n_im, L, st.nfft, st.hop_length)
            planes = stack_planes((n_re, n_im), self._stft_parts(clean) if clean is not None else None, (e_re, e_im), (d_re, d_im))
            sheets = [pc_variation_sheet(b, K, clean is not None, sx, sy, gutter) for b in range(B)]
            files = render_png(planes, sheets, palette=palette)
            root = Path(save_dir).absolute()
            dirs = [root / f"item_{b}" if B > 1 else root for b in range(B)]
            PNG.write_files([d / "spectrograms" / "pc_spectrograms_variations.png" for d in dirs], files)
            names, waves = [], []
            for b, d in enumerate(dirs):
                names.append(d / "audio" / "noisy.wav"), waves.append(noisy[b])
                if clean is not None:
                    names.append(d / "audio" / "clean.wav"), waves.append(clean[b])
                names.append(d / "audio" / "enhanced.wav"), waves.append(enhanced[b])
                for k in range(K):
                    for a, alpha in enumerate(ALPHAS):
                        names.append(d / "audio" / f"pc{k}_alpha{alpha:.1f}.wav"), waves.append(variants[b, k, a])
            FL.write_waves(names, self._normalised(torch.stack(waves)), 16000, fmt="wav")
            pc_specs = [torch.complex(d_re[:, k], d_im[:, k]) for k in range(K)]
            enhanced_spec_db = 20 * torch.log10(torch.sqrt(e_re * e_re + e_im * e_im) + 1e-8)
        return pc_specs, enhanced_spec_db

    def visualize_pc_pitch(self, noisy_audio: torch.Tensor, alphas=ALPHAS, save_dir=None, individual=True, sx=8, plot_height=240,
                           backend="auto", fmin=80.0, fmax=400.0, sr=16000):
        """noisy_audio [B,T] -> tracks the contours of the enhanced waveform and of every `enhanced + alpha * PC_k` on the
        device, writes <save_dir>/pitch/pc_<k>_pitch.png (individual) and <save_dir>/pitch/pitch_comparison.png (under
        <save_dir>/item_<b>/ when B > 1), the whole batch in one curve_png.render_png call, and returns (paths, the dict of
        pc_pitch.pc_direction_pitch)."""
        from . import curve_png as CP
        from .pc_pitch import pc_direction_pitch
        H.require_gpu()
        if noisy_audio.dim() != 2:
            raise ValueError(f"Expected noisy_audio shape [B,T], got {tuple(noisy_audio.shape)}")
        if save_dir is None:
            raise ValueError("visualize_pc_pitch writes files: pass save_dir")
        alphas = [float(a) for a in alphas]
        pitch = pc_direction_pitch(self.nppc_model, noisy_audio.to(self.device).float().contiguous(), alphas, fmin=fmin, fmax=fmax, sr=sr)
        B, K, A, T = pitch["f0"].shape
        hop = 2048 // 4                                             # pitch.pyin's default frame and hop
        names, sheets = CP.pitch_sheets(B, K, alphas, T, hop / sr, individual=individual, sx=sx, plot_height=plot_height, fmin=fmin,
                                        fmax=fmax, markers=False)
        files = CP.render_png(CP.stack_contours(pitch), sheets, backend=backend)
        root = Path(save_dir).absolute()
        paths = [(root / f"item_{b}" if B > 1 else root) / "pitch" / name for b, name in names]
        PNG.write_files(paths, files)
        return paths, pitch

    def save_posterior_samples(self, noisy_audio: torch.Tensor, save_dir, n_samples=8, seed=0, fmt="flac", sx=1, sy=1,
                               palette="viridis", flac_predictor="fixed"):
        """noisy_audio [B,T] -> n_samples waveforms drawn from the posterior the net states (posterior.py: z ~ N(0, 1) along
        every direction, compressed domain), written peak-normalised as <save_dir>/posterior/sample_<s>.<fmt>, and the
        standard deviation of the samples' spectrogram magnitudes in dB as <save_dir>/posterior/std_spec.png (under
        <save_dir>/item_<b>/ when B > 1).  All samples and both statistics come from one fused launch.  flac_predictor: the
        FLAC encoder's predictor, "fixed" or "lpc" (flac.encode_pcm).  Returns the paths."""
        from .posterior import PosteriorSampler
        H.require_gpu()
        if noisy_audio.dim() != 2:
            raise ValueError(f"Expected noisy_audio shape [B,T], got {tuple(noisy_audio.shape)}")
        if n_samples < 2:
            raise ValueError("save_posterior_samples draws at least 2 samples (it writes their standard deviation)")
        B = noisy_audio.shape[0]
        r = PosteriorSampler(model=self.nppc_model).sample(noisy_audio, n_samples=n_samples, seed=seed, spec_stats=True)
        root = Path(save_dir).absolute()
        dirs = [(root / f"item_{b}" if B > 1 else root) / "posterior" for b in range(B)]
        waves = [d / f"sample_{s}.{fmt}" for d in dirs for s in range(n_samples)]
        FL.write_waves(waves, self._normalised(r["samples"].reshape(B * n_samples, -1)), 16000, fmt=fmt, predictor=flac_predictor)
        std = torch.stack((r["mag_std"], torch.zeros_like(r["mag_std"])), dim=1)[:, None].contiguous()      # [B,1,2,F,T]
        pngs = [d / "std_spec.png" for d in dirs]
        PNG.write_files(pngs, render_png(std, [Sheet(b, [[Cell(p=0, g="db")]], sx=sx, sy=sy) for b in range(B)], palette=palette))
        return waves + pngs

    def pc_spectrogram_indices(self, planes, has_clean=True, sx=1, sy=1, gutter=4):
        """the sheets of stacked complex planes [B, 3 + K, 2, F, T] (stack_planes) as index images: for tests and for
        callers who want pixels"""
        K = planes.shape[1] - 3
        return render_indices(planes, [pc_variation_sheet(b, K, has_clean, sx, sy, gutter) for b in range(planes.shape[0])])
