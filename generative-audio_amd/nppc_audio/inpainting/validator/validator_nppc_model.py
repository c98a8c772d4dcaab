"""Inpainting NPPC validator on the MI355X kernels: mirrors nppc_audio/inpainting/validator/validator_nppc_model.py
(NPPCModelValidatorConfig :905-910, NPPCModelValidator :913-1027, save_pc_audio_variations :528-659,
compute_metrics :742-828, save_metrics_to_json :831-859).

The reference validates one held-out sample at a time: direction net, MC-dropout + PCA baseline, compute_metrics on the
host, K x A inverse STFTs one by one.  Here a whole uniform batch goes through each stage at once: the baseline is
mc_baseline.calculate_unet_baseline (batched PCA), the metrics come from one Gram launch per batch
(mc_baseline.metrics_gram_batch) and ONE device-to-host copy per `validate_dataloader` call, and the K x A + 1 waveforms
of `pc_audio_variations` come from one launch whose complex spectrograms never reach memory.

`validate_batch(..., phase="griffin_lim")` adds waveforms that do not use the clean phase at all (inpainting/phase.py:
Griffin-Lim restricted to the gap, the damaged recording's STFT held fixed), which is what a recording with a real gap allows.

`validate_batch(..., pitch=True)` adds the f0 contours of plot_pitch_comparison (:19-270) for the clean waveform and every
variation, tracked on the device (nppc_audio/pitch.py), and what each direction does to them.

`save_pc_audio_variations` writes what validate_batch(..., alphas=) synthesised in the reference's layout, as FLAC encoded
on the device (nppc_audio/flac.py) or as wav.

`save_pc_spectrograms` writes the spectrogram panels of plot_pc_spectrograms (:273-478) under the reference's file names and
one sheet per sample, as PNG files drawn and encoded on the device (nppc_audio/spectrogram_png.py): the whole batch in one
device call.  Titles, axes and colour bars are not drawn; no pixel parity with matplotlib's figures is claimed.

`save_pc_pitch_plots` writes the pitch figures of plot_pitch_comparison (:19-154) from the contours of
validate_batch(..., pitch=True): pc_<k>_pitch.png per direction and the stacked pitch_comparison.png, as PNG files drawn and
encoded on the device (nppc_audio/curve_png.py), the whole batch in one device call.  Not reproduced: matplotlib's 0.7 line
alpha (paint order stands in for it: later alphas lie over earlier ones), titles, axis names and anti-aliasing; no pixel
parity with matplotlib's figures is claimed.

Outside this build: whisper / phoneme transcription, wandb.
Splicing a restoration or a variation into the full source recording is inpainting/restore.py (RecordingRestorer).
"""
import json
from pathlib import Path
from typing import Optional

import numpy as np
import pydantic
import torch

from ... import _hip as H
from ... import ops
from ... import pitch as PT
from .. import mc_baseline as MB
from .. import phase as PH
from ..nppc.nppc_model import NPPCModel, NPPCModelConfig
from ..utils import preprocess_data

__all__ = ["NPPCModelValidatorConfig", "NPPCModelValidator", "pc_audio_variations", "compute_metrics",
           "compute_metrics_batch", "save_metrics_to_json", "default_alphas", "save_pc_audio_variations",
           "save_pc_spectrograms", "pc_spectrogram_sheets", "save_pc_pitch_plots", "pitch_windows", "save_posterior_samples",
           "posterior_std_planes"]

compute_metrics = MB.compute_metrics
compute_metrics_batch = MB.compute_metrics_batch


def default_alphas(device=None):
    """the reference's sweep, validator_nppc_model.py:972"""
    return torch.arange(-3, 3.5, 0.5, device=device)


def pc_audio_variations(clean_spec_mag_norm_log, pred_spec_mag, pc_directions_mag, clean_spec, alphas, mean, std,
                        n_fft=255, hop_length=128, length=None):
    """save_pc_audio_variations (:553-619) for a batch, waveforms only.
    clean_spec_mag_norm_log, pred_spec_mag [B,1,F,T]; pc_directions_mag [B,K,F,T]; clean_spec [B,2,F,T]; alphas [A];
    mean, std: the batch-global statistics of preprocess_data(..., plot_mean_std=True), device scalars (read on the
    device, no host synchronisation)  ->  (variations [B,K,A,L], clean_audio [B,L]) fp32:
        variations[b,k,a] = istft(exp((pred[b] + alphas[a] * pc[b,k]) * std + mean) * exp(i angle(clean[b])))
        clean_audio[b]    = istft((exp(clean_norm[b] * std + mean) - 1e-6) * exp(i angle(clean[b])))
    As in the reference the variations do not subtract the 1e-6 the clean path subtracts, and angle(0) = 0.
    L = `length`, default torch.istft's own (hop (T - 1), + 1 for odd n_fft)."""
    H.require_gpu()
    f32 = lambda t: t.contiguous().float()
    pred, pc, cn, cs = f32(pred_spec_mag), f32(pc_directions_mag), f32(clean_spec_mag_norm_log), f32(clean_spec)
    B, K, F, T = pc.shape
    if F != n_fft // 2 + 1:
        raise ValueError(f"{F} frequency bins do not fit n_fft {n_fft}")
    if pred.shape != (B, 1, F, T) or cn.shape != (B, 1, F, T) or cs.shape != (B, 2, F, T):
        raise ValueError(f"shapes {tuple(pred.shape)}, {tuple(cn.shape)}, {tuple(cs.shape)} do not fit directions {tuple(pc.shape)}")
    dev = pc.device
    alphas = torch.as_tensor(alphas, dtype=torch.float32).to(dev).contiguous().reshape(-1)
    A = alphas.numel()
    if A == 0:
        raise ValueError("no alphas given")
    L = ops.check_istft_any_config(n_fft, hop_length, T, length)
    as_scalar = lambda v: torch.as_tensor(v, dtype=torch.float32).to(dev).reshape(1).contiguous()
    out = torch.empty(B, K, A, L, dtype=torch.float32, device=dev)
    clean_wave = torch.empty(B, L, dtype=torch.float32, device=dev)
    with ops.envelope_refusal(n_fft, hop_length, T, L):
        H.call("nppc_pc_variation_waves", pred, pc, cn, cs, as_scalar(mean), as_scalar(std), alphas, out, clean_wave, B, K, A,
               T, n_fft, hop_length, L, H.stream())
    return out, clean_wave


def save_pc_audio_variations(out, save_dir, alphas, first_index=0, fmt="flac", sample_rate=16000, backend="auto",
                             flac_predictor="fixed"):
    """save_pc_audio_variations (:579-634), the audio files, for a whole batch: from validate_batch's dict (called with
    `alphas`) writes, for sample b of the batch, under <save_dir>/sample_<first_index + b>/
        clean.<ext>                            'clean_audio'[b]
        pc_<k+1>/alpha_<a:.1f>.<ext>           'audio_variations'[b, k, a]
        pc_<k+1>/alpha_<a:.1f>_blind.<ext>     'audio_variations_blind'[b, k, a], when the dict holds them
    16-bit mono at sample_rate.  fmt "flac": all B (1 + K A [+ K A]) waveforms are quantised and encoded in ONE device call
    (flac.encode_waves) and cross to the host as FLAC bytes; fmt "wav": the same samples as wav.  The reference's *_full
    files (the variation spliced into the source recording) are RecordingRestorer.save_variations, the spectrogram pictures
    save_pc_spectrograms, the pitch figures save_pc_pitch_plots; transcriptions and phonemes are outside this build.
    flac_predictor: the FLAC encoder's predictor, "fixed" or "lpc" (flac.encode_pcm).  -> the paths written"""
    from ... import flac as FL
    var, clean = out["audio_variations"], out["clean_audio"]
    B, K, A, L = var.shape
    alphas = [float(a) for a in torch.as_tensor(alphas).reshape(-1).tolist()]
    if len(alphas) != A:
        raise ValueError(f"{len(alphas)} alphas for {A} variations per direction")
    blind = out.get("audio_variations_blind")
    root = Path(save_dir)
    paths, waves = [], [clean.reshape(B, L), var.reshape(B * K * A, L)]
    paths += [root / f"sample_{first_index + b}" / f"clean.{fmt}" for b in range(B)]
    paths += [root / f"sample_{first_index + b}" / f"pc_{k + 1}" / f"alpha_{a:.1f}.{fmt}"
              for b in range(B) for k in range(K) for a in alphas]
    if blind is not None:
        if blind.shape != var.shape:
            raise ValueError(f"blind variations {tuple(blind.shape)} do not fit {tuple(var.shape)}")
        waves.append(blind.reshape(B * K * A, L))
        paths += [root / f"sample_{first_index + b}" / f"pc_{k + 1}" / f"alpha_{a:.1f}_blind.{fmt}"
                  for b in range(B) for k in range(K) for a in alphas]
    FL.write_waves(paths, torch.cat([w.float() for w in waves]), sample_rate, fmt, backend=backend, predictor=flac_predictor)
    return paths


SPEC_RANGE, SPEC_ERROR_RANGE = (-3.0, 3.0), (0.0, 3.0)               # plot_pc_spectrograms :292-293


def pc_spectrogram_sheets(B, K, alphas, individual=True, sx=2, sy=2, gutter=4):
    """the panels of plot_pc_spectrograms over the planes (clean, masked, output, pc_1 .. pc_K) of every item:
    -> (names, sheets), names[i] the file of sheets[i] below the sample's spectrograms directory, item by item.  Every
    individual panel carries the gap markers, as save_individual_spectrogram draws them; on the sheet the first four panels
    of row 0 do not, as in the reference's figure."""
    from ...spectrogram_png import Cell, Sheet
    CLEAN, MASKED, OUT, PC = 0, 1, 2, 3
    rng = dict(vmin=SPEC_RANGE[0], vmax=SPEC_RANGE[1])
    err = dict(p=CLEAN, q=OUT, alpha=-1.0, g="abs", vmin=SPEC_ERROR_RANGE[0], vmax=SPEC_ERROR_RANGE[1])
    names, sheets = [], []
    for b in range(B):
        if individual:
            panels = [("clean_spec.png", Cell(p=CLEAN, markers=True, **rng)), ("masked_spec.png", Cell(p=MASKED, markers=True, **rng)),
                      ("output_spec.png", Cell(p=OUT, markers=True, **rng)), ("error_spec.png", Cell(markers=True, **err))]
            for k in range(K):
                panels.append((f"pc_direction_{k + 1}.png", Cell(q=PC + k, markers=True, **rng)))
                panels += [(f"pc{k + 1}_alpha_{a:.1f}.png", Cell(p=OUT, q=PC + k, alpha=a, markers=True, **rng)) for a in alphas]
            for name, cell in panels:
                names.append((b, name))
                sheets.append(Sheet(b, [[cell]], sx=sx, sy=sy))
        cols = max(len(alphas) + 1, 6)
        top = [Cell(p=CLEAN, **rng), Cell(p=MASKED, **rng), Cell(p=OUT, **rng), Cell(**err), Cell(p=CLEAN, markers=True, **rng),
               Cell(p=OUT, markers=True, **rng)] + [None] * (cols - 6)
        rows = [top]
        for k in range(K):
            row = [Cell(q=PC + k, markers=True, **rng)] + [Cell(p=OUT, q=PC + k, alpha=a, markers=True, **rng) for a in alphas]
            rows.append(row + [None] * (cols - len(row)))
        names.append((b, "sheet.png"))
        sheets.append(Sheet(b, rows, sx=sx, sy=sy, gutter=gutter))
    return names, sheets


def save_pc_spectrograms(out, save_dir, alphas, first_index=0, max_dirs=None, individual=True, sx=2, sy=2, gutter=4,
                         palette="viridis", max_frames=None):
    """plot_pc_spectrograms (:273-478) for a whole batch, from the dict of validate_batch(..., spectrograms=True): under
    <save_dir>/sample_<first_index + b>/spectrograms/ the reference's files
        clean_spec.png, masked_spec.png, output_spec.png, error_spec.png            |clean - output| in [0, 3]
        pc_direction_<k>.png, pc<k>_alpha_<a:.1f>.png                               output + a * direction k, in [-3, 3]
    (individual=True) and one sheet.png: row 0 clean, masked, output, error, clean, output (the last two with the gap
    markers), row k direction k and its variations.  Every panel shows the reference's context window (:296-302): the gap
    widened by its own length on each side, found on the device from the mask, so widths differ within a batch; an item
    without a gap shows the whole clip.  Every source pixel is sx x sy pixels; the dashed columns in the marker colour stand
    at the gap's first frame and at the one past its last.  The whole batch, B (4 + K (1 + A) + 1) files, is drawn and
    encoded in ONE device call (spectrogram_png.render_png).  max_frames: the widest window there can be (default T), which
    sizes the workspace.  -> the paths written"""
    from ... import png as PNG
    from ...spectrogram_png import render_png, windows_from_mask
    H.require_gpu()
    pc, pred, clean, mask4 = out["pc_directions"], out["pred_spec_mag_norm"], out["clean_spec_mag_norm"], out["mask"]
    if "masked_spec_mag_norm" not in out:
        raise ValueError("save_pc_spectrograms takes the dict of validate_batch(..., spectrograms=True), which holds "
                         "'masked_spec_mag_norm'")
    masked = out["masked_spec_mag_norm"]
    B, K, F, T = pc.shape
    if max_dirs is not None:
        K = min(K, int(max_dirs))
    alphas = [float(a) for a in torch.as_tensor(alphas).reshape(-1).tolist()]
    if not alphas:
        raise ValueError("no alphas given")
    f32 = lambda t: t.detach().float().reshape(B, -1, F, T)
    planes = torch.cat([f32(clean), f32(masked), f32(pred), f32(pc)[:, :K]], dim=1).contiguous()
    win = windows_from_mask(mask4.detach().float().reshape(B, -1, F, T)[:, 0, 0, :])
    names, sheets = pc_spectrogram_sheets(B, K, alphas, individual, sx, sy, gutter)
    files = render_png(planes, sheets, win, palette=palette, max_frames=max_frames)
    root = Path(save_dir)
    paths = [root / f"sample_{first_index + b}" / "spectrograms" / name for b, name in names]
    PNG.write_files(paths, files)
    return paths


def posterior_std_planes(out):
    """the plane save_posterior_samples draws, [B,1,2,F,T] complex (imaginary part 0): 'mag_std' on the gap frames and NaN
    on the known ones, where the directions are zero and the spread with them, so a cell's autoscale sees the gap alone"""
    sd, mask4 = out["posterior"]["mag_std"], out["mask"]
    B, F, T = sd.shape
    gap = mask4.detach().float().reshape(B, -1, F, T)[:, 0] == 0
    re = torch.where(gap, sd.detach().float(), torch.full_like(sd, float("nan")))
    return torch.stack([re, torch.zeros_like(re)], 1)[:, None].contiguous()


def save_posterior_samples(out, save_dir, first_index=0, fmt="flac", sample_rate=16000, backend="auto", sx=2, sy=2,
                           palette="viridis", max_frames=None, flac_predictor="fixed"):
    """from the dict of validate_batch(..., posterior_samples=S) writes, for sample b of the batch, under
    <save_dir>/sample_<first_index + b>/posterior/
        sample_<s>.<ext>          'posterior'['samples'][b, s] (and sample_<s>_blind.<ext> when the dict holds 'samples_blind'),
                                  16-bit mono: fmt "flac" encodes all of them in one device call (flac.write_waves), "wav" writes
                                  the same samples
        std_spec.png              'posterior'['mag_std'][b] in dB (20 log10(std + 1e-8), autoscaled over the gap) over the
                                  reference's context window with the gap markers (spectrogram_png: one Sheet per item, all
                                  drawn and encoded in one device call); known frames, where the spread is zero, take index 0
    flac_predictor: the FLAC encoder's predictor, "fixed" or "lpc" (flac.encode_pcm).  -> the paths written"""
    from ... import flac as FL
    from ... import png as PNG
    from ...spectrogram_png import Cell, Sheet, render_png, windows_from_mask
    if "posterior" not in out:
        raise ValueError("save_posterior_samples takes the dict of validate_batch(..., posterior_samples=S), which holds 'posterior'")
    post = out["posterior"]
    smp = post["samples"]
    B, S, L = smp.shape
    root = Path(save_dir)
    folder = lambda b: root / f"sample_{first_index + b}" / "posterior"
    paths, waves = [folder(b) / f"sample_{s}.{fmt}" for b in range(B) for s in range(S)], [smp.reshape(B * S, L)]
    if "samples_blind" in post:
        paths += [folder(b) / f"sample_{s}_blind.{fmt}" for b in range(B) for s in range(S)]
        waves.append(post["samples_blind"].reshape(B * S, L))
    FL.write_waves(paths, torch.cat([w.float() for w in waves]), sample_rate, fmt, backend=backend, predictor=flac_predictor)
    planes = posterior_std_planes(out)
    F, T = planes.shape[-2:]
    win = windows_from_mask(out["mask"].detach().float().reshape(B, -1, F, T)[:, 0, 0, :])
    sheets = [Sheet(b, [[Cell(p=0, g="db", markers=True)]], sx=sx, sy=sy) for b in range(B)]
    pngs = [folder(b) / "std_spec.png" for b in range(B)]
    PNG.write_files(pngs, render_png(planes, sheets, win, palette=palette, max_frames=max_frames))
    return paths + pngs


PITCH_RANGE, PITCH_SR, PITCH_HOP = (80.0, 400.0), 16000, 512          # validate_batch's pYIN setting (plot_pitch_comparison :60-66)


def pitch_windows(mask, stft_hop, n_pitch_frames, pitch_hop=PITCH_HOP):
    """mask [B, T] (device, 0 inside the gap) -> int32 [B, 4] in pitch frames: the whole clip [0, n_pitch_frames) and the gap
    markers.  Integer arithmetic on the device: STFT frame f is centred on sample f * stft_hop and pitch frame j on sample
    j * pitch_hop, so frame f becomes the nearest pitch frame (f * stft_hop + pitch_hop // 2) // pitch_hop; the markers are
    the gap's first STFT frame and the one past its last (spectrogram_png.windows_from_mask); an item without a gap has
    none (-1)."""
    from ...spectrogram_png import windows_from_mask
    m = windows_from_mask(mask)[:, 2:4].long()
    conv = torch.where(m >= 0, (m * int(stft_hop) + pitch_hop // 2) // pitch_hop, torch.full_like(m, -1))
    whole = torch.tensor([0, int(n_pitch_frames)], dtype=torch.long, device=m.device).expand(m.shape[0], 2)
    return torch.cat([whole, conv], dim=1).to(torch.int32).contiguous()


def save_pc_pitch_plots(out, save_dir, alphas, first_index=0, max_dirs=None, individual=True, sx=8, plot_height=240,
                        backend="auto", hop_length=None):
    """plot_pitch_comparison (:19-154) for a whole batch, from the dict of validate_batch(..., pitch=True): under
    <save_dir>/sample_<first_index + b>/
        pitch_contours/pc_<k>_pitch.png     the clean contour (black, 2 pixels) under direction k's A variations in viridis
                                            colours (curve_png.alpha_colours), a legend of every second alpha   (individual)
        pitch_comparison.png                the clean panel and one such panel per direction, stacked
    y runs over the call's 80..400 Hz with a grid line and a label every 100 Hz; x is the whole clip, every pitch frame sx
    pixels wide, with a grid line and a label in seconds every 16 frames (0.512 s: the whole number of 32 ms frames nearest
    to half a second).  The dashed columns stand at the gap's first frame and the one past its last, converted from
    out['mask'] on the device (pitch_windows; hop_length: the STFT's hop, default L // (T - 1)).  The whole batch,
    B (K + 1) files, is drawn and encoded in ONE curve_png.render_png call and written by one png.write_files.
    -> the paths written"""
    from ... import curve_png as CP
    from ... import png as PNG
    if "pitch" not in out:
        raise ValueError("save_pc_pitch_plots takes the dict of validate_batch(..., pitch=True), which holds 'pitch'")
    pitch = out["pitch"]
    B, K, A, T = pitch["f0"].shape
    alphas = [float(a) for a in torch.as_tensor(alphas).reshape(-1).tolist()]
    if len(alphas) != A:
        raise ValueError(f"{len(alphas)} alphas for {A} variations per direction")
    if max_dirs is not None:
        K = min(K, int(max_dirs))
    mask = out["mask"].detach().float()
    mask = mask.reshape(B, -1, mask.shape[-2], mask.shape[-1])[:, 0, 0, :]
    L = out["clean_audio"].shape[-1]
    hop = int(hop_length) if hop_length is not None else L // max(1, mask.shape[-1] - 1)
    values = CP.stack_contours(pitch)
    win = pitch_windows(mask.to(values.device), hop, T)
    names, sheets = CP.pitch_sheets(B, K, alphas, T, PITCH_HOP / PITCH_SR, individual=individual, sx=sx, plot_height=plot_height,
                                    fmin=PITCH_RANGE[0], fmax=PITCH_RANGE[1], per_item=1 + pitch["f0"].shape[1] * A)
    files = CP.render_png(values, sheets, win, backend=backend)
    root = Path(save_dir)
    paths = [root / f"sample_{first_index + b}" / ("pitch_contours" if name != "pitch_comparison.png" else "") / name
             for b, name in names]
    PNG.write_files(paths, files)
    return paths


def save_metrics_to_json(metrics, save_dir, sample_idx):
    """:831-859: <save_dir>/validation_metrics/sample_<idx>.json, {'nppc': {...}, 'mc_dropout': {...},
    'principal_angles': [...]}"""
    json_metrics = {}
    for method, values in metrics.items():
        if method == 'principal_angles':
            json_metrics[method] = [float(angle) for angle in values]
        else:
            json_metrics[method] = {k: float(v) if isinstance(v, (torch.Tensor, np.ndarray)) else v for k, v in values.items()}
    metrics_dir = Path(save_dir) / "validation_metrics"
    metrics_dir.mkdir(parents=True, exist_ok=True)
    with open(metrics_dir / f"sample_{sample_idx}.json", 'w') as f:
        json.dump(json_metrics, f, indent=4)


class NPPCModelValidatorConfig(pydantic.BaseModel):
    checkpoint_path: str
    device: str = "cuda"
    save_dir: Optional[str] = "validation_nppc_results"
    model_configuration: NPPCModelConfig
    max_dirs_to_plot: Optional[int] = None


class NPPCModelValidator:
    """Loads a checkpoint written by NPPCAudioInpaintingTrainer.save_checkpoint ({'model_state_dict': ...}) and scores it
    on held-out batches.

    The MC-dropout baseline gathers the gap elements of every item into one [K, B, N_masked] stack, so by default every
    item of a batch must have the same number of gap (mask == 0) elements; it raises ValueError otherwise.
    `ragged_gaps=True` (validate_batch, validate_dataloader) lifts that: the stack is padded to the largest gap of the
    batch (mc_baseline.calculate_unet_baseline_ragged), which is what batches of the reference's dataset need (its
    2048-sample gap covers 17 or 18 frames depending on where it starts).  Everything downstream of the baseline works
    per item through the mask and is the same in both modes."""

    def __init__(self, config: NPPCModelValidatorConfig):
        self.config = config
        self.device = config.device
        if config.device == 'cuda':
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        checkpoint = torch.load(Path(config.checkpoint_path).absolute(), map_location="cpu")
        self.model = NPPCModel(config.model_configuration)
        self.model.load_state_dict(checkpoint["model_state_dict"])
        self.model.to(self.device)
        self.model.eval()

    def _run_batch(self, masked_spec, mask, clean_spec, n_mc_samples, n_components, ragged_gaps=False):
        """every device stage of one batch; the Gram matrices stay on the device"""
        H.require_gpu()
        self.model.eval()
        with torch.no_grad():
            masked_spec, mask, clean_spec = (t.to(self.device) for t in (masked_spec, mask, clean_spec))
            clean_norm, mask4, masked_norm, mean, std = preprocess_data(clean_spec, masked_spec, mask, plot_mean_std=True)
            mask4 = mask4.contiguous()
            pc_directions = self.model(masked_norm, mask4)
            pred = self.model.get_pred_spec_mag_norm(masked_norm, mask4)
            if n_components != pc_directions.shape[1]:
                raise ValueError(f"n_components = {n_components} but the model has {pc_directions.shape[1]} directions: "
                                 "the metrics compare subspaces of the same dimension")
            restorer = self.model.pretrained_restoration_model
            baseline = MB.calculate_unet_baseline_ragged if ragged_gaps else MB.calculate_unet_baseline
            try:
                mc = baseline(restorer, masked_norm, mask4, n_mc_samples=n_mc_samples, n_components=n_components)
            finally:
                restorer.eval()                                     # enable_dropout left the Dropout modules in train mode
            gram = MB.metrics_gram_batch(pc_directions, mc['scaled_principal_components'], pred, mc['mean_prediction'],
                                         clean_norm, mask4)
        return {'pc_directions': pc_directions, 'pred_spec_mag_norm': pred, 'clean_spec_mag_norm': clean_norm,
                'mask': mask4, 'mean': mean, 'std': std, 'mc_dropout': mc, 'gram': gram, 'clean_spec': clean_spec,
                'masked_spec_mag_norm': masked_norm}

    def validate_batch(self, masked_spec, mask, clean_spec, n_mc_samples=50, n_components=5, alphas=None, n_fft=255,
                       hop_length=128, pitch=False, phase="clean", gl_iters=32, ragged_gaps=False, long_spans=False,
                       spectrograms=False, posterior_samples=None, posterior_seed=None):
        """validate_sample + _validate_with_baseline (:930-1027) for a uniform batch: masked_spec, clean_spec [B,2,F,T],
        mask [B,T] (1 = known; the same number of gap frames in every item) -> dict with 'pc_directions' [B,K,F,T],
        'pred_spec_mag_norm', 'clean_spec_mag_norm', 'mask' [B,1,F,T], 'mean', 'std', 'mc_dropout' (calculate_unet_baseline's
        dict), 'metrics' (list of B compute_metrics dicts) and, when `alphas` is given, 'audio_variations' [B,K,A,L] and
        'clean_audio' [B,L] (pc_audio_variations).

        pitch=True (needs `alphas`; ValueError otherwise) adds 'pitch': pYIN contours at the reference's setting (fmin 80,
        fmax 400, sr 16000; plot_pitch_comparison :60-66) of the clean waveform and of every variation, from one batched
        call: {'f0_clean' [B,T'], 'voiced_flag_clean', 'voiced_prob_clean', 'f0' [B,K,A,T'], 'voiced_flag', 'voiced_prob',
        'summary' (pitch.pitch_variation_summary, [B,K,A] tensors)}, T' = 1 + L // 512.  Everything else is unchanged.

        phase="griffin_lim" (needs `alphas`; ValueError otherwise) adds 'audio_variations_blind' [B,K,A,L],
        'restored_audio_blind' [B,L] and 'phase_info' (phase.pc_audio_variations_blind: `gl_iters` iterations of
        gap-constrained Griffin-Lim from the damaged recording's STFT, no clean phase).  The default phase="clean" returns
        exactly what it returned before; pitch tracking keeps using the clean-phase waveforms.  `long_spans` is passed to
        pc_audio_variations_blind: True lets gaps over Griffin-Lim's resident span cap through (the reference yaml's 0.256 s
        gap is 33 frames at 255 / 128), the default flags them with status 1 and NaN.

        ragged_gaps=True accepts items with different numbers of gap frames (every item needs at least one); the keys
        and shapes are the same.  The default keeps raising ValueError for such a batch.

        spectrograms=True adds 'masked_spec_mag_norm' [B,1,F,T], the normalised masked input, which save_pc_spectrograms
        draws beside the clean and the restored spectrogram; the default returns the keys it always returned.

        posterior_samples=S (2 <= S <= 4096) adds 'posterior' (inpainting.posterior): 'coeffs' [B,S,K]
        drawn by draw_coefficients(seed=posterior_seed), 'samples' [B,S,L] on the clean phase, their per-sample 'std' [B,L]
        and the spread 'mag_std' [B,F,T] of the linear magnitudes; with phase="griffin_lim" (which then does not need
        `alphas`) also 'samples_blind' [B,S,L] from the damaged recording's STFT and their 'phase_info'.  Without it the call
        returns exactly the keys it returned before."""
        S_post = None
        if posterior_samples is not None:
            S_post = int(posterior_samples)
            if isinstance(posterior_samples, bool) or S_post != posterior_samples or not 2 <= S_post <= 4096:
                raise ValueError(f"posterior_samples = {posterior_samples!r}: 2 .. 4096 samples (their spread is part of the result)")
        if phase not in ("clean", "griffin_lim"):
            raise ValueError(f"phase = {phase!r}: 'clean' or 'griffin_lim'")
        if pitch and alphas is None:
            raise ValueError("pitch=True tracks the f0 of the PC audio variations: pass `alphas` (e.g. default_alphas())")
        if phase == "griffin_lim" and alphas is None and S_post is None:
            raise ValueError("phase='griffin_lim' synthesises the PC audio variations: pass `alphas` (e.g. default_alphas())")
        masked_dev = masked_spec.to(self.device) if phase == "griffin_lim" else None
        out = self._run_batch(masked_spec, mask, clean_spec, n_mc_samples, n_components, ragged_gaps)
        out['metrics'] = MB.metrics_from_gram(out.pop('gram').cpu().numpy(), n_components)
        clean_spec = out.pop('clean_spec')
        if not spectrograms:
            out.pop('masked_spec_mag_norm')
        if alphas is not None:
            with torch.no_grad():
                out['audio_variations'], out['clean_audio'] = pc_audio_variations(
                    out['clean_spec_mag_norm'], out['pred_spec_mag_norm'], out['pc_directions'], clean_spec, alphas,
                    out['mean'], out['std'], n_fft=n_fft, hop_length=hop_length)
                if pitch:
                    out['pitch'] = PT.contours_of_variations(out['clean_audio'], out['audio_variations'],
                                                             **PT.REFERENCE_SETTING)
                if phase == "griffin_lim":
                    out['audio_variations_blind'], out['restored_audio_blind'], out['phase_info'] = \
                        PH.pc_audio_variations_blind(out['pred_spec_mag_norm'], out['pc_directions'], masked_dev, out['mask'],
                                                     alphas, out['mean'], out['std'], n_iter=gl_iters, n_fft=n_fft,
                                                     hop_length=hop_length, long_spans=long_spans)
        if S_post is not None:
            from .. import posterior as IPOST
            with torch.no_grad():
                pc = out['pc_directions']
                z = IPOST.draw_coefficients(pc.shape[0], S_post, pc.shape[1], seed=posterior_seed, device=pc.device)
                r = IPOST.sample_waveforms(out['pred_spec_mag_norm'], pc, clean_spec, z, out['mean'], out['std'], n_fft=n_fft,
                                           hop_length=hop_length, stats=True, spec_stats=True)
                out['posterior'] = {'coeffs': z, 'samples': r['samples'], 'std': r['std'], 'mag_std': r['mag_std']}
                if phase == "griffin_lim":
                    blind, _, info = IPOST.sample_waveforms_blind(out['pred_spec_mag_norm'], pc, masked_dev, out['mask'], z,
                                                                  out['mean'], out['std'], n_iter=gl_iters, n_fft=n_fft,
                                                                  hop_length=hop_length, long_spans=long_spans)
                    out['posterior'].update(samples_blind=blind, phase_info=info)
        return out

    def validate_dataloader(self, dataloader, n_mc_samples=50, n_components=5, save=False, ragged_gaps=False,
                            spectrogram_alphas=None):
        """every item of every batch ((masked_spec, mask, clean_spec) or utils.collate_fn's five-tuple): the Gram
        matrices stay on the device until the loader is exhausted, then ONE copy to the host and the n x n algebra.
        -> {'per_item': [compute_metrics dicts], 'mean': {'nppc': {...}, 'mc_dropout': {...}, 'principal_angles': [...]},
            'n_items': int}; save=True also writes validation_metrics/sample_<i>.json under config.save_dir.
        ragged_gaps=True: batches whose items have different numbers of gap frames (one host read of the gap counts per
        batch on top of the one copy per loader).  With save=True and `spectrogram_alphas` (e.g. default_alphas()) every
        batch's spectrogram panels and sheets are written too (save_pc_spectrograms, config.max_dirs_to_plot directions)."""
        grams, seen = [], 0
        for batch in dataloader:
            out = self._run_batch(*batch[:3], n_mc_samples, n_components, ragged_gaps)
            grams.append(out['gram'])
            if save and spectrogram_alphas is not None and self.config.save_dir is not None:
                save_pc_spectrograms(out, self.config.save_dir, spectrogram_alphas, first_index=seen,
                                     max_dirs=self.config.max_dirs_to_plot)
            seen += out['gram'].shape[0]
        if not grams:
            raise ValueError("the dataloader yielded no batches")
        per_item = MB.metrics_from_gram(torch.cat(grams).cpu().numpy(), n_components)
        mean = {m: {k: float(np.mean([it[m][k] for it in per_item])) for k in ('rmse', 'residual_error')}
                for m in ('nppc', 'mc_dropout')}
        n_ang = min(len(it['principal_angles']) for it in per_item)
        mean['principal_angles'] = [float(np.mean([it['principal_angles'][j] for it in per_item])) for j in range(n_ang)]
        if save and self.config.save_dir is not None:
            for i, it in enumerate(per_item):
                save_metrics_to_json(it, self.config.save_dir, i)
        return {'per_item': per_item, 'mean': mean, 'n_items': len(per_item)}
