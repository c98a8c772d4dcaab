"""Restore a whole damaged recording: window, inpaint, splice, on the device (csrc/restore_rec.hip, DESIGN.md section 8f;
specification tests/restore_ref.py).

Every other entry point of the inpainting side takes crops [B, 2, F, T] with one gap each, already cut, gain-normalised,
masked and transformed by the dataset.  `RecordingRestorer.restore` takes the recording itself and the list of its gaps:

    gain -> windows -> frame mask -> STFT -> preprocess_data -> restorer (and direction net) -> gap-constrained Griffin-Lim
    -> splice

and returns the restored recording and, when `alphas` is given, the K x A recordings (or windows) along the principal
directions.  The reference only hints at this step (get_with_full_audio, validator_nppc_model.py:518-526).

Normalisation rules
  * ONE gain for the whole recording: the dataset's _normalize_audio (dataset/audio_dataset_inpainting.py:154-168, the same
    1e-8), with the RMS taken over the samples OUTSIDE the gaps only (the gaps are zeros and would bias it), in fp64.
    The output is divided by the gain again.
  * The log-magnitude mean / std are `utils.preprocess_data`'s: scalars over the batch of all windows of ONE call, taken
    from the damaged windows' STFT (there is no clean one).  So a gap restored together with other gaps is not bit-equal
    to the same gap restored alone.
  * Samples outside every [s - crossfade, e + crossfade) are the input's, bit for bit: they never pass through the gain.
    A recording at another rate than the model's keeps this rule at ITS rate: restore(..., sample_rate=44100) resamples
    down (nppc_audio.resample), restores, resamples up and splices there; inside the gaps nothing above the model's
    Nyquist frequency is synthesised.

Policy (`plan_windows`, pure Python): gaps are sorted; two gaps closer than 2 x crossfade_samples are merged into their hull
(the few known samples between them are synthesised too); every merged gap gets one window of `window_samples` centred on it
and clamped to the recording, and is written back from that window alone; other gaps inside a window are masked there.
"""
import math
from typing import Optional

import pydantic
import torch

from .. import _hip as H
from . import phase as PH
from .nppc.nppc_model import NPPCModel, NPPCModelConfig

__all__ = ["RecordingRestorerConfig", "RecordingRestorer", "plan_windows", "native_crossfade", "merge_native_gaps",
           "REC_GAIN_WORK", "ZERO_RUN_CHUNK"]

REC_GAIN_WORK = 256          # NPPC_REC_GAIN_WORK
ZERO_RUN_CHUNK = 4096        # NPPC_ZERO_RUN_CHUNK


class RecordingRestorerConfig(pydantic.BaseModel):
    checkpoint_path: str                       # NPPCAudioInpaintingTrainer.save_checkpoint's file (NPPCModelValidator's)
    model_configuration: NPPCModelConfig
    device: str = "cuda"
    sample_rate: int = 16000                   # restore_file decodes to it and writes it
    window_samples: int = 32704                # the reference yaml's 2.044 s
    n_fft: int = 255
    hop_length: int = 128
    target_dB_FS: float = -25.0
    gl_iters: int = 32
    momentum: float = 0.0
    crossfade_samples: int = 64
    min_gap_samples: int = 160                 # detect_gaps: shorter runs of zeros are signal
    long_gaps: bool = False                    # gaps over Griffin-Lim's resident span cap run its tiled path (long_spans)


def _frame_range(a, b, n_fft, hop, T):
    """frames of a centred STFT whose window [t hop - n_fft // 2, + n_fft) meets the samples [a, b): (lo, hi) inclusive,
    clipped to [0, T - 1]; hi < lo when none does"""
    half = n_fft // 2
    lo = (a - n_fft + half) // hop + 1                 # smallest t with t hop - half + n_fft > a
    hi = -((-(b + half)) // hop) - 1                   # largest t with t hop - half < b
    return max(lo, 0), min(hi, T - 1)


def plan_windows(length, gaps, window_samples=32704, crossfade_samples=64, n_fft=255, hop_length=128, long_gaps=False):
    """The windows that restore `gaps` (half-open sample pairs) of a recording of `length` samples: a list, ascending, of
    {'start': first sample of the window, 'gap': (s, e) the merged gap this window owns and writes back,
     'masked': [(a, b)] every gap's part inside the window in window coordinates, 'frames': (lo, hi) the bounding range of
     the window's masked frames}.
    ValueError for a pair that is empty, negative or out of range (it names the pair), a recording shorter than the window,
    a gap with fewer than ceil(n_fft / hop) known frames on either side inside its window, a crossfade that leaves the
    window, and a window whose masked frames (+ the 2 (ceil(n_fft / hop) - 1) neighbours Griffin-Lim keeps with them) exceed
    phase.gl_gap_shape(...)['span_cap'].  With long_gaps=True that last refusal is dropped (griffin_lim_gap's long_spans=True
    takes such windows); every other one stays.  No GPU."""
    length, W, xf, hop = int(length), int(window_samples), int(crossfade_samples), int(hop_length)
    if xf < 0 or W <= 0 or hop <= 0 or n_fft < 2:
        raise ValueError(f"window_samples {W}, crossfade_samples {xf}, n_fft {n_fft}, hop_length {hop}: not a configuration")
    pairs = []
    for g in gaps:
        try:
            s, e = (int(v) for v in g)
        except (TypeError, ValueError) as err:
            raise ValueError(f"gap {g!r} is not a (start, end) pair of samples") from err
        if s < 0 or e <= s or e > length:
            raise ValueError(f"gap ({s}, {e}) is empty, negative or outside the recording's {length} samples")
        pairs.append((s, e))
    if not pairs:
        return []
    if length < W:
        raise ValueError(f"the recording has {length} samples, fewer than one window of {W}")
    pairs.sort()
    merged = [pairs[0]]
    for s, e in pairs[1:]:
        if s - merged[-1][1] < 2 * xf:
            merged[-1] = (merged[-1][0], max(merged[-1][1], e))
        else:
            merged.append((s, e))
    T = 1 + W // hop
    sh = PH.gl_gap_shape(1, 1, n_fft // 2 + 1, T, n_fft, hop, length=W, n_iter=0)
    need = -(-n_fft // hop)
    plan = []
    for s, e in merged:
        ws = min(max((s + e) // 2 - W // 2, 0), length - W)
        if s < ws or e > ws + W:
            raise ValueError(f"gap ({s}, {e}) does not fit a window of {W} samples")
        masked = [(max(a, ws) - ws, min(b, ws + W) - ws) for a, b in merged if a < ws + W and b > ws]
        known = [True] * T
        for a, b in masked:
            lo, hi = _frame_range(a, b, n_fft, hop, T)
            for t in range(lo, hi + 1):
                known[t] = False
        lo, hi = _frame_range(s - ws, e - ws, n_fft, hop, T)
        if sum(known[:lo]) < need or sum(known[hi + 1:]) < need:
            raise ValueError(f"gap ({s}, {e}) leaves fewer than {need} known frames on one side inside its window "
                             f"[{ws}, {ws + W}): frames {lo}..{hi} of {T} are masked")
        if (s - xf < ws and ws > 0) or (e + xf > ws + W and ws + W < length):
            raise ValueError(f"the crossfade of {xf} samples around gap ({s}, {e}) leaves its window [{ws}, {ws + W})")
        f_lo, f_hi = known.index(False), T - 1 - known[::-1].index(False)
        if not long_gaps and f_hi - f_lo + 1 + 2 * sh["r"] > sh["span_cap"]:
            raise ValueError(f"the window [{ws}, {ws + W}) of gap ({s}, {e}) masks frames {f_lo}..{f_hi}: with "
                             f"{2 * sh['r']} neighbours that is more than the span cap of {sh['span_cap']} frames "
                             "(a gap too long, or two gaps inside one window)")
        plan.append({"start": ws, "gap": (s, e), "masked": masked, "frames": (f_lo, f_hi)})
    return plan


def native_crossfade(crossfade_samples, rate, model_rate):
    """the crossfade of `crossfade_samples` at model_rate, in samples at `rate`, rounded up"""
    return -(-int(crossfade_samples) * int(rate) // int(model_rate))


def merge_native_gaps(gaps, crossfade):
    """sorted; two gaps closer than 2 x crossfade become their hull (plan_windows' rule, at the recording's own rate), so
    that the regions [s - crossfade, e + crossfade) nppc_rec_splice blends never overlap"""
    pairs = sorted((int(s), int(e)) for s, e in gaps)
    merged = pairs[:1]
    for s, e in pairs[1:]:
        if s - merged[-1][1] < 2 * crossfade:
            merged[-1] = (merged[-1][0], max(merged[-1][1], e))
        else:
            merged.append((s, e))
    return merged


def _upload_plan(plan, device):
    """-> gaps [W, 2] and window starts [W], int64 on the device, one copy"""
    host = torch.tensor([[p["gap"][0], p["gap"][1], p["start"]] for p in plan], dtype=torch.int64)
    dev = host.to(device)
    return dev[:, :2].contiguous(), dev[:, 2].contiguous()


def recording_gain(wave, gaps, target_dB_FS=-25.0):
    """nppc_rec_gain: wave [L] fp32 (device), gaps [G, 2] int64 (device, sorted, disjoint) -> fp64 device scalar [1]"""
    H.require_gpu()
    work = torch.empty(REC_GAIN_WORK, dtype=torch.float64, device=wave.device)
    gain = torch.empty(1, dtype=torch.float64, device=wave.device)
    H.call("nppc_rec_gain", wave, wave.numel(), gaps, gaps.shape[0], float(target_dB_FS), work, gain, H.stream())
    return gain


def gather_windows(wave, gaps, win_start, window_samples, gain):
    """nppc_rec_windows -> (windows [W, window_samples] = wave * gain with zeros inside every gap, sample mask of the same
    shape: 0 inside every gap)"""
    H.require_gpu()
    W = win_start.numel()
    out = torch.empty(W, window_samples, dtype=torch.float32, device=wave.device)
    mask = torch.empty_like(out)
    H.call("nppc_rec_windows", wave, wave.numel(), gaps, gaps.shape[0], win_start, W, window_samples, gain, out, mask,
           H.stream())
    return out, mask


def splice_windows(wave, gaps, win_start, window_out, gain, crossfade_samples=64):
    """nppc_rec_splice: window_out [W, V, window_samples] or [W, window_samples] (V = 1; strided views of one buffer are
    taken as they are) -> [V, L]: the recording with gap w replaced by window w's output / gain and a raised-cosine
    crossfade of `crossfade_samples` on both sides; every other sample is the input's, bit for bit"""
    H.require_gpu()
    if window_out.dim() == 2:
        window_out = window_out[:, None]
    W, V, Lw = window_out.shape
    if W != win_start.numel() or gaps.shape != (W, 2):
        raise ValueError(f"window outputs {tuple(window_out.shape)} do not fit {win_start.numel()} windows")
    if window_out.stride(2) != 1 or window_out.dtype != torch.float32:
        window_out = window_out.float().contiguous()
    out = torch.empty(V, wave.numel(), dtype=torch.float32, device=wave.device)
    H.call("nppc_rec_splice", wave, wave.numel(), gaps, win_start, W, H.c_p(window_out.data_ptr()), window_out.stride(0),
           window_out.stride(1), Lw, V, int(crossfade_samples), gain, out, H.stream())
    return out


def zero_runs(wave, min_len, capacity=1024):
    """nppc_zero_runs: wave [L] fp32 (device) -> (runs [capacity, 2] int64, count [1] int64), device tensors; rows past
    min(count, capacity) are unwritten"""
    H.require_gpu()
    L, min_len = wave.numel(), int(min_len)
    if min_len < 1:
        raise ValueError(f"min_len = {min_len}: a run has at least one sample")
    nchunks = -(-L // ZERO_RUN_CHUNK)
    work = torch.empty(nchunks * (4 + 2 * (ZERO_RUN_CHUNK // (min_len + 1) + 1)), dtype=torch.int64, device=wave.device)
    runs = torch.empty(capacity, 2, dtype=torch.int64, device=wave.device)
    count = torch.empty(1, dtype=torch.int64, device=wave.device)
    H.call("nppc_zero_runs", wave, L, min_len, work, work.numel(), runs, capacity, count, H.stream())
    return runs, count


class RecordingRestorer:
    """Loads the checkpoint NPPCModelValidator loads ({'model_state_dict': ...} of an NPPCModel: restorer and direction net)
    and restores whole recordings with it.  See the module docstring for the normalisation rules."""

    def __init__(self, config: RecordingRestorerConfig):
        from pathlib import Path
        self.config = config
        self.device = config.device
        if config.device == "cuda":
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        checkpoint = torch.load(Path(config.checkpoint_path).absolute(), map_location="cpu")
        self.model = NPPCModel(config.model_configuration)
        self.model.load_state_dict(checkpoint["model_state_dict"])
        self.model.to(self.device)
        self.model.eval()

    def plan(self, length, gaps):
        c = self.config
        return plan_windows(length, gaps, c.window_samples, c.crossfade_samples, c.n_fft, c.hop_length, c.long_gaps)

    def _check_samples(self, samples, coeffs, n_windows):
        """the refusals of restore(samples=, coeffs=), from the plan and the configuration alone -> S, or None when no
        samples are asked for"""
        if samples is None and coeffs is None:
            return None
        K = int(self.config.model_configuration.audio_pc_wrapper_configuration.n_dirs)
        if coeffs is not None:
            from .posterior import as_coefficients
            z = as_coefficients(coeffs)
            if z.shape[0] != n_windows or z.shape[2] != K or z.shape[1] < 1 or (samples is not None and z.shape[1] != int(samples)):
                raise ValueError(f"coeffs {tuple(z.shape)}: one draw per window and sample, [W, S, K] = [{n_windows}, "
                                 f"{'S' if samples is None else int(samples)}, {K}]")
            return int(z.shape[1])
        if isinstance(samples, bool) or int(samples) != samples or int(samples) < 1:
            raise ValueError(f"samples = {samples!r}: a positive number of posterior samples")
        return int(samples)

    def restore(self, wave, gaps, alphas=None, variations="windows", sample_rate=None, samples=None, seed=None, coeffs=None):
        """wave [L] float (host or device), gaps [(start, end)] half-open sample pairs -> dict:
          'restored' [L]; 'windows' (plan_windows' list); 'gain' (fp64 device scalar [1]); 'inconsistency' [W, V, gl_iters],
          'target_norm' [W, V], 'status' [W] as phase.griffin_lim_gap reports them, per window (V = 1, or K A + 1 with the
          prediction last);
          with `alphas` [A] and variations='windows': 'variation_windows' [W, K, A, window_samples], divided by the gain,
          ready to be written as wav; with variations='full': 'variations' [K, A, L], the recording with every gap replaced
          by that variation.
        With no gaps the input comes back as it is (the same tensor) and nothing is launched.  One host read per call: the
        status check at the end.
        sample_rate: None or config.sample_rate runs exactly the above.  Another rate: `wave` and `gaps` are at that rate
        and so are 'restored' and 'variations' (see _restore_native); 'variation_windows' stay at the model's rate.
        samples=S (or coeffs [W, S, K], real) adds S posterior samples of every gap (inpainting.posterior, DESIGN.md
        section 8n): 'coeffs' [W, S, K], drawn by posterior.draw_coefficients(W, S, K, seed=seed) -- one independent draw
        per window; plan_windows keeps the gaps apart (each is written back from its own window alone), so no alignment
        of the directions across windows is needed -- run through posterior.sample_waveforms_blind on the windows:
        'sample_windows' [W, S, window_samples], divided by the gain, and with variations='full' 'samples' [S, L], in
        which sample s of the recording takes sample s of every window ('samples' at `sample_rate`, 'sample_windows' at
        the model's rate, as the variations).  'restored' and every other key are what they are without `samples`;
        `samples` together with `alphas` returns both.  'sample_status' [W] is the samples' own Griffin-Lim status."""
        if variations not in ("windows", "full"):
            raise ValueError(f"variations = {variations!r}: 'windows' or 'full'")
        if wave.dim() != 1:
            raise ValueError(f"wave {tuple(wave.shape)}: want one channel, [L]")
        c = self.config
        if sample_rate is not None and int(sample_rate) != int(c.sample_rate):
            return self._restore_native(wave, gaps, alphas, variations, int(sample_rate), samples, seed, coeffs)
        plan = self.plan(wave.numel(), gaps)
        S = self._check_samples(samples, coeffs, len(plan))
        if not plan:
            none = {} if S is None else {"coeffs": None, "sample_windows": None}
            return {"restored": wave, "windows": [], "gain": None, "inconsistency": None, "target_norm": None, "status": None,
                    **none}
        H.require_gpu()
        from .data import time_to_spec_mask
        from .utils import preprocess_data
        x = wave.to(self.device).float().contiguous()
        gaps_d, starts_d = _upload_plan(plan, x.device)
        W, Lw, F, T = len(plan), c.window_samples, c.n_fft // 2 + 1, 1 + c.window_samples // c.hop_length
        self.model.eval()
        with torch.no_grad():
            gain = recording_gain(x, gaps_d, c.target_dB_FS)
            xw, mask_t = gather_windows(x, gaps_d, starts_d, Lw, gain)
            mask_f = time_to_spec_mask(mask_t, T, Lw, c.n_fft, c.hop_length, True)
            spec = torch.empty(W, 2, F, T, dtype=torch.float32, device=x.device)
            masked = torch.empty_like(spec)
            H.call("nppc_stft_pair", xw, mask_f, spec, masked, W, Lw, c.n_fft, c.hop_length, H.stream())
            _, mask4, masked_norm, mean, std = preprocess_data(masked, masked, mask_f, plot_mean_std=True)
            mask4 = mask4.contiguous()
            kw = dict(n_iter=c.gl_iters, momentum=c.momentum, n_fft=c.n_fft, hop_length=c.hop_length, length=Lw)
            if c.long_gaps:
                kw["long_spans"] = True
            out = {"windows": plan, "gain": gain}
            if alphas is not None:
                out["alphas"] = [float(a) for a in torch.as_tensor(alphas).reshape(-1).tolist()]
            if alphas is None:
                pred = self.model.get_pred_spec_mag_norm(masked_norm, mask4, reuse=False)
                waves, info = PH.griffin_lim_gap(torch.exp(pred[:, 0] * std + mean), masked, mask_f, **kw)
                stack = waves                                                           # [W, 1, Lw]
            else:
                pc = self.model(masked_norm, mask4)
                pred = self.model.get_pred_spec_mag_norm(masked_norm, mask4)
                var, rest, info = PH.pc_audio_variations_blind(pred, pc, masked, mask_f, alphas, mean, std, **kw)
                K, A = var.shape[1], var.shape[2]
                stack = _stacked(var, rest)                                             # [W, K A + 1, Lw], prediction last
            if alphas is not None and variations == "full":
                full = splice_windows(x, gaps_d, starts_d, stack, gain, c.crossfade_samples)
                out["variations"], out["restored"] = full[:K * A].view(K, A, -1), full[K * A]
            else:
                out["restored"] = splice_windows(x, gaps_d, starts_d, stack[:, -1], gain, c.crossfade_samples)[0]
                if alphas is not None:
                    out["variation_windows"] = var / gain.float()
            out.update(info)
            if S is not None:
                from . import posterior as IPOST
                if alphas is None:
                    pc = self.model(masked_norm, mask4)
                    pred = self.model.get_pred_spec_mag_norm(masked_norm, mask4)
                z = IPOST.as_coefficients(coeffs).to(x.device) if coeffs is not None else IPOST.draw_coefficients(
                    W, S, pc.shape[1], seed=seed, device=x.device)
                smp, _, sinfo = IPOST.sample_waveforms_blind(pred, pc, masked, mask_f, z, mean, std, **kw)
                out["coeffs"], out["sample_status"] = z, sinfo["status"]
                if variations == "full":
                    out["samples"] = splice_windows(x, gaps_d, starts_d, smp, gain, c.crossfade_samples)
                out["sample_windows"] = smp / gain.float()
        if bool(info["status"].any()):                                                  # the one host read
            raise RuntimeError(f"griffin_lim_gap refused windows {info['status'].nonzero().flatten().tolist()}: their gap "
                               "span exceeds the cap (plan_windows should have raised)")
        return out

    def _restore_native(self, wave, gaps, alphas, variations, rate, samples=None, seed=None, coeffs=None):
        """restore() for a recording at `rate` != config.sample_rate:
          the recording is resampled to config.sample_rate (nppc_audio.resample, the reference's windowed sinc); every gap
          [s, e) becomes resample.map_gap's [a, b), the outputs the gap's samples reach through the filter, so nothing
          outside the mapped gaps depends on what the gaps hold; restore() runs on that, unchanged; its result is resampled
          back, cut to len(wave) and spliced AT `rate` (nppc_rec_splice with the upsampled recording as one stride-0
          window starting at sample 0 and a gain of one): inside each gap (gaps closer than twice the native crossfade
          ceil(crossfade_samples rate / config.sample_rate) are merged) the upsampled signal, a raised-cosine blend over
          the native crossfade on both sides, and everywhere else the input's own samples, bit for bit and full band.
        The model is a config.sample_rate model: inside the gaps nothing above config.sample_rate / 2 is synthesised.
        Posterior samples (samples / seed / coeffs, variations='full') ride through the same resample-up and splice as
        the K A variations, as S more rows.
        Adds 'sample_rate', 'restored_model_rate' [ceil(L model / rate)], 'gaps_model_rate' (the mapped gaps, in the order
        given) and 'gaps_merged' (the native gaps as spliced).  Still one host read: the inner call's status check."""
        from .. import resample as RSM
        c = self.config
        if rate <= 0:
            raise ValueError(f"sample_rate = {rate}: not a rate")
        if coeffs is None:
            self._check_samples(samples, None, 0)                                       # a bad S, before anything is launched
        N = wave.numel()
        pairs = []
        for g in gaps:
            try:
                s, e = (int(v) for v in g)
            except (TypeError, ValueError) as err:
                raise ValueError(f"gap {g!r} is not a (start, end) pair of samples") from err
            if s < 0 or e <= s or e > N:
                raise ValueError(f"gap ({s}, {e}) is empty, negative or outside the recording's {N} samples")
            pairs.append((s, e))
        extra = {"sample_rate": rate, "restored_model_rate": None, "gaps_model_rate": [], "gaps_merged": []}
        if not pairs:
            if self._check_samples(samples, coeffs, 0) is not None:
                extra.update(coeffs=None, sample_windows=None)
            return {"restored": wave, "windows": [], "gain": None, "inconsistency": None, "target_norm": None,
                    "status": None, **extra}
        down_t, up_t = RSM.sinc_table(rate, c.sample_rate), RSM.sinc_table(c.sample_rate, rate)
        for t, pair in ((down_t, (rate, c.sample_rate)), (up_t, (c.sample_rate, rate))):
            if t.tile == 0:                                                             # before anything is launched
                raise RSM._unsupported(t, *pair)
        H.require_gpu()
        n_model = RSM.out_length(N, rate, c.sample_rate)
        mapped = [RSM.map_gap(s, e, down_t, out_len=n_model) for s, e in pairs]
        for (s, e), (a, b) in zip(pairs, mapped):
            if b <= a:
                raise ValueError(f"gap ({s}, {e}) reaches no sample at {c.sample_rate} Hz")
        xf = native_crossfade(c.crossfade_samples, rate, c.sample_rate)
        merged = merge_native_gaps(pairs, xf)
        x = wave.to(self.device).float().contiguous()
        with torch.no_grad():
            low = RSM.resample(x, rate, c.sample_rate, backend="hip")
            out = self.restore(low, mapped, alphas, variations, samples=samples, seed=seed, coeffs=coeffs)
            rows = []
            if "variations" in out:
                K, A = out["variations"].shape[:2]
                rows.append(out["variations"].reshape(K * A, -1))
            if "samples" in out:
                rows.append(out["samples"])
            stack = torch.cat(rows + [out["restored"][None]]) if rows else out["restored"][None]
            up = RSM.resample(stack, c.sample_rate, rate, backend="hip")                # [V, >= N], one batched launch
            gaps_d = torch.tensor(merged, dtype=torch.int64).to(x.device)
            zeros = torch.zeros(len(merged), dtype=torch.int64, device=x.device)
            one = torch.ones(1, dtype=torch.float64, device=x.device)
            V = up.shape[0]
            full = torch.empty(V, N, dtype=torch.float32, device=x.device)
            H.call("nppc_rec_splice", x, N, gaps_d, zeros, len(merged), up, 0, up.stride(0), N, V, xf, one, full, H.stream())
        out["restored_model_rate"] = out["restored"]
        out["restored"] = full[V - 1]
        if "variations" in out:
            out["variations"] = full[:K * A].view(K, A, N)
        if "samples" in out:
            out["samples"] = full[V - 1 - out["samples"].shape[0]:V - 1]
        out.update(sample_rate=rate, gaps_model_rate=mapped, gaps_merged=merged)
        return out

    def detect_gaps(self, wave):
        """the maximal runs of exactly-zero samples at least config.min_gap_samples long, [(start, end)] ascending: how a
        digital dropout looks, and the reference's masked_audio = audio * mask.  On the device (nppc_zero_runs); one host
        read (two when there are more than 1024 runs)."""
        H.require_gpu()
        x = wave.to(self.device).float().contiguous()
        cap = 1024
        while True:
            runs, count = zero_runs(x, self.config.min_gap_samples, cap)
            host = torch.cat([count, runs.flatten()]).cpu()
            n = int(host[0])
            if n <= cap:
                return [(int(s), int(e)) for s, e in host[1:1 + 2 * n].view(-1, 2).tolist()]
            cap = n

    def restore_file(self, path_in, path_out, gaps=None, verify_flac_md5=True, keep_rate=False, out_format="wav",
                     flac_predictor="fixed"):
        """wav or flac -> wav or flac: decodes with data._decode_wav, or data._decode_flac for a name ending in .flac (mono,
        config.sample_rate), detects the gaps when none are given, restores, writes 16-bit PCM: out_format "wav" (the
        default), "flac" (flac.encode_waves: the same samples, at the rate the wav would have had) or "auto" (flac when
        path_out ends in .flac).  A flac file whose STREAMINFO states an MD5 is checked against it (flac.FlacError, status
        9, when the decoded samples differ); verify_flac_md5=False takes it as it decodes.  -> restore's dict
        keep_rate=True: the file is decoded at ITS rate (the wav header's, flac.probe's), the gaps are detected on those
        samples -- a filter would smear the exact zeros of a dropout -- and given at that rate, restore(...,
        sample_rate=rate) keeps every sample outside the crossfaded gaps, and the wav written has the file's rate and
        sample count.  Inside the gaps there is nothing above config.sample_rate / 2.
        flac_predictor: the FLAC encoder's predictor, "fixed" or "lpc" (flac.encode_pcm)."""
        import numpy as np
        from scipy.io import wavfile
        from ..data import _decode_flac, _decode_wav
        if out_format not in ("wav", "flac", "auto"):
            raise ValueError(f"out_format = {out_format!r}: 'wav', 'flac' or 'auto'")
        if out_format == "auto":
            out_format = "flac" if str(path_out).lower().endswith(".flac") else "wav"
        is_flac = str(path_in).lower().endswith(".flac")
        rate = self.config.sample_rate
        if keep_rate:
            if is_flac:
                from ..flac import probe
                rate = int(probe(path_in).sample_rate)
            else:
                rate = int(wavfile.read(str(path_in), mmap=True)[0])
        if is_flac:
            wave = _decode_flac(path_in, rate, verify_md5=verify_flac_md5)
        else:
            wave = _decode_wav(path_in, rate)
        if wave is None:
            raise ValueError(f"{path_in} holds no samples")
        if gaps is None:
            gaps = self.detect_gaps(wave)
        out = self.restore(wave, gaps, sample_rate=rate) if keep_rate else self.restore(wave, gaps)
        if out_format == "flac":
            from ..flac import write_waves
            write_waves([path_out], out["restored"][None], rate, "flac", predictor=flac_predictor)
            return out
        pcm = np.clip(np.rint(out["restored"].detach().cpu().double().numpy() * 32768.0), -32768, 32767).astype(np.int16)
        wavfile.write(str(path_out), rate, pcm)
        return out

    def save_variations(self, out, directory, fmt="flac", alphas=None, flac_predictor="fixed"):
        """restore's dict -> <directory>/restored.<ext> and, when it holds 'variations' [K, A, L] (restore(..., alphas,
        variations="full")), <directory>/pc_<k+1>/alpha_<a:.1f>.<ext>: 16-bit mono at the rate of the dict.  fmt "flac"
        encodes every waveform in one device call (flac.encode_waves), "wav" writes the same samples.  When it holds
        'samples' [S, L] (restore(..., samples=S, variations="full")) also <directory>/posterior/sample_<s>.<ext>.  alphas: the sweep,
        when the dict does not carry it ('alphas', which restore adds).  flac_predictor: the FLAC encoder's predictor, "fixed" or
        "lpc" (flac.encode_pcm).  -> the paths written"""
        import os
        from ..flac import write_waves
        rate = int(out.get("sample_rate", self.config.sample_rate))
        paths, waves = [os.path.join(str(directory), f"restored.{fmt}")], [out["restored"].reshape(1, -1)]
        if "variations" in out:
            var = out["variations"]
            K, A, L = var.shape
            alphas = out.get("alphas") if alphas is None else alphas
            alphas = [float(a) for a in (alphas.tolist() if hasattr(alphas, "tolist") else alphas or [])]
            if len(alphas) != A:
                raise ValueError(f"{len(alphas)} alphas for {A} variations per direction")
            paths += [os.path.join(str(directory), f"pc_{k + 1}", f"alpha_{a:.1f}.{fmt}") for k in range(K) for a in alphas]
            waves.append(var.reshape(K * A, L))
        if out.get("samples") is not None:
            smp = out["samples"]
            paths += [os.path.join(str(directory), "posterior", f"sample_{i}.{fmt}") for i in range(smp.shape[0])]
            waves.append(smp)
        write_waves(paths, torch.cat([w.to(self.device).float() for w in waves]) if fmt == "flac"
                    else torch.cat([w.float().cpu() for w in waves]), rate, fmt, predictor=flac_predictor)
        return paths


def _stacked(variations, restored):
    """pc_audio_variations_blind returns two views of one [W, K A + 1, L] buffer: that buffer, without a copy when the
    views still are what they were"""
    W, K, A, L = variations.shape
    V = K * A + 1
    if (variations.stride() == (V * L, A * L, L, 1) and restored.stride() == (V * L, 1)
            and restored.data_ptr() == variations.data_ptr() + K * A * L * 4):
        return torch.as_strided(variations, (W, V, L), (V * L, L, 1))
    return torch.cat([variations.reshape(W, K * A, L), restored[:, None]], 1)
