"""Audio from an inpainted spectrogram WITHOUT the clean phase: Griffin-Lim restricted to the gap (csrc/gl_gap.hip,
DESIGN.md section 8c; specification tests/gl_gap_ref.py).

The restorer and the direction net predict log-magnitudes only.  `pc_audio_variations` (validator) borrows the phase of the
clean recording, which exists for held-out data alone.  Here the magnitude inside the gap comes from the model, the complex
STFT outside the gap comes from the damaged recording and is held fixed, and only the phase of the gap frames is iterated:

    C_0 = where(gap, M exp(i phi0), Kn)
    x_n = istft(C_n);  R_n = stft(x_n);  A = R_n - mu / (1 + mu) R_{n-1};  C_{n+1} = where(gap, M A / (|A| + 1e-16), Kn)

A blind reconstruction is judged by its spectral consistency (`info['inconsistency'] / info['target_norm']`), not by a
waveform SDR against the clean signal: many waveforms share a magnitude.
A gap whose span (its frames' bounding range + the neighbour frames) exceeds the resident kernel's cap is refused by
default (NaN, status 1); `long_spans=True` runs such items through the tiled path (csrc/gl_gap_long.hip, DESIGN.md section
8g): the same algorithm and the same bits, the state in a workspace instead of LDS, one launch per half-iteration.
`inconsistency` sums the one-sided bins unweighted, as the contract states it; in that norm it is not guaranteed to be
non-increasing from step to step (DESIGN.md section 8c has the measurements).
"""
import ctypes

import torch

from .. import _hip as H
from .. import ops

__all__ = ["griffin_lim_gap", "phase_advance_init", "pc_audio_variations_blind", "gl_gap_shape", "GL_MAX_SPAN_FRAMES"]



def __getattr__(name):
    """GL_MAX_SPAN_FRAMES: the compiled NPPC_GL_MAX_SPAN_FRAMES, read from the library (a configuration small enough that
    the LDS budget does not lower the cap)"""
    if name == "GL_MAX_SPAN_FRAMES":
        return gl_gap_shape(1, 1, 2, 2, n_fft=2, hop_length=2, length=2, n_iter=0)["span_cap"]
    raise AttributeError(name)


_WHY = {1: "{F} frequency bins do not fit n_fft {n_fft} (n_fft // 2 + 1 = {Fw})",
        2: "length {L} at hop {hop} has {Tw} frames, the spectrogram has {T} (1 + length // hop_length must equal T)",
        3: "n_fft {n_fft} / hop {hop} outside n_fft <= 512, ceil(n_fft / hop) <= 8",
        4: "n_iter {n_iter} and momentum {momentum} must not be negative",
        5: "unsupported arguments: B {B}, V {V}, T {T}, n_fft {n_fft}, hop {hop}, length {L}, max_span {max_span} "
           "(1 <= hop <= n_fft, length >= n_fft, max_span > 2 (ceil(n_fft / hop) - 1))"}
_LONG_MODES = {False: 0, True: 1, "always": 2}


def _long_mode(long_spans):
    if not isinstance(long_spans, (bool, str)) or long_spans not in _LONG_MODES:
        raise ValueError(f"long_spans = {long_spans!r}: False, True or 'always'")
    return _LONG_MODES[long_spans]


def gl_gap_shape(B, V, F, T, n_fft=255, hop_length=128, length=None, n_iter=32, momentum=0.0, max_span=None, long_spans=False,
                 long_max_span=None):
    """nppc_gl_gap_shape: runs without a GPU and carries the argument rules as ValueErrors.
    -> dict(length, r, span_cap, lds_bytes, work_bytes); with long_spans (nppc_gl_gap_long_shape: the same rules) also
    long_span_cap, the cap of the tiled path (T + 2 r unless long_max_span lowers it), and work_bytes covers both paths."""
    L = ops.istft_natural_length(n_fft, hop_length, T) if length is None else int(length)
    mode = _long_mode(long_spans)
    name = "nppc_gl_gap_long_shape" if mode else "nppc_gl_gap_shape"
    fn = getattr(H.lib(), name)
    fn.argtypes, fn.restype = H.SIGS[name], ctypes.c_int
    why, r, cap, lcap = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lds, work = ctypes.c_long(), ctypes.c_long()
    ms = 0 if max_span is None else int(max_span)
    if long_max_span is not None and int(long_max_span) <= 0:
        raise ValueError(f"griffin_lim_gap: long_max_span = {long_max_span}: a positive number of frames, or None")
    try:
        args = [int(B), int(V), int(F), int(T), int(n_fft), int(hop_length), L, int(n_iter), float(momentum), ms]
        if mode:
            args.append(0 if long_max_span is None else int(long_max_span))
        refs = [why, r, cap] + ([lcap] if mode else []) + [lds, work]
        rc = fn(*args, *(ctypes.byref(v) for v in refs))
    except (ctypes.ArgumentError, OverflowError) as err:
        raise ValueError(f"griffin_lim_gap: {err}") from err
    if rc != 0:
        raise ValueError("griffin_lim_gap: " + _WHY[why.value if why.value in _WHY else 5].format(
            F=F, Fw=n_fft // 2 + 1, n_fft=n_fft, hop=hop_length, L=L, T=T, Tw=1 + L // max(hop_length, 1), n_iter=n_iter,
            momentum=momentum, B=B, V=V, max_span=max_span))
    out = {"length": L, "r": r.value, "span_cap": cap.value, "lds_bytes": lds.value, "work_bytes": work.value}
    if mode:
        out["long_span_cap"] = lcap.value
    return out


def _f32c(t):
    return t.contiguous().float()


def phase_advance_init(known_spec, mask, n_fft=255, hop_length=128):
    """Default initial phase: known_spec [B,2,F,T], mask [B,T] (1 = known) -> [B,F,T]; for each maximal run of gap frames
    phi0[f,t] = angle(Kn[f,t0]) + 2 pi f hop (t - t0) / n_fft with t0 the known frame left of the run (right of it for a
    run that starts at frame 0); 0 on known frames."""
    H.require_gpu()
    known_spec, mask = _f32c(known_spec), _f32c(mask)
    B, two, F, T = known_spec.shape
    if two != 2 or F != n_fft // 2 + 1 or mask.shape != (B, T):
        raise ValueError(f"known_spec {tuple(known_spec.shape)} / mask {tuple(mask.shape)} do not fit n_fft {n_fft}")
    phase = torch.empty(B, F, T, dtype=torch.float32, device=known_spec.device)
    H.call("nppc_gl_phase_init", known_spec, mask, phase, B, T, n_fft, hop_length, H.stream())
    return phase


def _prepare(known_spec, mask, init_phase, V, F, T, n_fft, hop_length, length, n_iter, momentum, max_span, long_spans=False,
             long_max_span=None):
    B = known_spec.shape[0]
    if known_spec.shape != (B, 2, F, T) or mask.shape != (B, T):
        raise ValueError(f"known_spec {tuple(known_spec.shape)} / mask {tuple(mask.shape)} do not fit [B={B}, F={F}, T={T}]")
    sh = gl_gap_shape(B, V, F, T, n_fft, hop_length, length, n_iter, momentum, max_span, long_spans, long_max_span)
    H.require_gpu()
    dev = known_spec.device
    if init_phase is None:
        init_phase = phase_advance_init(known_spec, mask, n_fft, hop_length)
    init_phase = _f32c(init_phase)
    if init_phase.shape not in ((B, F, T), (B, V, F, T)):
        raise ValueError(f"init_phase {tuple(init_phase.shape)} is neither [B,F,T] nor [B,V,F,T]")
    L = sh["length"]
    bufs = {"out": torch.empty(B, V, L, dtype=torch.float32, device=dev),
            "dist": torch.empty(B, V, n_iter, dtype=torch.float64, device=dev),
            "tn": torch.empty(B, V, dtype=torch.float64, device=dev),
            "status": torch.empty(B, dtype=torch.int32, device=dev),
            "work": torch.empty(sh["work_bytes"], dtype=torch.uint8, device=dev)}
    return sh, init_phase, bufs


def _tail(max_span, long_spans, long_max_span):
    """the arguments between momentum and the stream, and the entry point's suffix"""
    ms = 0 if max_span is None else int(max_span)
    mode = _long_mode(long_spans)
    if not mode:
        return "", (ms,)
    return "_long", (ms, 0 if long_max_span is None else int(long_max_span), mode)


def griffin_lim_gap(target_mag, known_spec, mask, n_iter=32, momentum=0.0, init_phase=None, n_fft=255, hop_length=128,
                    length=None, max_span=None, long_spans=False, long_max_span=None):
    """Gap-constrained Griffin-Lim.  target_mag [B,V,F,T] or [B,F,T] (linear magnitudes, read on gap frames only),
    known_spec [B,2,F,T] (read on known frames only), mask [B,T] (1 = known, 0 = gap), init_phase [B,F,T] or [B,V,F,T]
    (default phase_advance_init) -> (waves [B,V,L], info) with info = {'inconsistency' [B,V,n_iter] fp64: distance of
    stft(x_n) to the constraint set before step n, 'target_norm' [B,V] fp64 = |M| on the gap (divide by it yourself: it is 0
    for an item without a gap), 'status' [B] int32: 1 = the item's gap span exceeds the cap, its outputs are NaN}.
    momentum 0 is classic Griffin-Lim, 0.99 the fast variant.  max_span lowers the span cap (bounding range of the gap
    frames + 2 (ceil(n_fft / hop) - 1) neighbours) below GL_MAX_SPAN_FRAMES: less LDS per workgroup, more of them per CU.
    long_spans=True: an item over the cap runs the tiled path in the same call instead of being refused, items within it run
    as before; 'always': every item runs the tiled path (bit-equal waveforms; 'inconsistency' and 'target_norm' are folded
    in another order and agree to the last bits only).  long_max_span caps the tiled path's span (default: any gap of the
    clip) and with it the workspace; an item over it is refused as above.
    Nothing here synchronises with the host."""
    target_mag, known_spec, mask = _f32c(target_mag), _f32c(known_spec), _f32c(mask)
    if target_mag.dim() == 3:
        target_mag = target_mag.unsqueeze(1)
    if target_mag.dim() != 4 or known_spec.dim() != 4 or target_mag.shape[0] != known_spec.shape[0]:
        raise ValueError(f"target_mag {tuple(target_mag.shape)} / known_spec {tuple(known_spec.shape)}: want [B,V,F,T] / [B,2,F,T]")
    B, V, F, T = target_mag.shape
    sh, init_phase, w = _prepare(known_spec, mask, init_phase, V, F, T, n_fft, hop_length, length, n_iter, momentum, max_span,
                                 long_spans, long_max_span)
    suffix, tail = _tail(max_span, long_spans, long_max_span)
    with ops.envelope_refusal(n_fft, hop_length, T, sh["length"]):
        H.call("nppc_gl_gap" + suffix, target_mag, known_spec, mask, init_phase, int(init_phase.dim() == 4), w["out"], w["dist"], w["tn"],
               w["status"], w["work"], w["work"].numel(), B, V, T, n_fft, hop_length, sh["length"], n_iter, float(momentum),
               *tail, H.stream())
    return w["out"], {"inconsistency": w["dist"], "target_norm": w["tn"], "status": w["status"]}


def pc_audio_variations_blind(pred_spec_mag, pc_directions_mag, masked_spec, mask, alphas, mean, std, n_iter=32, momentum=0.0,
                              init_phase=None, n_fft=255, hop_length=128, length=None, max_span=None, long_spans=False,
                              long_max_span=None):
    """pc_audio_variations without the clean phase: pred_spec_mag [B,1,F,T], pc_directions_mag [B,K,F,T] (normalised
    log-magnitudes), masked_spec [B,2,F,T] (the damaged recording's STFT), mask [B,T] or [B,1,F,T], alphas [A], mean / std
    (device scalars, read on the device) -> (variations [B,K,A,L], restored [B,L], info):
        variations[b,k,a] = griffin_lim_gap(exp((pred[b] + alphas[a] pc[b,k]) std + mean), ...)
        restored[b]       = the same at alpha = 0
    from one call; the B K A F T magnitude stack is never formed.  info as griffin_lim_gap with V = K A + 1 (the
    prediction last).  long_spans / long_max_span as griffin_lim_gap."""
    pred, pc, known = _f32c(pred_spec_mag), _f32c(pc_directions_mag), _f32c(masked_spec)
    if pc.dim() != 4:
        raise ValueError(f"pc_directions_mag {tuple(pc.shape)}: want [B,K,F,T]")
    B, K, F, T = pc.shape
    if pred.shape != (B, 1, F, T):
        raise ValueError(f"pred_spec_mag {tuple(pred.shape)} does not fit directions {tuple(pc.shape)}")
    mask = _f32c(mask)
    if mask.dim() == 4:
        mask = mask[:, 0, 0, :].contiguous()
    alphas = torch.as_tensor(alphas, dtype=torch.float32).to(pc.device).contiguous().reshape(-1)
    A = alphas.numel()
    if A == 0:
        raise ValueError("no alphas given")
    V = K * A + 1
    sh, init_phase, w = _prepare(known, mask, init_phase, V, F, T, n_fft, hop_length, length, n_iter, momentum, max_span,
                                 long_spans, long_max_span)
    suffix, tail = _tail(max_span, long_spans, long_max_span)
    if init_phase.dim() != 3:
        raise ValueError("pc_audio_variations_blind takes one initial phase per item, [B,F,T]")
    as_scalar = lambda v: torch.as_tensor(v, dtype=torch.float32).to(pc.device).reshape(1).contiguous()
    with ops.envelope_refusal(n_fft, hop_length, T, sh["length"]):
        H.call("nppc_gl_gap_pc" + suffix, pred, pc, as_scalar(mean), as_scalar(std), alphas, known, mask, init_phase, w["out"], w["dist"],
               w["tn"], w["status"], w["work"], w["work"].numel(), B, K, A, T, n_fft, hop_length, sh["length"], n_iter,
               float(momentum), *tail, H.stream())
    L = sh["length"]
    info = {"inconsistency": w["dist"], "target_norm": w["tn"], "status": w["status"]}
    return w["out"][:, :K * A].reshape(B, K, A, L), w["out"][:, K * A], info
