"""Energy voice-activity detector and the gap draw of the inpainting dataset, on the HIP device (csrc/inpaint_data.hip).

The reference places the inpainting gap inside a speech segment found by silero-vad (dataset/audio_dataset_inpainting.py
:183-221).  silero is a network fetched through torch.hub and is not part of this build; this detector is an ENERGY
detector with the same output contract (a list of [start, end) sample ranges per clip, none shorter than the gap) and the
shape of silero's get_speech_timestamps post-processing.  Its segments differ from silero's on real speech; no parity with
the reference's gaps is claimed.  The specification is tests/vad_ref.py (fp64 NumPy), DESIGN.md section 8e.
"""
from typing import Optional

import pydantic
import torch

from .. import _hip as H

__all__ = ["EnergyVadConfig", "MAX_WINDOWS", "vad_window", "energy_vad", "draw_gaps"]

MAX_WINDOWS = 2048           # csrc/inpaint_data.hip: the window levels of one clip live in LDS
SEED_MASK = 0x7FFFFFFFFFFFFFFF


class EnergyVadConfig(pydantic.BaseModel):
    """Constants of the energy detector.  A window is speech-like when its level is `on_db` above the clip's noise floor
    (the `floor_percentile` nearest-rank percentile of the window levels) and within `range_db` of the clip's loudest
    window; a segment ends after `min_silence_ms` below that threshold minus `hysteresis_db`.

    These defaults are a judgement: nobody has tuned them on speech.  What is pinned (and tested) is the algorithm."""
    on_db: float = 15.0
    range_db: float = 40.0
    hysteresis_db: float = 5.0
    floor_percentile: float = pydantic.Field(0.10, ge=0.0, le=1.0)
    min_silence_ms: float = pydantic.Field(100.0, ge=0.0)

    def min_silence_samples(self, sample_rate: int) -> int:
        return int(sample_rate * self.min_silence_ms / 1000)


def vad_window(sample_rate: int) -> int:
    """silero's window: 512 samples at 16 kHz, 256 at 8 kHz"""
    if sample_rate == 16000:
        return 512
    if sample_rate == 8000:
        return 256
    raise ValueError(f"the voice-activity detector runs at 8000 or 16000 Hz, got {sample_rate}")


def max_segments(length: int, win: int) -> int:
    """rows of the segment table: a segment takes at least one window and the window that ends it"""
    return max(1, (length // win + 1) // 2)


def check_windows(length: int, win: int):
    if length // win > MAX_WINDOWS:
        raise ValueError(f"{length} samples are {length // win} windows of {win}; the detector supports {MAX_WINDOWS} "
                         f"({MAX_WINDOWS * win} samples)")


def _index_tensor(index, B, dev):
    t = torch.as_tensor(index, dtype=torch.int32, device=dev).reshape(-1)
    if t.numel() == 1 and B > 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"index has {t.numel()} entries for {B} items")
    return t.contiguous()


def energy_vad(wave, missing_length: int, cfg: Optional[EnergyVadConfig] = None, sample_rate: int = 16000):
    """wave [B, L] fp32 on the device -> (segments [B, S_max, 2] int32, n_segments [B] int32), both on the device:
    item b has the n_segments[b] speech segments [start, end) of segments[b, :n_segments[b]], in order, each at least
    missing_length samples long; rows past them hold -1.  One launch, no host synchronisation."""
    H.require_gpu()
    cfg = cfg or EnergyVadConfig()
    if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
        raise ValueError("wave must be a tensor on the HIP device")
    if wave.dim() != 2:
        raise ValueError(f"wave is [B, L], got {tuple(wave.shape)}")
    wave = wave.contiguous().float()
    B, L = wave.shape
    win = vad_window(sample_rate)
    missing_length = int(missing_length)
    if not 0 < missing_length <= L:
        raise ValueError(f"missing_length {missing_length} must lie in [1, L = {L}]")
    check_windows(L, win)
    dev = wave.device
    S = max_segments(L, win)
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * L
    gains = torch.ones(B, dtype=torch.float32, device=dev)
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    segments = torch.empty(B, S, 2, dtype=torch.int32, device=dev)
    n_segments = torch.empty(B, dtype=torch.int32, device=dev)
    g0, g1, fb = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    H.call("nppc_inpaint_vad_batch", wave, B * L, offsets, gains, B, rows, rows, B, L, win, missing_length, -1, 1, 0, 0, 0,
           0.0, cfg.on_db, cfg.range_db, cfg.hysteresis_db, cfg.floor_percentile, cfg.min_silence_samples(sample_rate), S,
           None, None, g0, g1, segments, n_segments, fb, H.stream())
    return segments, n_segments


def draw_gaps(segments, n_segments, length: int, missing_length: int, seed: int, index, epoch: int = 0,
              missing_start: Optional[int] = None):
    """the gap of AudioInpaintingDataset._create_mask (:199-221) for every item, on the device: segments [B, S, 2] and
    n_segments [B] as `energy_vad` returns them (n_segments = 0: the random gap of _create_random_mask, which is also the
    result for a chosen segment not longer than the gap), `index` the item indices [B] (or one int), -> (gap_start,
    gap_end, used_fallback), int32 [B].  The draws are Philox4x32-10 with key `seed` and counter (index, epoch, 0, purpose);
    missing_start (samples) fixes the fallback gap instead of drawing it."""
    H.require_gpu()
    for name, t in (("segments", segments), ("n_segments", n_segments)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on the HIP device")
    if segments.dim() != 3 or segments.shape[2] != 2 or segments.shape[1] < 1:
        raise ValueError(f"segments is [B, S, 2] with S >= 1, got {tuple(segments.shape)}")
    B, S, _ = segments.shape
    dev = segments.device
    segments = segments.to(torch.int32).contiguous()
    n_segments = n_segments.to(torch.int32).contiguous()
    if tuple(n_segments.shape) != (B,):
        raise ValueError(f"n_segments has shape {tuple(n_segments.shape)}, expected {(B,)}")
    length, missing_length = int(length), int(missing_length)
    fixed = -1 if missing_start is None else int(missing_start)
    if not 0 < missing_length <= length or (fixed >= 0 and fixed + missing_length > length):
        raise ValueError(f"a gap of {missing_length} samples (fixed start {missing_start}) does not fit into {length}")
    g0, g1, fb = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    H.call("nppc_inpaint_draw_gaps", segments, n_segments, _index_tensor(index, B, dev), B, length, missing_length, fixed, S,
           int(seed) & SEED_MASK, int(epoch), g0, g1, fb, H.stream())
    return g0, g1, fb
