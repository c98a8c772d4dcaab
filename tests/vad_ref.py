"""fp64 NumPy restatement of the inpainting dataset's energy voice-activity detector and gap draw: the specification of
csrc/inpaint_data.hip and nppc_audio/inpainting/vad.py.  The reference places its gaps with silero-vad, a network that is
not available to this project, so nothing here was compared with silero; what is kept is the contract of
AudioInpaintingDataset._create_mask (dataset/audio_dataset_inpainting.py:183-221): the gap lies inside a detected speech
segment longer than the gap, otherwise it is the gap of _create_random_mask (:170-181).

Per clip x of L samples:
- Windows: W = L // win non-overlapping windows (win = 512 at 16 kHz, 256 at 8 kHz); samples past W * win are ignored.
- Level: e_w = 10 log10(mean(x_w^2) + 1e-12) dB.
- Floor n = sorted(e)[floor(q (W - 1))] (nearest rank), peak pk = max(e).
- theta_on = max(n + on_db, pk - range_db), theta_off = theta_on - hysteresis_db; pk - n < on_db: no segments.
- Segments, over the windows in order (the shape of silero's get_speech_timestamps post-processing, no speech padding):
    not triggered and e_w >= theta_on: start = w win, triggered;
    triggered and e_w < theta_off: temp_end = w win if unset; once w win - temp_end >= min_silence the segment
      [start, temp_end) closes, untriggered;
    triggered, e_w >= theta_on and temp_end set: temp_end is cleared;
    at the end an open segment closes at temp_end if set, else at W win;
    a closed segment is kept iff its length >= min_speech (= missing_length).
- Gap: no segment -> fallback; else segment k = uniform_int(0, n_seg - 1); length <= missing_length -> fallback; else
  gap_start = seg_start + uniform_int(0, length - missing_length).  Fallback: missing_start when set, else
  uniform_int(0, L - missing_length).  use_vad False: always the fallback.
- Random numbers: Philox4x32-10, key = the 64-bit seed (low word, high word), counter (item, epoch, 0, purpose) with
  purpose 0 crop start, 1 segment choice, 2 gap offset (also the fallback's), 3 dBFS float; the first output word u;
  uniform_int(0, n) = (u (n + 1)) >> 32.
- Crop: uniform_int(0, file_len - L) when file_len > L and the crop is random, else 0.
- Level float f > 0: the whole-file gain is multiplied by fp32(10^(f (2 u / 2^32 - 1) / 20)).
"""
import math

import numpy as np

CROP, SEGMENT, OFFSET, DBFS = 0, 1, 2, 3
M32 = 0xFFFFFFFF
DEFAULTS = dict(on_db=15.0, range_db=40.0, hysteresis_db=5.0, floor_percentile=0.10, min_silence_ms=100.0)


def philox4x32_10(counter, key):
    """Salmon et al. 2011: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, item, epoch, purpose):
    return philox4x32_10((item, epoch, 0, purpose), (seed & M32, (seed >> 32) & M32))[0]


def uniform_int(u, n):
    """integer in [0, n] from a 32-bit word"""
    return (int(u) * (int(n) + 1)) >> 32


def vad_window(sample_rate):
    return {16000: 512, 8000: 256}[sample_rate]


def window_levels(x, win):
    x = np.asarray(x, dtype=np.float64)
    W = len(x) // win
    return 10.0 * np.log10(np.mean(x[:W * win].reshape(W, win) ** 2, axis=1) + 1e-12)


def thresholds(e, on_db, range_db, hysteresis_db, floor_percentile):
    """-> (floor, peak, theta_on, theta_off)"""
    W = len(e)
    n = float(np.sort(e)[int(math.floor(floor_percentile * (W - 1)))])
    pk = float(np.max(e))
    on = max(n + on_db, pk - range_db)
    return n, pk, on, on - hysteresis_db


def energy_vad(x, missing_length, sample_rate=16000, **cfg):
    """-> list of (start, end) sample ranges"""
    c = dict(DEFAULTS, **cfg)
    win = vad_window(sample_rate)
    min_silence = int(sample_rate * c["min_silence_ms"] / 1000)
    W = len(x) // win
    if W == 0:
        return []
    e = window_levels(x, win)
    n, pk, on, off = thresholds(e, c["on_db"], c["range_db"], c["hysteresis_db"], c["floor_percentile"])
    if pk - n < c["on_db"]:
        return []
    out, triggered, start, temp_end = [], False, 0, None

    def close(s, t):
        if t - s >= missing_length:
            out.append((s, t))

    for w in range(W):
        pos = w * win
        if not triggered:
            if e[w] >= on:
                triggered, start, temp_end = True, pos, None
            continue
        if e[w] < off:
            if temp_end is None:
                temp_end = pos
            if pos - temp_end >= min_silence:
                close(start, temp_end)
                triggered, temp_end = False, None
        elif e[w] >= on and temp_end is not None:
            temp_end = None
    if triggered:
        close(start, temp_end if temp_end is not None else W * win)
    return out


def draw_gap(segments, length, missing_length, seed, item, epoch=0, missing_start=None, use_vad=True):
    """-> (gap_start, gap_end, used_fallback)"""
    start = None
    if use_vad and segments:
        s0, s1 = segments[uniform_int(draw(seed, item, epoch, SEGMENT), len(segments) - 1)]
        if s1 - s0 > missing_length:
            start = s0 + uniform_int(draw(seed, item, epoch, OFFSET), s1 - s0 - missing_length)
    fallback = start is None
    if fallback:
        start = missing_start if missing_start is not None else uniform_int(draw(seed, item, epoch, OFFSET),
                                                                            length - missing_length)
    return start, start + missing_length, int(fallback)


def crop_start(file_len, length, seed, item, epoch=0, random_crop=True):
    return uniform_int(draw(seed, item, epoch, CROP), file_len - length) if (file_len > length and random_crop) else 0


def level_gain(dbfs_float, seed, item, epoch=0):
    """the fp32 factor on the whole-file gain for target_dB_FS_floating_value = dbfs_float"""
    if not dbfs_float > 0:
        return np.float32(1.0)
    u = draw(seed, item, epoch, DBFS) / 4294967296.0
    return np.float32(10.0 ** (dbfs_float * (2.0 * u - 1.0) / 20.0))


def item(file_wave, gain, length, missing_length, seed, item_index, epoch=0, sample_rate=16000, use_vad=True,
         missing_start=None, random_crop=True, dbfs_float=0.0, **cfg):
    """one dataset item from a whole file (fp32 [n]) and its fp32 whole-file gain -> dict(crop_start, clean fp32 [L],
    segments, gap_start, gap_end, used_fallback)"""
    file_wave = np.asarray(file_wave, dtype=np.float32)
    c0 = crop_start(len(file_wave), length, seed, item_index, epoch, random_crop)
    g = np.float32(np.float32(gain) * level_gain(dbfs_float, seed, item_index, epoch))
    clean = file_wave[c0:c0 + length] * g                                  # fp32 product, like the kernel
    segs = energy_vad(clean, missing_length, sample_rate, **cfg) if use_vad else []
    g0, g1, fb = draw_gap(segs, length, missing_length, seed, item_index, epoch, missing_start, use_vad)
    return dict(crop_start=c0, clean=clean, segments=segs, gap_start=g0, gap_end=g1, used_fallback=fb)


# ---- constructed clips shared by the CPU and GPU tests --------------------------------------------------------------------
def bursts(length, spans, seed, burst_db=-25.0, floor_db=-75.0):
    """white noise at floor_db dBFS with noise bursts at burst_db over the sample ranges `spans` -> fp32 [length]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(length) * 10.0 ** (floor_db / 20.0)
    for s, t in spans:
        x[s:t] = rng.standard_normal(t - s) * 10.0 ** (burst_db / 20.0)
    return x.astype(np.float32)


def six_clips(length=8000):
    """the six constructed clips at `length` >= 8000 samples, 16 kHz, for a gap of 1024 samples (64 ms):
    merge (a 50 ms pause inside one segment), split (a 300 ms pause), short (a burst shorter than the gap is dropped),
    ends_in_speech, flat (no segments), plain (one burst in the middle).  name -> (fp32 clip, expected segments)"""
    W = length // 512 * 512
    return {
        "merge": (bursts(length, [(512, 2048), (2848, 4608)], 1), [(512, 4608)]),
        "split": (bursts(length, [(0, 1536), (6336, length)], 2), [(0, 1536), (6144, W)]),
        "short": (bursts(length, [(1024, 1536), (4096, 6656)], 3), [(4096, 6656)]),
        "ends_in_speech": (bursts(length, [(5120, length)], 4), [(5120, W)]),
        "flat": (bursts(length, [(0, length)], 5), []),
        "plain": (bursts(length, [(2048, 5632)], 6), [(2048, 5632)]),
    }


def margin_db(x, win=512, **cfg):
    """the smallest distance (dB) of any window level of x to theta_on and theta_off, and of pk - n to on_db"""
    c = dict(DEFAULTS, **cfg)
    e = window_levels(x, win)
    n, pk, on, off = thresholds(e, c["on_db"], c["range_db"], c["hysteresis_db"], c["floor_percentile"])
    return min(float(np.min(np.abs(e - on))), float(np.min(np.abs(e - off))), abs(pk - n - c["on_db"]))
