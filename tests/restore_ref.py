"""Specification of whole-recording restoration (nppc_audio/inpainting/restore.py, csrc/restore_rec.hip):
an fp64 NumPy restatement of plan_windows' arithmetic, the gain, the gather / mask, the splice and the zero-run search,
written from the contract, with sample-by-sample loops where the package uses closed forms.

Decisions this project makes that the reference does not (it only hints at the step, get_with_full_audio,
validator_nppc_model.py:518-526, and never restores a recording):
  1. gaps are half-open (start, end) sample pairs; two gaps closer than 2 x crossfade are merged into their hull, and the
     known samples between them are synthesised with the gap;
  2. one window of `window_samples` per merged gap, centred on the gap's midpoint ((s + e) // 2 - window // 2) and clamped
     to [0, length - window]; a gap is written back from its own window only; other gaps inside a window are masked there;
  3. a gap needs ceil(n_fft / hop) known frames on both sides inside its window, and the window's masked frames (bounding
     range + 2 (ceil(n_fft / hop) - 1) neighbours) must fit Griffin-Lim's span cap: otherwise ValueError, never a status;
  4. ONE gain per recording, _normalize_audio's formula (10^((target - 20 log10(rms + 1e-8)) / 20)) in fp64 with the RMS
     over the samples outside the (merged) gaps; window samples are (float)(double(x) * gain), exactly 0 inside gaps;
  5. the log-magnitude mean / std are batch-global over all windows of one call (utils.preprocess_data on the damaged STFT);
  6. splice: inside [s, e) the window output / gain; on [s - xf, s) and [e, e + xf) a raised-cosine blend
         out = rec + c (y - rec),  c = 0.5 - 0.5 cos(pi (t + 1) / (xf + 1)),
     t = 0 at the outer end of the ramp and xf - 1 next to the gap (c would be 0 one sample further out and 1 on the gap),
     clipped at the recording's ends; every other sample is the input's bits;
  7. a gap in a file is a maximal run of exactly-zero samples (-0.0 included) of at least min_len samples.
"""
import math

import numpy as np

CHUNK = 4096                      # NPPC_ZERO_RUN_CHUNK: only used to build inputs that straddle the kernel's chunks


def frame_mask(sample_mask, n_fft, hop):
    """time_to_spec_mask, centred: frame t is known iff every sample of [t hop - n_fft // 2, + n_fft) clipped to the
    signal is known (an empty window is masked).  sample_mask [L] -> [1 + L // hop]"""
    L = sample_mask.shape[0]
    T = 1 + L // hop
    out = np.zeros(T)
    for t in range(T):
        a, b = max(t * hop - n_fft // 2, 0), min(t * hop - n_fft // 2 + n_fft, L)
        out[t] = 1.0 if b > a and bool(np.all(sample_mask[a:b] == 1)) else 0.0
    return out


def merge_gaps(gaps, xf):
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in gaps):
        if out and s - out[-1][1] < 2 * xf:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def plan(length, gaps, window, xf, n_fft, hop, span_cap):
    """-> [(start, (s, e), frame mask of the window [T])] for valid input; ValueError with the reason's key word otherwise"""
    for s, e in gaps:
        if s < 0 or e <= s or e > length:
            raise ValueError(f"gap ({s}, {e})")
    if not gaps:
        return []
    if length < window:
        raise ValueError("fewer than one window")
    merged = merge_gaps(gaps, xf)
    need, r = math.ceil(n_fft / hop), math.ceil(n_fft / hop) - 1
    out = []
    for s, e in merged:
        ws = min(max((s + e) // 2 - window // 2, 0), length - window)
        sm = np.ones(length)
        for a, b in merged:
            sm[a:b] = 0
        fm = frame_mask(sm[ws:ws + window], n_fft, hop)
        own = np.ones(length)
        own[s:e] = 0
        of = np.flatnonzero(frame_mask(own[ws:ws + window], n_fft, hop) == 0)
        if fm[:of[0]].sum() < need or fm[of[-1] + 1:].sum() < need:
            raise ValueError("known frames")
        gone = np.flatnonzero(fm == 0)
        if gone[-1] - gone[0] + 1 + 2 * r > span_cap:
            raise ValueError("span cap")
        out.append((ws, (s, e), fm))
    return out


def gain(wave, gaps, target_dbfs=-25.0):
    known = np.ones(wave.shape[0], bool)
    for s, e in gaps:
        known[s:e] = False
    x = wave.astype(np.float64)[known]
    rms = math.sqrt(float(np.sum(x * x)) / x.size) if x.size else 0.0
    return 10.0 ** ((target_dbfs - 20.0 * math.log10(rms + 1e-8)) / 20.0)


def windows(wave, gaps, starts, window, g):
    """-> (samples [W, window] fp64 = wave * g, 0 inside every gap; sample mask [W, window])"""
    L = wave.shape[0]
    known = np.ones(L)
    for s, e in gaps:
        known[s:e] = 0
    x = wave.astype(np.float64) * g * known
    return np.stack([x[ws:ws + window] for ws in starts]), np.stack([known[ws:ws + window] for ws in starts])


def crossfade_weight(t, xf):
    """weight of the window output at ramp position t in [0, xf): 0 < c < 1, rising towards the gap"""
    return 0.5 - 0.5 * math.cos(math.pi * (t + 1) / (xf + 1))


def splice(wave, gaps, starts, window_out, g, xf):
    """wave [L], gaps [(s, e)] (gap i owned by window i), window_out [W, V, window] -> [V, L] fp64, sample by sample"""
    W, V, Lw = window_out.shape
    L = wave.shape[0]
    rec = wave.astype(np.float64)
    out = np.tile(rec, (V, 1))
    for i, ((s, e), ws) in enumerate(zip(gaps, starts)):
        y = window_out[i].astype(np.float64) / g
        for n in range(max(s - xf, 0, ws), min(e + xf, L, ws + Lw)):
            if s <= n < e:
                c = 1.0
            else:
                c = crossfade_weight(n - (s - xf) if n < s else e + xf - 1 - n, xf)
            out[:, n] = rec[n] + c * (y[:, n - ws] - rec[n]) if c < 1.0 else y[:, n - ws]
    return out


def spliced_region(L, gaps, xf):
    """bool [L]: samples the splice may change"""
    m = np.zeros(L, bool)
    for s, e in gaps:
        m[max(s - xf, 0):min(e + xf, L)] = True
    return m


def zero_runs(wave, min_len):
    """maximal runs of samples == 0 with at least min_len samples, [(start, end)] ascending; one pass, sample by sample"""
    out, start = [], None
    for n, v in enumerate(np.asarray(wave).tolist() + [1.0]):
        if v == 0:
            start = n if start is None else start
        else:
            if start is not None and n - start >= min_len:
                out.append((start, n))
            start = None
    return out


ZERO_RUN_CASES = {}


def _case(name, L, zeros, min_len):
    x = np.random.default_rng(len(ZERO_RUN_CASES)).uniform(0.1, 1.0, L).astype(np.float32)
    for a, b in zeros:
        x[a:b] = 0.0
    ZERO_RUN_CASES[name] = (x, min_len)


_case("touches_both_ends", 3000, [(0, 200), (2800, 3000)], 160)
_case("one_short_of_min_len", 3000, [(100, 259), (1000, 1160)], 160)
_case("split_by_one_sample", 3000, [(500, 700), (701, 900)], 160)
# L = 2 chunks + 1: a run one sample into each neighbour of a chunk boundary, a run over a whole chunk and its neighbours'
# edges, a run that is exactly the last sample's chunk
_case("straddles_chunks", 2 * CHUNK + 1, [(CHUNK - 1, CHUNK + 1), (2 * CHUNK - 300, 2 * CHUNK + 1)], 2)
_case("whole_chunk_and_edges", 3 * CHUNK + 1, [(CHUNK - 1, 2 * CHUNK + 1), (3 * CHUNK - 1, 3 * CHUNK + 1)], 2)
_case("all_zero", 2 * CHUNK + 1, [(0, 2 * CHUNK + 1)], 160)
_case("no_zero", 1000, [], 1)
_case("many_short_runs", CHUNK + 1, [(a, a + 3) for a in range(1, CHUNK - 4, 7)], 3)
_case("negative_zero", 600, [(100, 300)], 160)
ZERO_RUN_CASES["negative_zero"][0][100:300:2] = -0.0
