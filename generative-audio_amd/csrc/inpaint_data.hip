// Inpainting batch assembly on the device (dataset/audio_dataset_inpainting.py __getitem__ :253-293): the crop of a
// device-resident corpus, the file's dBFS gain, an energy voice-activity detector and the gap draw of _create_mask
// (:183-221) / _create_random_mask (:170-181).  Plain HIP for gfx950, wave64, no atomics, no host synchronisation.
// The specification is tests/vad_ref.py (fp64 NumPy); the detector is NOT silero-vad.
//
// One workgroup of 256 threads per item:
//   1. copy:      clean[b][i] = corpus[offset + crop + i] * gain, one coalesced dword per lane, each sample read once; a wave
//                 owns whole windows (w = wave, wave + 4, ...), a lane sums the squares of its samples in fp64 in index order,
//                 the wave butterfly adds the 64 partial sums, lane 0 stores e_w = 10 log10(sum / win + 1e-12) in LDS.
//   2. floor/peak a copy of the levels, padded with +inf to a power of two, is sorted in LDS (bitonic, 256 threads, several
//                 compare-exchanges per thread and stage above 512 windows): floor = sorted[floor(q (W - 1))], peak = sorted[W - 1].
//   3. segments:  thread 0 walks the windows in order (the state machine of silero's get_speech_timestamps post-processing,
//                 without speech padding) and keeps the segments of at least min_speech samples in LDS (a table of its own).
//   4. gap:       thread 0 draws the segment and the offset, or falls back to the random / fixed gap.
// Every sum has a fixed order and every draw is a function of (seed, item, epoch, purpose), so an item's result does not
// depend on what else is in the batch.
#include "common.h"
#include "nppc_hip.h"
#include "philox.h"

#define IV_THREADS 256
#define IV_MAXW 2048

// one Philox call per purpose: counter (item, epoch, 0, purpose), key = the 64-bit dataset seed, word 0
enum { IV_CROP = 0, IV_SEGMENT = 1, IV_OFFSET = 2, IV_DBFS = 3 };

struct iv_rng {
  unsigned item, epoch, k0, k1;
  __device__ __forceinline__ unsigned draw(unsigned purpose) const { return philox4x32(item, epoch, 0u, purpose, k0, k1).x; }
};

// uniform integer in [0, n] (n >= 0): the high 32 bits of u * (n + 1)
__device__ __forceinline__ int iv_uniform_int(unsigned u, int n) {
  return (int)(((unsigned long long)u * (unsigned long long)((unsigned)n + 1u)) >> 32);
}

// _create_mask :199-221 on the kept segments seg[nseg][2]; fixed_start < 0 = the random fallback of _create_random_mask
__device__ __forceinline__ int iv_gap_start(const int* seg, int nseg, int L, int missing, int fixed_start, const iv_rng& rng,
                                            int* used_fallback) {
  int start = -1;
  if (nseg > 0) {
    const int k = iv_uniform_int(rng.draw(IV_SEGMENT), nseg - 1);
    const int s0 = seg[2 * k], len = seg[2 * k + 1] - s0;
    if (len > missing) start = s0 + iv_uniform_int(rng.draw(IV_OFFSET), len - missing);
  }
  *used_fallback = start < 0;
  if (start < 0) start = fixed_start >= 0 ? fixed_start : iv_uniform_int(rng.draw(IV_OFFSET), L - missing);
  return start;
}

struct iv_args {
  const float* corpus;
  long corpus_len;
  const long* offsets;      // [n_files + 1]
  const float* gains;       // [n_files]
  int n_files;
  const int* file_index;    // [B]
  const int* item_index;    // [B]
  int L, win, missing, fixed_start, use_vad, random_crop;
  unsigned k0, k1, epoch;
  float dbfs_float;
  double on_db, range_db, hyst_db, floor_q;
  int min_silence, s_max;
  float* clean;             // [B][L], nullable
  int* crop_start;          // [B], nullable
  int* gap_start;           // [B]
  int* gap_end;             // [B]
  int* segments;            // [B][s_max][2], -1 past n_segments[b]
  int* n_segments;          // [B]
  int* used_fallback;       // [B]
};

__global__ __launch_bounds__(IV_THREADS) void inpaint_vad_batch_kernel(iv_args p) {
  __shared__ double lev[IV_MAXW];
  __shared__ double srt[IV_MAXW];          // the sorted copy
  __shared__ int seg[IV_MAXW];             // the kept segments as (start, end) pairs: s_max <= IV_MAXW / 2
  __shared__ int bc[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = p.L, win = p.win, W = L / win;
  int* segs = p.segments + (size_t)b * p.s_max * 2;
  const int fi = p.file_index[b];
  long off = 0, flen = 0;
  bool ok = fi >= 0 && fi < p.n_files;
  if (ok) {
    off = p.offsets[fi];
    flen = p.offsets[fi + 1] - off;
    ok = off >= 0 && flen >= L && off + flen <= p.corpus_len;
  }
  if (!ok) {                                // an index the host should have refused: nothing is read, the item is marked
    if (p.clean)
      for (int i = tid; i < L; i += IV_THREADS) p.clean[(size_t)b * L + i] = 0.f;
    for (int i = tid; i < 2 * p.s_max; i += IV_THREADS) segs[i] = -1;
    if (tid == 0) {
      if (p.crop_start) p.crop_start[b] = 0;
      p.gap_start[b] = 0;
      p.gap_end[b] = 0;
      p.n_segments[b] = 0;
      p.used_fallback[b] = -1;
    }
    return;
  }
  const iv_rng rng{(unsigned)p.item_index[b], p.epoch, p.k0, p.k1};
  const int crop = (flen > L && p.random_crop) ? iv_uniform_int(rng.draw(IV_CROP), (int)(flen - L)) : 0;
  float gain = p.gains[fi];
  if (p.dbfs_float > 0.f) {                 // _normalize_audio :156-160: the level is uniform in target +- floating value
    const double u = (double)rng.draw(IV_DBFS) * (1.0 / 4294967296.0);
    gain *= (float)pow(10.0, (double)p.dbfs_float * (2.0 * u - 1.0) / 20.0);
  }
  const float* src = p.corpus + off + crop;
  float* dst = p.clean ? p.clean + (size_t)b * L : nullptr;

  if (!p.use_vad) {
    if (dst)
      for (int i = tid; i < L; i += IV_THREADS) dst[i] = src[i] * gain;
  } else {
    for (int w = wave; w < W; w += IV_THREADS / 64) {
      const int base = w * win;
      double s = 0.0;
      for (int i = lane; i < win; i += 64) {
        const float v = src[base + i] * gain;
        if (dst) dst[base + i] = v;
        s = fma((double)v, (double)v, s);
      }
      s = wave_sum(s);
      if (lane == 0) lev[w] = 10.0 * log10(s / (double)win + 1e-12);
    }
    if (dst)
      for (int i = W * win + tid; i < L; i += IV_THREADS) dst[i] = src[i] * gain;   // the tail no window covers
  }

  int nseg = 0;
  if (p.use_vad && W > 0) {
    int n2 = 2;
    while (n2 < W) n2 <<= 1;
    __syncthreads();
    for (int i = tid; i < n2; i += IV_THREADS) srt[i] = i < W ? lev[i] : __builtin_huge_val();
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int t = tid; t < n2 / 2; t += IV_THREADS) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const bool up = (i & k) == 0;
          const double a = srt[i], c = srt[l];
          if ((a > c) == up) {
            srt[i] = c;
            srt[l] = a;
          }
        }
      }
    __syncthreads();
    if (tid == 0) {
      int qi = (int)floor(p.floor_q * (double)(W - 1));
      qi = qi < 0 ? 0 : (qi > W - 1 ? W - 1 : qi);
      const double floor_db = srt[qi], peak_db = srt[W - 1];
      const double th_on = fmax(floor_db + p.on_db, peak_db - p.range_db), th_off = th_on - p.hyst_db;
      if (!(peak_db - floor_db < p.on_db)) {
        const int min_speech = p.missing;
        bool trig = false;
        int start = 0, temp_end = -1;
        for (int w = 0; w < W; ++w) {
          const double e = lev[w];
          const int pos = w * win;
          if (!trig) {
            if (e >= th_on) {
              trig = true;
              start = pos;
              temp_end = -1;
            }
          } else if (e < th_off) {
            if (temp_end < 0) temp_end = pos;
            if (pos - temp_end >= p.min_silence) {
              if (temp_end - start >= min_speech && nseg < p.s_max) {
                seg[2 * nseg] = start;
                seg[2 * nseg + 1] = temp_end;
                ++nseg;
              }
              trig = false;
              temp_end = -1;
            }
          } else if (e >= th_on && temp_end >= 0) {
            temp_end = -1;
          }
        }
        if (trig) {
          const int end = temp_end >= 0 ? temp_end : W * win;
          if (end - start >= min_speech && nseg < p.s_max) {
            seg[2 * nseg] = start;
            seg[2 * nseg + 1] = end;
            ++nseg;
          }
        }
      }
      bc[0] = nseg;
    }
    __syncthreads();
    nseg = bc[0];
  }
  for (int i = tid; i < 2 * p.s_max; i += IV_THREADS) segs[i] = i < 2 * nseg ? seg[i] : -1;
  if (tid == 0) {
    int fb;
    const int g0 = iv_gap_start(seg, nseg, L, p.missing, p.fixed_start, rng, &fb);
    if (p.crop_start) p.crop_start[b] = crop;
    p.gap_start[b] = g0;
    p.gap_end[b] = g0 + p.missing;
    p.n_segments[b] = nseg;
    p.used_fallback[b] = fb;
  }
}

// the gap draw alone, on given segments: one thread per item
__global__ __launch_bounds__(64) void inpaint_draw_gaps_kernel(const int* __restrict__ segments, const int* __restrict__ n_segments,
                                                               const int* __restrict__ item_index, int B, int L, int missing,
                                                               int fixed_start, int s_max, unsigned k0, unsigned k1,
                                                               unsigned epoch, int* __restrict__ gap_start,
                                                               int* __restrict__ gap_end, int* __restrict__ used_fallback) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int nseg = n_segments[b];
  nseg = nseg < 0 ? 0 : (nseg > s_max ? s_max : nseg);
  const iv_rng rng{(unsigned)item_index[b], epoch, k0, k1};
  int fb;
  const int g0 = iv_gap_start(segments + (size_t)b * s_max * 2, nseg, L, missing, fixed_start, rng, &fb);
  gap_start[b] = g0;
  gap_end[b] = g0 + missing;
  used_fallback[b] = fb;
}

extern "C" {

int nppc_inpaint_vad_batch(const float* corpus, long corpus_len, const long* offsets, const float* gains, int n_files,
                           const int* file_index, const int* item_index, int B, int L, int win, int missing, int fixed_start,
                           int use_vad, int random_crop, long seed, int epoch, float dbfs_float, double on_db, double range_db,
                           double hysteresis_db, double floor_percentile, int min_silence, int s_max, float* clean,
                           int* crop_start, int* gap_start, int* gap_end, int* segments, int* n_segments, int* used_fallback,
                           void* stream) {
  if (!corpus || !offsets || !gains || !file_index || !item_index || !gap_start || !gap_end || !segments || !n_segments ||
      !used_fallback)
    return NPPC_EBADARG;
  if (corpus_len <= 0 || n_files <= 0 || B <= 0 || L <= 0 || win < 64 || win % 64 || missing <= 0 || missing > L ||
      min_silence < 0 || s_max < 1 || !(floor_percentile >= 0.0 && floor_percentile <= 1.0))
    return NPPC_EBADARG;
  if (fixed_start >= 0 && (long)fixed_start + missing > L) return NPPC_EBADARG;
  if ((use_vad && L / win > IV_MAXW) || s_max > IV_MAXW / 2) return NPPC_EUNSUPPORTED;
  if (use_vad && 2 * s_max < L / win) return NPPC_EBADARG;       // a segment takes at least two windows (itself and its end)
  iv_args p;
  p.corpus = corpus; p.corpus_len = corpus_len; p.offsets = offsets; p.gains = gains; p.n_files = n_files;
  p.file_index = file_index; p.item_index = item_index;
  p.L = L; p.win = win; p.missing = missing; p.fixed_start = fixed_start; p.use_vad = use_vad; p.random_crop = random_crop;
  p.k0 = (unsigned)((unsigned long long)seed & 0xffffffffull); p.k1 = (unsigned)((unsigned long long)seed >> 32);
  p.epoch = (unsigned)epoch; p.dbfs_float = dbfs_float;
  p.on_db = on_db; p.range_db = range_db; p.hyst_db = hysteresis_db; p.floor_q = floor_percentile;
  p.min_silence = min_silence; p.s_max = s_max;
  p.clean = clean; p.crop_start = crop_start; p.gap_start = gap_start; p.gap_end = gap_end; p.segments = segments;
  p.n_segments = n_segments; p.used_fallback = used_fallback;
  hipLaunchKernelGGL(inpaint_vad_batch_kernel, dim3(B), dim3(IV_THREADS), 0, (hipStream_t)stream, p);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_inpaint_draw_gaps(const int* segments, const int* n_segments, const int* item_index, int B, int L, int missing,
                           int fixed_start, int s_max, long seed, int epoch, int* gap_start, int* gap_end, int* used_fallback,
                           void* stream) {
  if (!segments || !n_segments || !item_index || !gap_start || !gap_end || !used_fallback) return NPPC_EBADARG;
  if (B <= 0 || L <= 0 || missing <= 0 || missing > L || s_max < 1) return NPPC_EBADARG;
  if (fixed_start >= 0 && (long)fixed_start + missing > L) return NPPC_EBADARG;
  hipLaunchKernelGGL(inpaint_draw_gaps_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, segments, n_segments,
                     item_index, B, L, missing, fixed_start, s_max, (unsigned)((unsigned long long)seed & 0xffffffffull),
                     (unsigned)((unsigned long long)seed >> 32), (unsigned)epoch, gap_start, gap_end, used_fallback);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
