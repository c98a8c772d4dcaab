// Whole-recording restoration for gfx950 (nppc_audio/inpainting/restore.py; specification
// tests/restore_ref.py): the kernels around the nets when the input is a recording with gaps rather than a cut crop.
//   nppc_rec_gain      known-sample RMS -> dBFS gain in fp64: a fixed grid of partials, one folding workgroup (the pattern of
//                      masked_mse.hip); the sample mask is the gap interval list, never an [L] tensor
//   nppc_rec_windows   one workgroup per window: gather * gain, zero inside the gaps, the window's sample mask
//   nppc_rec_splice    V copies of the recording with the owned gap of every window replaced and crossfaded, one launch
//   nppc_zero_runs     maximal runs of exact zeros: per-chunk head / tail / interior summaries, then one stitching workgroup
// Gaps are long [G][2] half-open intervals, sorted and disjoint; a thread finds its gap by binary search.  Plain vector
// loads and stores, integer LDS atomics only, every sum in a fixed order: two runs give identical bits.
#include "common.h"
#include "nppc_hip.h"

namespace {

constexpr int REC_BLOCKS = NPPC_REC_GAIN_WORK;
constexpr int ZR_CHUNK = NPPC_ZERO_RUN_CHUNK;
constexpr int ZR_PER = ZR_CHUNK / 256;
static_assert(REC_BLOCKS == 256, "the folding workgroup reads one partial per thread");

// the first interval with end + pad > n (ends ascend, so this is a lower bound); G when there is none
__device__ __forceinline__ int first_end_after(const long* __restrict__ iv, int G, long n, long pad) {
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (iv[2 * mid + 1] + pad > n) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ bool in_gap(const long* __restrict__ iv, int G, long n) {
  const int g = first_end_after(iv, G, n, 0);
  return g < G && iv[2 * g] <= n;
}

// ---------------------------------------------------------------------------------------------------------------- gain
__global__ __launch_bounds__(256) void rec_gain_part_kernel(const float* __restrict__ wave, long L,
                                                            const long* __restrict__ gaps, int G, double* __restrict__ work) {
  __shared__ double red[256];
  const bool aligned = (reinterpret_cast<uintptr_t>(wave) & 15) == 0;
  const long nvec = L >> 2;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nvec; q += (long)REC_BLOCKS * 256) {
    const long i0 = q * 4;
    float x[4];
    if (aligned) {
      const float4 v = *reinterpret_cast<const float4*>(wave + i0);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = wave[i0 + k];
    }
    int g = first_end_after(gaps, G, i0, 0);
    const bool clear = g >= G || gaps[2 * g] >= i0 + 4;          // no gap touches these four samples
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool known = true;
      if (!clear) {
        const long n = i0 + k;
        while (g < G && gaps[2 * g + 1] <= n) ++g;
        known = !(g < G && gaps[2 * g] <= n);
      }
      if (known) acc += (double)x[k] * (double)x[k];
    }
  }
  if (blockIdx.x == 0) {                                         // the up to three samples past the last whole group
    const long n = nvec * 4 + threadIdx.x;
    if (threadIdx.x < 4 && n < L && !in_gap(gaps, G, n)) acc += (double)wave[n] * (double)wave[n];
  }
  acc = block_sum_tree256(acc, red);
  if (threadIdx.x == 0) work[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void rec_gain_finish_kernel(const double* __restrict__ work, long L,
                                                              const long* __restrict__ gaps, int G, float target_dbfs,
                                                              double* __restrict__ gain) {
  __shared__ double red[256];
  const double sum = block_sum_tree256(work[threadIdx.x], red);
  if (threadIdx.x == 0) {
    long known = L;
    for (int g = 0; g < G; ++g) known -= gaps[2 * g + 1] - gaps[2 * g];
    const double rms = known > 0 ? sqrt(sum / (double)known) : 0.0;
    gain[0] = pow(10.0, ((double)target_dbfs - 20.0 * log10(rms + 1e-8)) / 20.0);
  }
}

// ------------------------------------------------------------------------------------------------------------- windows
__global__ __launch_bounds__(256) void rec_windows_kernel(const float* __restrict__ wave, long L, const long* __restrict__ gaps,
                                                          int G, const long* __restrict__ win_start, int win_len,
                                                          const double* __restrict__ gain, float* __restrict__ out,
                                                          float* __restrict__ mask) {
  const int w = blockIdx.x;
  const long ws = win_start[w];
  const double g = gain[0];
  float* o = out + (size_t)w * win_len;
  float* m = mask + (size_t)w * win_len;
  for (int j = threadIdx.x; j < win_len; j += 256) {
    const long n = ws + j;
    const bool known = n >= 0 && n < L && !in_gap(gaps, G, n);
    o[j] = known ? (float)((double)wave[n] * g) : 0.f;
    m[j] = known ? 1.f : 0.f;
  }
}

// -------------------------------------------------------------------------------------------------------------- splice
struct SpliceArgs {
  const float* wave;
  const long* gaps;
  const long* win_start;
  const float* wout;
  const double* gain;
  float* out;
  long L, w_stride, v_stride;
  int G, win_len, xf;
};

// sample n of output v; g = a gap index at or before the one whose padded range could hold n (advanced here)
__device__ __forceinline__ float splice_sample(const SpliceArgs& a, long n, float rec, int& g, int v, double gain) {
  while (g < a.G && a.gaps[2 * g + 1] + a.xf <= n) ++g;
  if (g >= a.G) return rec;
  const long s = a.gaps[2 * g], e = a.gaps[2 * g + 1];
  if (n < s - a.xf) return rec;
  const long j = n - a.win_start[g];
  if (j < 0 || j >= a.win_len) return rec;                       // a crossfade that leaves the window: the recording stays
  const double y = (double)a.wout[(size_t)g * a.w_stride + (size_t)v * a.v_stride + j] / gain;
  if (n >= s && n < e) return (float)y;
  const long t = n < s ? n - (s - a.xf) : e + a.xf - 1 - n;      // 0 at the outer end of the ramp, xf - 1 next to the gap
  const double c = 0.5 - 0.5 * cos(M_PI * (double)(t + 1) / (double)(a.xf + 1));
  return (float)((double)rec + c * (y - (double)rec));           // the blend in fp64, rounded once
}

template <bool VEC>
__global__ __launch_bounds__(256) void rec_splice_kernel(SpliceArgs a) {
  const int v = blockIdx.y;
  const double gain = a.gain[0];
  float* o = a.out + (size_t)v * a.L;
  const long stride = (long)gridDim.x * 256;
  if (VEC) {                                                     // L % 4 == 0 and both bases 16-byte aligned
    const long nvec = a.L >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nvec; q += stride) {
      const long i0 = q * 4;
      float4 r = *reinterpret_cast<const float4*>(a.wave + i0);
      int g = first_end_after(a.gaps, a.G, i0, a.xf);
      if (g < a.G && a.gaps[2 * g] - a.xf < i0 + 4) {
        r.x = splice_sample(a, i0, r.x, g, v, gain);
        r.y = splice_sample(a, i0 + 1, r.y, g, v, gain);
        r.z = splice_sample(a, i0 + 2, r.z, g, v, gain);
        r.w = splice_sample(a, i0 + 3, r.w, g, v, gain);
      }
      *reinterpret_cast<float4*>(o + i0) = r;
    }
  } else {
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < a.L; n += stride) {
      int g = first_end_after(a.gaps, a.G, n, a.xf);
      o[n] = splice_sample(a, n, a.wave[n], g, v, gain);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- zero runs
// phase 1, one workgroup per chunk: summ[c] = (head, tail, n_interior, len) with head / tail the zero prefix / suffix of the
// chunk (both = len for an all-zero chunk) and ilist[c][k] the interior runs (touching neither edge) of at least min_len
// samples, in ascending order.  A sample past L counts as non-zero.
__global__ __launch_bounds__(256) void zero_runs_chunk_kernel(const float* __restrict__ wave, long L, long min_len, int icap,
                                                              long* __restrict__ summ, long* __restrict__ ilist) {
  __shared__ unsigned char z[ZR_CHUNK];
  __shared__ int scan[256];
  __shared__ int first_nz, last_nz;
  const int c = blockIdx.x, tid = threadIdx.x;
  const long base = (long)c * ZR_CHUNK;
  const int len = (int)(L - base < ZR_CHUNK ? L - base : ZR_CHUNK);
  for (int i = tid; i < ZR_CHUNK; i += 256) z[i] = (i < len && wave[base + i] == 0.f) ? 1 : 0;
  if (tid == 0) first_nz = len, last_nz = -1;
  __syncthreads();
  int lo = len, hi = -1;
  for (int k = 0; k < ZR_PER; ++k) {
    const int i = tid * ZR_PER + k;
    if (i < len && !z[i]) {
      lo = i < lo ? i : lo;
      hi = i;
    }
  }
  if (hi >= 0) {
    atomicMin(&first_nz, lo);
    atomicMax(&last_nz, hi);
  }
  // interior runs that START in this thread's samples: counted, scanned, then found again and written in order
  int cnt = 0;
  for (int k = 0; k < ZR_PER; ++k) {
    const int i = tid * ZR_PER + k;
    if (i >= 1 && i < len && z[i] && !z[i - 1]) {
      int j = i + 1;
      while (j < len && z[j]) ++j;
      cnt += (j < len && j - i >= min_len) ? 1 : 0;
    }
  }
  scan[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int off = scan[tid] - cnt;
  const int total = scan[255];
  for (int k = 0; k < ZR_PER; ++k) {
    const int i = tid * ZR_PER + k;
    if (i >= 1 && i < len && z[i] && !z[i - 1]) {
      int j = i + 1;
      while (j < len && z[j]) ++j;
      if (j < len && j - i >= min_len) {
        if (off < icap) {
          ilist[((size_t)c * icap + off) * 2] = base + i;
          ilist[((size_t)c * icap + off) * 2 + 1] = base + j;
        }
        ++off;
      }
    }
  }
  if (tid == 0) {
    long* s = summ + (size_t)c * 4;
    s[0] = first_nz;
    s[1] = len - 1 - last_nz;
    s[2] = total < icap ? total : icap;
    s[3] = len;
  }
}

// the runs that chunk c contributes, ascending: the run that opens at its first sample (when the chunk before does not end in
// zeros), its interior runs, the run that opens at its zero suffix; a run that reaches the end of a chunk goes on through
// all-zero chunks and ends after the zero prefix of the first chunk that is not, or at L
template <class Emit>
__device__ __forceinline__ void chunk_events(const long* __restrict__ summ, const long* __restrict__ ilist, int nchunks,
                                             int icap, long L, long min_len, int c, Emit emit) {
  const long* s = summ + (size_t)c * 4;
  const long head = s[0], tail = s[1], ni = s[2], len = s[3];
  const long start = (long)c * ZR_CHUNK;
  const bool full = head == len;
  auto run_end = [&](int d) -> long {
    while (d < nchunks && summ[(size_t)d * 4] == summ[(size_t)d * 4 + 3]) ++d;
    return d < nchunks ? (long)d * ZR_CHUNK + summ[(size_t)d * 4] : L;
  };
  if (head > 0 && (c == 0 || summ[(size_t)(c - 1) * 4 + 1] == 0)) {
    const long e = full ? run_end(c + 1) : start + head;
    if (e - start >= min_len) emit(start, e);
  }
  for (long k = 0; k < ni; ++k) emit(ilist[((size_t)c * icap + k) * 2], ilist[((size_t)c * icap + k) * 2 + 1]);
  if (!full && tail > 0) {
    const long b = start + len - tail, e = run_end(c + 1);
    if (e - b >= min_len) emit(b, e);
  }
}

// phase 2, one workgroup: thread t owns a contiguous block of chunks; counts, block scan, then writes in order
__global__ __launch_bounds__(256) void zero_runs_stitch_kernel(const long* __restrict__ summ, const long* __restrict__ ilist,
                                                               int nchunks, int icap, long L, long min_len,
                                                               long* __restrict__ runs, int cap, long* __restrict__ count) {
  __shared__ long scan[256];
  const int tid = threadIdx.x;
  const int per = (nchunks + 255) / 256;
  const int c0 = tid * per < nchunks ? tid * per : nchunks;
  const int c1 = c0 + per < nchunks ? c0 + per : nchunks;
  long cnt = 0;
  for (int c = c0; c < c1; ++c) chunk_events(summ, ilist, nchunks, icap, L, min_len, c, [&](long, long) { ++cnt; });
  scan[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const long add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  long off = scan[tid] - cnt;
  for (int c = c0; c < c1; ++c)
    chunk_events(summ, ilist, nchunks, icap, L, min_len, c, [&](long b, long e) {
      if (off < cap) runs[off * 2] = b, runs[off * 2 + 1] = e;
      ++off;
    });
  if (tid == 0) count[0] = scan[255];
}

}  // namespace

extern "C" {

int nppc_rec_gain(const float* wave, long L, const long* gaps, int G, float target_dbfs, double* work, double* gain,
                  void* stream) {
  if (!wave || !work || !gain || L <= 0 || G < 0 || (G > 0 && !gaps)) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rec_gain_part_kernel, dim3(REC_BLOCKS), dim3(256), 0, s, wave, L, gaps, G, work);
  hipLaunchKernelGGL(rec_gain_finish_kernel, dim3(1), dim3(256), 0, s, work, L, gaps, G, target_dbfs, gain);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_rec_windows(const float* wave, long L, const long* gaps, int G, const long* win_start, int W, int win_len,
                     const double* gain, float* out, float* mask, void* stream) {
  if (!wave || !gaps || !win_start || !gain || !out || !mask || L <= 0 || G <= 0 || W <= 0 || win_len <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(rec_windows_kernel, dim3(W), dim3(256), 0, (hipStream_t)stream, wave, L, gaps, G, win_start, win_len, gain,
                     out, mask);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_rec_splice(const float* wave, long L, const long* gaps, const long* win_start, int G, const float* wout,
                    long w_stride, long v_stride, int win_len, int V, int xf, const double* gain, float* out, void* stream) {
  if (!wave || !gaps || !win_start || !wout || !gain || !out || L <= 0 || G <= 0 || win_len <= 0 || V <= 0 || xf < 0 ||
      w_stride < 0 || v_stride < 0)
    return NPPC_EBADARG;
  if (V > 65535) return NPPC_EUNSUPPORTED;
  SpliceArgs a{wave, gaps, win_start, wout, gain, out, L, w_stride, v_stride, G, win_len, xf};
  const bool vec = (L & 3) == 0 && ((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const long items = vec ? L >> 2 : L;
  const long blocks = (items + 255) / 256;
  const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)V);
  if (vec) hipLaunchKernelGGL(rec_splice_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rec_splice_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_zero_runs(const float* wave, long L, long min_len, long* work, long work_elems, long* runs, int cap, long* count,
                   void* stream) {
  if (!wave || !work || !count || L <= 0 || min_len < 1 || cap < 0 || (cap > 0 && !runs)) return NPPC_EBADARG;
  const long nchunks = (L + ZR_CHUNK - 1) / ZR_CHUNK;
  if (nchunks >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const long icap = ZR_CHUNK / (min_len + 1) + 1;
  if (work_elems < nchunks * (4 + 2 * icap)) return NPPC_EBADARG;
  long* summ = work;
  long* ilist = work + nchunks * 4;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_runs_chunk_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, wave, L, min_len, (int)icap, summ, ilist);
  hipLaunchKernelGGL(zero_runs_stitch_kernel, dim3(1), dim3(256), 0, s, summ, ilist, (int)nchunks, (int)icap, L, min_len, runs,
                     cap, count);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
