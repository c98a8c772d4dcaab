// Ragged (variable-length) forward of the NPPC validation step: the pieces the ragged restorer forward of
// ragged.hip does not have.  A padded batch holds item b in frames t < T_b = frames[b] (device int[B]) of planes
// [..][F][T]; every kernel here computes for item b exactly what it computes for that item alone (B = 1, T = T_b):
//   * the raw-magnitude staging of the direction net (n_maps = 2: the sub-band source is the RAW noisy magnitude),
//   * the Gram matrices of the Gram-Schmidt step and of the NPPC loss, summed over f < F, t < T_b,
//   * the Gram-Schmidt combination, zero at t >= T_b,
//   * the compressed ground-truth cIRM, zero at t >= T_b.
// Elements at t >= T_b are never loaded.  No float or double atomics: every sum has one writer and one fixed order that
// depends on (F, T_b) alone, so an item's bits do not depend on the batch it sits in, on the padded width T, or on what
// the padding holds.  Forward only.
#include "common.h"
#include "nppc_hip.h"

namespace {

// ---------------------------------------------------------------- raw magnitude staging (spec.hip: scale_transpose_kernel)
// y[b][t][c] = x[b][c][t] for t < T_b, 0 for T_b <= t < Tp: EVERY row of the buffer is written (it is reused across calls
// of other lengths); columns F..ld-1 stay as the caller left them (zero)
template <typename TT>
__global__ __launch_bounds__(256) void rawmag_ragged_kernel(const float* __restrict__ x, TT* __restrict__ y,
                                                            const int* __restrict__ frames, int C, int Tn, int Tp, int ld) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
  const int Tb = clampi(frames[b], 0, Tn);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    float v = 0.f;
    if (c < C && t < Tb) v = x[((size_t)b * C + c) * Tn + t];
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t < Tp && c < C) y[((size_t)b * Tp + t) * ld + c] = from_f32<TT>(tile[tx][i]);
  }
}

// ---------------------------------------------------------------- Gram matrix of one vector set (gsloss.hip: gram_kernel, SAME)
// set: K vectors [B][K][2][F][T] (+ e = gt - pred, [B][2][F][T], as index K when gt is given); KV = K (+ 1).
// G[b][i][n] = sum_{f < F, t < T_b} conj(a_i) a_n, fp64 products (fp32 x fp32 is exact in fp64) and fp64 sums.
// Pass 1: workgroup (x, b) owns the GR_ROWS frequency rows f = GR_ROWS x .., one per wave; lane l adds t = l, l + 64, .. < T_b
// in that order, the wave folds its lanes with the xor tree of wave_sum, wave 0..3 are added in index order -> one partial
// [NP][2] per workgroup, NP = KV (KV + 1) / 2 (n >= i).  Pass 2: one thread per entry adds the ceil(F / GR_ROWS) partials
// of the item in index order and writes both triangles.  Every step depends on (F, T_b) only.
constexpr int GR_ROWS = 4;

template <int KV>
__global__ __launch_bounds__(256) void gram_ragged_kernel(const float* __restrict__ v, const float* __restrict__ gt,
                                                          const float* __restrict__ pred, double* __restrict__ part,
                                                          const int* __restrict__ frames, int K, int F, int T) {
  constexpr int NP = KV * (KV + 1) / 2;
  __shared__ double red[GR_ROWS][NP * 2];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * GR_ROWS + wave;
  const int Tb = clampi(frames[b], 0, T);
  const size_t N = (size_t)F * T;
  double ar[NP], ai[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) ar[i] = ai[i] = 0.0;
  if (f < F) {
    const size_t row = (size_t)f * T;
    for (int t = lane; t < Tb; t += 64) {
      float xr[KV], xi[KV];
#pragma unroll
      for (int i = 0; i < KV; ++i) {
        if (i < K) {
          const float* p = v + ((size_t)(b * K + i) * 2) * N + row + t;
          xr[i] = p[0];
          xi[i] = p[N];
        } else {
          const size_t o = (size_t)b * 2 * N + row + t;
          xr[i] = gt[o] - pred[o];
          xi[i] = gt[o + N] - pred[o + N];
        }
      }
      int p = 0;
#pragma unroll
      for (int i = 0; i < KV; ++i)
#pragma unroll
        for (int n = i; n < KV; ++n) {
          ar[p] += (double)xr[i] * (double)xr[n] + (double)xi[i] * (double)xi[n];
          ai[p] += (double)xr[i] * (double)xi[n] - (double)xi[i] * (double)xr[n];
          ++p;
        }
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const double r = wave_sum(ar[i]), m = wave_sum(ai[i]);
    if (lane == 0) { red[wave][2 * i] = r; red[wave][2 * i + 1] = m; }
  }
  __syncthreads();
  if (threadIdx.x < NP * 2) {
    const int e = threadIdx.x;
    part[((size_t)b * gridDim.x + blockIdx.x) * NP * 2 + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  }
}

template <int KV>
__global__ __launch_bounds__(64) void gram_ragged_finish_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                int nchunk) {
  constexpr int NP = KV * (KV + 1) / 2;
  const int b = blockIdx.x, p = threadIdx.x;
  if (p >= NP) return;
  const double* q = part + (size_t)b * nchunk * NP * 2 + 2 * p;
  double r = 0.0, m = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    r += q[(size_t)c * NP * 2];
    m += q[(size_t)c * NP * 2 + 1];
  }
  int i = 0, rem = p;
  for (i = 0; i < KV; ++i) {
    if (rem < KV - i) break;
    rem -= KV - i;
  }
  const int n = i + rem;
  double* o = out + (size_t)b * KV * KV * 2;
  o[(i * KV + n) * 2] = r;
  o[(i * KV + n) * 2 + 1] = n == i ? 0.0 : m;          // <a_i, a_i> is real: xr xi - xi xr cancels term by term
  if (n != i) {
    o[(n * KV + i) * 2] = r;
    o[(n * KV + i) * 2 + 1] = -m;
  }
}

// ---------------------------------------------------------------- combination (gsloss.hip: combine_kernel, one set)
// out_i[f][t] = sum_m M1[b][i][m] a_m[f][t] for t < T_b (fp64, terms in index order), 0 for T_b <= t < T.
// One workgroup per (f, b) row.
template <int KV>
__global__ __launch_bounds__(256) void combine_ragged_kernel(const float* __restrict__ v, const double* __restrict__ M1,
                                                             float* __restrict__ out, const int* __restrict__ frames, int F,
                                                             int T) {
  __shared__ double2 c1[KV * KV];
  const int b = blockIdx.y, f = blockIdx.x;
  for (int i = threadIdx.x; i < KV * KV; i += 256)
    c1[i] = make_double2(M1[((size_t)b * KV * KV + i) * 2], M1[((size_t)b * KV * KV + i) * 2 + 1]);
  __syncthreads();
  const int Tb = clampi(frames[b], 0, T);
  const size_t N = (size_t)F * T, row = (size_t)f * T;
  for (int t = threadIdx.x; t < T; t += 256) {
    float xr[KV], xi[KV];
    if (t < Tb) {
#pragma unroll
      for (int i = 0; i < KV; ++i) {
        const float* p = v + ((size_t)(b * KV + i) * 2) * N + row + t;
        xr[i] = p[0];
        xi[i] = p[N];
      }
    }
#pragma unroll
    for (int i = 0; i < KV; ++i) {
      double orr = 0.0, oi = 0.0;
      if (t < Tb) {
#pragma unroll
        for (int m = 0; m < KV; ++m) {
          const double2 c = c1[i * KV + m];
          orr += c.x * xr[m] - c.y * xi[m];
          oi += c.x * xi[m] + c.y * xr[m];
        }
      }
      float* p = out + ((size_t)(b * KV + i) * 2) * N + row + t;
      p[0] = (float)orr;
      p[N] = (float)oi;
    }
  }
}

// ---------------------------------------------------------------- ground-truth cIRM (frontend.hip: cirm_build_kernel, G = 1)
// gt[b][{0,1}][f][t] = compress(cIRM(noisy, clean)) for t < T_b, 0 for T_b <= t < T (no drop-band)
__global__ __launch_bounds__(256) void cirm_build_ragged_kernel(const float* __restrict__ nr, const float* __restrict__ ni,
                                                                const float* __restrict__ cr, const float* __restrict__ ci,
                                                                float* __restrict__ out, const int* __restrict__ frames, int B,
                                                                int F, int T, float eps) {
  const size_t total = (size_t)B * F * T, FT = (size_t)F * T;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int t = (int)(e % T);
    const int b = (int)(e / FT);
    const size_t o = (size_t)b * 2 * FT + (e - (size_t)b * FT);
    float gr = 0.f, gi = 0.f;
    if (t < clampi(frames[b], 0, T)) {
      const float a = nr[e], bb = ni[e], c = cr[e], d = ci[e];
      const float den = a * a + bb * bb + eps;
      gr = compress_cirm((a * c + bb * d) / den);
      gi = compress_cirm((a * d - bb * c) / den);
    }
    out[o] = gr;
    out[o + FT] = gi;
  }
}

#define KV_SWITCH(KVv, CALL)                        \
  switch (KVv) {                                    \
    case 1: { constexpr int KVc = 1; CALL; } break; \
    case 2: { constexpr int KVc = 2; CALL; } break; \
    case 3: { constexpr int KVc = 3; CALL; } break; \
    case 4: { constexpr int KVc = 4; CALL; } break; \
    case 5: { constexpr int KVc = 5; CALL; } break; \
    case 6: { constexpr int KVc = 6; CALL; } break; \
    case 7: { constexpr int KVc = 7; CALL; } break; \
    case 8: { constexpr int KVc = 8; CALL; } break; \
    case 9: { constexpr int KVc = 9; CALL; } break; \
    default: return NPPC_EUNSUPPORTED;              \
  }

template <int KV>
static void launch_gram_ragged(const float* a, const float* gt, const float* pred, double* out, double* work,
                               const int* frames, int B, int K, int F, int T, hipStream_t s) {
  const int nchunk = ceil_div(F, GR_ROWS);
  hipLaunchKernelGGL(gram_ragged_kernel<KV>, dim3(nchunk, B), dim3(256), 0, s, a, gt, pred, work, frames, K, F, T);
  hipLaunchKernelGGL(gram_ragged_finish_kernel<KV>, dim3(B), dim3(64), 0, s, work, out, nchunk);
}

static long gram_ragged_work(int B, int KV, int F) { return (long)B * ceil_div(F, GR_ROWS) * (KV * (KV + 1) / 2) * 2; }

}  // namespace

extern "C" {

int nppc_rawmag_stage_ragged(int prec, const float* x, void* y, const int* frames, int B, int F, int T, int Tp, int ld,
                             void* stream) {
  if (!x || !y || !frames || B <= 0 || F <= 0 || T <= 0 || T > Tp || F > ld) return NPPC_EBADARG;
  dim3 grid(ceil_div(Tp, 32), ceil_div(F, 32), B);
  hipStream_t s = (hipStream_t)stream;
  if (prec == NPPC_PREC_BF16)
    hipLaunchKernelGGL(rawmag_ragged_kernel<bf16_t>, grid, dim3(256), 0, s, x, (bf16_t*)y, frames, F, T, Tp, ld);
  else if (prec == NPPC_PREC_F32)
    hipLaunchKernelGGL(rawmag_ragged_kernel<float>, grid, dim3(256), 0, s, x, (float*)y, frames, F, T, Tp, ld);
  else
    return NPPC_EBADARG;
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gram_ragged_work_elems(int B, int K, int with_e, int F, long* n) {
  if (!n || B <= 0 || K < 1 || F <= 0) return NPPC_EBADARG;
  *n = gram_ragged_work(B, K + (with_e ? 1 : 0), F);
  return NPPC_OK;
}

int nppc_gram_ragged(const float* a, const float* gt, const float* pred, double* out, double* work, long work_elems,
                     const int* frames, int B, int K, int F, int T, void* stream) {
  if (!a || !out || !work || !frames || B <= 0 || K < 1 || F <= 0 || T <= 0 || (gt == nullptr) != (pred == nullptr))
    return NPPC_EBADARG;
  const int KV = K + (gt ? 1 : 0);
  if (KV > 9) return NPPC_EUNSUPPORTED;
  if (work_elems < gram_ragged_work(B, KV, F)) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  KV_SWITCH(KV, launch_gram_ragged<KVc>(a, gt, pred, out, work, frames, B, K, F, T, s));
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_combine_ragged(const float* a, const double* M1, float* out, const int* frames, int B, int K, int F, int T,
                        void* stream) {
  if (!a || !M1 || !out || !frames || B <= 0 || K < 1 || F <= 0 || T <= 0) return NPPC_EBADARG;
  if (K > 8) return NPPC_EUNSUPPORTED;      // what nppc_gram_ragged takes with e (KV = K + 1 <= 9)
  hipStream_t s = (hipStream_t)stream;
  KV_SWITCH(K, hipLaunchKernelGGL(combine_ragged_kernel<KVc>, dim3(F, B), dim3(256), 0, s, a, M1, out, frames, F, T));
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_cirm_build_compress_ragged(const float* nr, const float* ni, const float* cr, const float* ci, float* out,
                                    const int* frames, int B, int F, int T, float eps, void* stream) {
  if (!nr || !ni || !cr || !ci || !out || !frames || B <= 0 || F <= 0 || T <= 0) return NPPC_EBADARG;
  const size_t total = (size_t)B * F * T;
  const int grid = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
  hipLaunchKernelGGL(cirm_build_ragged_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, nr, ni, cr, ci, out, frames, B, F,
                     T, eps);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
