// Whole-recording enhancement for gfx950 (nppc_audio/enhance.py; the rule: csrc/enhance_core.h;
// specification tests/enhance_ref.py): what stands between the direction net and a spliced recording when a recording is
// enhanced chunk by chunk.
//   nppc_enh_gram     grid (S, n - 1): workgroup (s, c - 1) takes samples [s seg, (s + 1) seg) of boundary c's H, stages
//                     tiles of its 2 K rows in LDS and accumulates its share of the K (K + 2) sums in fp64
//   nppc_enh_chain    one workgroup: folds the S partials of every boundary in index order, then walks the boundaries serially
//   nppc_enh_splice   one workgroup per tile of 1024 output samples, all 1 + K A rows: e and every p row of the (at most
//                     two) chunks under a lane's four samples are read once and serve every alpha
// No atomics, every sum in a fixed order: two runs give identical bits.
#include "common.h"
#include "enhance_core.h"
#include "nppc_hip.h"

namespace {

constexpr int GT = 256;                    // samples of a Gram tile
constexpr int GLD = GT + 1;                // LDS row stride: rows a thread pair reads land in different banks
constexpr int MAX_E = ENH_MAX_K * (ENH_MAX_K + 2);
static_assert(NPPC_ENH_MAX_K == ENH_MAX_K, "header and core disagree");
static_assert(MAX_E <= 2 * 256, "a thread holds at most two accumulators");

// entry e of a boundary's sums -> the two staged rows it multiplies (rows 0 .. K - 1: a_j, K .. 2 K - 1: b_k)
__device__ __forceinline__ void entry_rows(int e, int K, int* r1, int* r2) {
  if (e < K * K) *r1 = e / K, *r2 = K + e % K;
  else if (e < K * K + K) *r1 = *r2 = e - K * K;
  else *r1 = *r2 = e - K * K;                                    // K + k: the b rows follow the a rows
}

// ---------------------------------------------------------------------------------------------------------------- gram
// Work items: E entries x G sample groups (G = max(1, 256 / E)); item w = g E + e sums entry e over the tile samples
// i = g (mod G); thread t owns items t and t + 256.  The groups are folded in index order at the end.
__global__ __launch_bounds__(256) void enh_gram_kernel(const float* __restrict__ pcs, long p_cs, long p_ks, int K, int H, int S,
                                                       double* __restrict__ work) {
  __shared__ float rows[2 * ENH_MAX_K * GLD];
  __shared__ double red[2 * 256];
  const int s = blockIdx.x, c = blockIdx.y + 1, tid = threadIdx.x;
  const int E = ENH_E(K), G = E >= 256 ? 1 : 256 / E, items = E * G;
  const int seg = (H + S - 1) / S;
  const int lo = s * seg < H ? s * seg : H, hi = lo + seg < H ? lo + seg : H;
  const float* a = pcs + (c - 1) * p_cs + H;
  const float* b = pcs + c * p_cs;
  int r1[2], r2[2], g[2];
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int w = tid + u * 256;
    g[u] = w < items ? w / E : -1;
    entry_rows(w < items ? w % E : 0, K, &r1[u], &r2[u]);
  }
  for (int t0 = lo; t0 < hi; t0 += GT) {
    const int len = hi - t0 < GT ? hi - t0 : GT;
    __syncthreads();
    for (int r = 0; r < 2 * K; ++r) {
      const float* src = r < K ? a + r * p_ks : b + (r - K) * p_ks;
      if (tid < len) rows[r * GLD + tid] = src[t0 + tid];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (g[u] < 0) continue;
      const float* x = rows + r1[u] * GLD;
      const float* y = rows + r2[u] * GLD;
      for (int i = g[u]; i < len; i += G) acc[u] += (double)x[i] * (double)y[i];
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) red[tid + u * 256] = acc[u];
  __syncthreads();
  double* out = work + ((size_t)(c - 1) * S + s) * E;
  for (int e = tid; e < E; e += 256) {
    double sum = red[e];
    for (int q = 1; q < G; ++q) sum += red[q * E + e];
    out[e] = sum;
  }
}

// --------------------------------------------------------------------------------------------------------------- chain
// Phase 1, all threads: gram[c - 1][e] = the S partials in index order.  Phase 2: thread 0 walks the boundaries while the
// others stage the next boundary's sums in the other LDS buffer, so a step costs one barrier.
__global__ __launch_bounds__(256) void enh_chain_kernel(const double* __restrict__ work, int n, int K, int S, int match,
                                                        int* __restrict__ perm, int* __restrict__ sign,
                                                        double* __restrict__ continuity, double* __restrict__ gram) {
  __shared__ double g[2][MAX_E];
  __shared__ double cont[2][ENH_MAX_K];
  __shared__ int pm[2][ENH_MAX_K], sg[2][ENH_MAX_K];
  const int tid = threadIdx.x, E = ENH_E(K);
  if (tid < K) {
    pm[0][tid] = tid, sg[0][tid] = 1;
    perm[tid] = tid, sign[tid] = 1;
  }
  const long total = (long)(n - 1) * E;
  for (long q = tid; q < total; q += 256) {
    const double* p = work + (q / E) * S * E + q % E;
    double sum = p[0];
    for (int s = 1; s < S; ++s) sum += p[(size_t)s * E];
    gram[q] = sum;
  }
  __syncthreads();                                               // the block's own global writes, visible to the block
  if (n > 1)
    for (int e = tid; e < E; e += 256) g[1][e] = gram[e];
  __syncthreads();
  for (int c = 1; c < n; ++c) {
    const int was = (c - 1) & 1, now = c & 1;
    if (c + 1 < n)
      for (int e = tid; e < E; e += 256) g[was][e] = gram[(size_t)c * E + e];
    if (tid == 0) enh_chain_step(g[now], K, match, pm[was], sg[was], pm[now], sg[now], cont[now]);
    __syncthreads();
    if (tid < K) {
      perm[c * K + tid] = pm[now][tid];
      sign[c * K + tid] = sg[now][tid];
      continuity[(size_t)(c - 1) * K + tid] = cont[now][tid];
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- splice
struct SpliceArgs {
  EnhChunks q;
  const float* alphas;
  const float* w;
  const int* perm;
  const int* sign;
  float* out;
  long ldo;
  int A;
};

__device__ __forceinline__ void load4(const float* p, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[k];
  }
}

// IN4: H % 4 == 0, every chunk and direction stride a multiple of 4 and the bases 16-byte aligned: a lane's four samples sit
// in one chunk on one side of every boundary and are read with 16-byte loads.  OUT4: ldo % 4 == 0 and out 16-byte aligned.
template <bool IN4, bool OUT4>
__global__ __launch_bounds__(256) void enh_splice_kernel(SpliceArgs a) {
  const EnhChunks& q = a.q;
  const int H = q.C / 2, K = q.K, A = a.A;
  const long m0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (m0 >= q.L) return;
  const int cnt = q.L - m0 < 4 ? (int)(q.L - m0) : 4;
  int cur[4], i[4];
  bool blend[4];
  float wt[4], e_c[4], e_p[4], p_c[4], p_p[4], y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    blend[k] = enh_locate(k < cnt ? m0 + k : m0, H, q.n, &cur[k], &i[k]);      // past L: sample m0 again, never stored
    wt[k] = blend[k] ? a.w[i[k]] : 0.f;
  }
  const bool whole = IN4 && cnt == 4;                            // cur, blend equal and i consecutive over the four
  if (whole) {
    load4(q.enh + cur[0] * q.e_cs + i[0], true, e_c);
    if (blend[0]) load4(q.enh + (cur[0] - 1) * q.e_cs + i[0] + H, true, e_p);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e_c[k] = q.enh[cur[k] * q.e_cs + i[k]];
      if (blend[k]) e_p[k] = q.enh[(cur[k] - 1) * q.e_cs + i[k] + H];
    }
  }
  auto store = [&](int v) {
    float* o = a.out + (size_t)v * a.ldo + m0;
    if (OUT4 && cnt == 4) {
      *reinterpret_cast<float4*>(o) = float4{y[0], y[1], y[2], y[3]};
    } else {
      for (int k = 0; k < cnt; ++k) o[k] = y[k];
    }
  };
#pragma unroll
  for (int k = 0; k < 4; ++k) y[k] = blend[k] ? enh_blend(e_p[k], e_c[k], wt[k]) : e_c[k];
  store(0);
  if (A == 0) return;
  for (int s = 0; s < K; ++s) {
    float sc[4], sp[4];
    if (whole) {
      const int c = cur[0];
      load4(q.pcs + c * q.p_cs + enh_dir(a.perm[c * K + s], K) * q.p_ks + i[0], true, p_c);
      if (blend[0]) load4(q.pcs + (c - 1) * q.p_cs + enh_dir(a.perm[(c - 1) * K + s], K) * q.p_ks + i[0] + H, true, p_p);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cur[k];
      sc[k] = (float)a.sign[c * K + s];
      sp[k] = blend[k] ? (float)a.sign[(c - 1) * K + s] : 0.f;
      if (!whole) {
        p_c[k] = q.pcs[c * q.p_cs + enh_dir(a.perm[c * K + s], K) * q.p_ks + i[k]];
        if (blend[k]) p_p[k] = q.pcs[(c - 1) * q.p_cs + enh_dir(a.perm[(c - 1) * K + s], K) * q.p_ks + i[k] + H];
      }
    }
    for (int al = 0; al < A; ++al) {
      const float alpha = a.alphas[al];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float yc = enh_vary(e_c[k], enh_mul(alpha, sc[k]), p_c[k]);
        y[k] = blend[k] ? enh_blend(enh_vary(e_p[k], enh_mul(alpha, sp[k]), p_p[k]), yc, wt[k]) : yc;
      }
      store(1 + s * A + al);
    }
  }
}

int clamp_split(int n, int H, int split) {
  const int cap = H < NPPC_ENH_MAX_SPLIT ? H : NPPC_ENH_MAX_SPLIT;
  int S = split;
  if (S <= 0) {                                                   // two workgroups per CU, a tile or more of samples each
    const int want = (512 + (n - 2)) / (n - 1 > 0 ? n - 1 : 1);
    const int tiles = (H + GT - 1) / GT;
    S = want < tiles ? want : tiles;
  }
  return S < 1 ? 1 : (S > cap ? cap : S);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int nppc_enh_shape(int n, int K, int C, int split, int* S, long* work_bytes) {
  if (n < 1 || K < 1 || C < 2 || (C & 1) || split < 0) return NPPC_EBADARG;
  if (K > ENH_MAX_K) return NPPC_EUNSUPPORTED;
  const int s = clamp_split(n, C / 2, split);
  if (S) *S = s;
  if (work_bytes) *work_bytes = (long)sizeof(double) * (n - 1) * s * ENH_E(K);
  return NPPC_OK;
}

int nppc_enh_gram(const float* pcs, long p_cs, long p_ks, int n, int K, int C, int S, double* work, void* stream) {
  if (!pcs || !work || n < 2 || K < 1 || C < 2 || (C & 1) || p_cs < 0 || p_ks < 0) return NPPC_EBADARG;
  if (K > ENH_MAX_K) return NPPC_EUNSUPPORTED;
  if (S < 1 || S > NPPC_ENH_MAX_SPLIT || S > C / 2) return NPPC_EBADARG;
  if (n - 1 > 65535) return NPPC_EUNSUPPORTED;
  hipLaunchKernelGGL(enh_gram_kernel, dim3((unsigned)S, (unsigned)(n - 1)), dim3(256), 0, (hipStream_t)stream, pcs, p_cs, p_ks, K,
                     C / 2, S, work);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_enh_chain(const double* work, int n, int K, int S, int match, int* perm, int* sign, double* continuity, double* gram,
                   void* stream) {
  if (!perm || !sign || n < 1 || K < 1 || (match != ENH_MATCH_GREEDY && match != ENH_MATCH_SIGN)) return NPPC_EBADARG;
  if (K > ENH_MAX_K) return NPPC_EUNSUPPORTED;
  if (n > 1 && (!work || !continuity || !gram || S < 1 || S > NPPC_ENH_MAX_SPLIT)) return NPPC_EBADARG;
  hipLaunchKernelGGL(enh_chain_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, work, n, K, S, match, perm, sign, continuity,
                     gram);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

static int splice_args_ok(const float* enh, long e_cs, const float* pcs, long p_cs, long p_ks, int n, int K, int C, long L,
                          const float* alphas, int A, const float* w, const int* perm, const int* sign, const float* out,
                          long ldo) {
  if (!enh || !out || A < 0 || e_cs < 0 || p_cs < 0 || p_ks < 0 || ldo < L || K < 0) return NPPC_EBADARG;
  if (K > ENH_MAX_K) return NPPC_EUNSUPPORTED;
  if (!enh_plan_ok(n, K, C, L)) return NPPC_EBADARG;
  if (n > 1 && !w) return NPPC_EBADARG;
  if (K * A > 0 && (!pcs || !alphas || !perm || !sign)) return NPPC_EBADARG;
  return NPPC_OK;
}

int nppc_enh_splice(const float* enh, long e_cs, const float* pcs, long p_cs, long p_ks, int n, int K, int C, long L,
                    const float* alphas, int A, const float* w, const int* perm, const int* sign, float* out, long ldo,
                    void* stream) {
  const int rc = splice_args_ok(enh, e_cs, pcs, p_cs, p_ks, n, K, C, L, alphas, A, w, perm, sign, out, ldo);
  if (rc != NPPC_OK) return rc;
  const long blocks = (L + NPPC_ENH_TILE - 1) / NPPC_ENH_TILE;
  if (blocks >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const bool dirs = K * A > 0;
  SpliceArgs a{EnhChunks{enh, pcs, e_cs, p_cs, p_ks, n, dirs ? K : 0, C, L}, alphas, w, perm, sign, out, ldo, dirs ? A : 0};
  const bool in4 = (C / 2) % 4 == 0 && e_cs % 4 == 0 && aligned16(enh) &&
                   (!dirs || (p_cs % 4 == 0 && p_ks % 4 == 0 && aligned16(pcs)));
  const bool out4 = ldo % 4 == 0 && aligned16(out);
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (in4 && out4) hipLaunchKernelGGL((enh_splice_kernel<true, true>), grid, block, 0, s, a);
  else if (in4) hipLaunchKernelGGL((enh_splice_kernel<true, false>), grid, block, 0, s, a);
  else if (out4) hipLaunchKernelGGL((enh_splice_kernel<false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((enh_splice_kernel<false, false>), grid, block, 0, s, a);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_enh_chain_host(const float* pcs, long p_cs, long p_ks, int n, int K, int C, int match, int* perm, int* sign,
                        double* continuity, double* gram) {
  if (!perm || !sign || n < 1 || K < 1 || C < 2 || (C & 1) || p_cs < 0 || p_ks < 0 ||
      (match != ENH_MATCH_GREEDY && match != ENH_MATCH_SIGN))
    return NPPC_EBADARG;
  if (K > ENH_MAX_K) return NPPC_EUNSUPPORTED;
  if (n > 1 && (!pcs || !continuity)) return NPPC_EBADARG;
  enh_chain_serial(pcs, p_cs, p_ks, n, K, C, match, perm, sign, continuity, gram);
  return NPPC_OK;
}

int nppc_enh_splice_host(const float* enh, long e_cs, const float* pcs, long p_cs, long p_ks, int n, int K, int C, long L,
                         const float* alphas, int A, const float* w, const int* perm, const int* sign, float* out, long ldo) {
  const int rc = splice_args_ok(enh, e_cs, pcs, p_cs, p_ks, n, K, C, L, alphas, A, w, perm, sign, out, ldo);
  if (rc != NPPC_OK) return rc;
  const bool dirs = K * A > 0;
  enh_splice_serial(EnhChunks{enh, pcs, e_cs, p_cs, p_ks, n, dirs ? K : 0, C, L}, alphas, dirs ? A : 0, w, perm, sign, out, ldo);
  return NPPC_OK;
}

}  // extern "C"
