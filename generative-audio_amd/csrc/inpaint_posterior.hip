// Posterior samples of inpainted gaps (nppc_audio/inpainting/posterior.py; specification
// tests/inpaint_posterior_ref.py).
//
// The rule.  The inpainting direction net ends in a Gram-Schmidt step: its K directions w_k are orthogonal, un-normalised
// (their norms are the predicted spread) and zero on known frames, in the normalised log-magnitude domain where the loss is
// defined.  The distribution it states is x = pred + sum_k z_k w_k with z_k ~ N(0, 1) real.  pred [B][F][T], w [B][K][F][T],
// z [B][S][K], mean / sd device scalars.  Sample s of item b, bin o = (f, t), in fp64, k ascending:
//   x = (double)pred[b][o];  for k: x = x + (double)z[b][s][k] * (double)w[b][k][o]
//   mag = exp(x * sd + mean)
// The product of two fp32 values is exact in fp64, so the first line gives the same x fused or not; the second line is
// spelled fma(x, sd, mean) here and in gl_init_bin's third source (gl_gap_common.h), which is what pc_variation_kernel and
// gl_init_bin's alpha source compile to.  At z[b][s] = alpha e_k (w finite) x is pred + alpha w_k: the expression and the
// bits of those two, with no 1e-6 subtraction.  The clean-phase spectrum of a sample is (float)(mag ur), (float)(mag ui)
// with u the fp64 unit phasor of clean_spec, angle(0) = 0 and the signed-zero cases as pc_variation_kernel has them.
//
// nppc_inp_post_sample.  One workgroup = IS_S output samples of one item (blockIdx.x, blockIdx.y) and one tile of
// consecutive samples s (blockIdx.z), run one after the other through the one frame buffer.  Staged path: pred, the K
// direction rows and the unit phasor of the <= nfr frames that cover the block are read (and the phasor's square root and
// two divisions done) once per tile and kept in LDS; fallback path (the planes do not fit NPPC_INP_POST_LDS_STAGE): they
// are re-read and the phasor recomputed per sample, as pc_variation_kernel does per variation.  The gather is the shared
// direct fp64 DFT of istft_any_core.h.  The magnitude statistics need no transform and cover every frame, reached by a kept
// sample or not, so they have a kernel of their own (one thread per bin, the same tiles).
#include "common.h"
#include "istft_any_core.h"
#include "nppc_hip.h"
#include "post_stats.h"

namespace {

using namespace nppc_isany;

struct InpPostArgs {
  const float* pred;
  const float* pc;
  const float* clean;          // [B][2][F][T], null for the magnitude kernel
  const float* mean;
  const float* sd;
  const float* z;
  float* samples;              // [B][S][L] or null
  double2* tpart;              // [tiles][B][L] (sum y, sum y^2) or null
  double2* mpart;              // [tiles][B][F][T] (sum mag, sum mag^2) or null
  int K, S, spt;
};

// fp64 unit phasor of (xr, xi).  angle(0 + 0i) = 0; atan2 of signed zeros: a real part of -0 gives +-pi, i.e. (-1, 0)
__device__ __forceinline__ double2 unit_phasor(float re, float im) {
  const double xr = (double)re, xi = (double)im;
  const double h = sqrt(xr * xr + xi * xi);
  const double ur = h > 0.0 ? xr / h : (signbit(xr) ? -1.0 : 1.0), ui = h > 0.0 ? xi / h : 0.0;
  return make_double2(ur, ui);
}

// the rule: w_k at w[k * stride]
__device__ __forceinline__ double post_mag(float pred, const float* w, size_t stride, const float* __restrict__ z, int K,
                                           double sd, double mean) {
  double x = (double)pred;
  for (int k = 0; k < K; ++k) x = __builtin_fma((double)z[k], (double)w[k * stride], x);
  return exp(__builtin_fma(x, sd, mean));
}

template <bool STAGED, bool STATS>
__global__ __launch_bounds__(IS_S) void inp_post_kernel(InpPostArgs a, IstftGeom g) {
  extern __shared__ double2 ip_lds[];
  const size_t PF = (size_t)g.nfr * g.F;                      // elements of one staged plane
  double2* tw = ip_lds;
  double2* ph = tw + g.N;                                     // [nfr][F] unit phasors (staged only)
  float2* spec = reinterpret_cast<float2*>(ph + (STAGED ? PF : 0));
  float* plane = reinterpret_cast<float*>(spec + PF);         // [K + 1][nfr][F]: pred, then the directions (staged only)
  const int tid = threadIdx.x, b = blockIdx.y, B = gridDim.y, tile = blockIdx.z;
  const int K = a.K, S = a.S;
  const int s0 = tile * a.spt, s1 = s0 + a.spt < S ? s0 + a.spt : S;
  const int o0 = blockIdx.x * IS_S, o = o0 + tid;
  const int p0 = o0 + g.N / 2;
  const int pend = (o0 + IS_S < g.Lk ? o0 + IS_S : g.Lk) + g.N / 2;
  double sy = 0.0, syy = 0.0;
  if (pend > p0) {
    int t_lo, t_hi;
    frame_range(g, p0, pend, &t_lo, &t_hi);
    dft_twiddles(tw, g.N, IS_S);
    const int nt = t_hi - t_lo + 1;
    const size_t FT = (size_t)g.F * g.T;
    const double mean = (double)*a.mean, sd = (double)*a.sd;
    const float* pb = a.pred + b * FT;
    const float* wb = a.pc + (size_t)b * K * FT;
    const float* cr = a.clean + (size_t)b * 2 * FT;
    const float* ci = cr + FT;
    if (STAGED) {
      for (int e = tid; e < nt * g.F; e += IS_S) {
        const int k = e / nt, j = e % nt;
        const size_t og = (size_t)k * g.T + t_lo + j;
        const int i = j * g.F + k;
        ph[i] = unit_phasor(cr[og], ci[og]);
        plane[i] = pb[og];
        for (int r = 0; r < K; ++r) plane[(r + 1) * PF + i] = wb[r * FT + og];
      }
    }
    for (int s = s0; s < s1; ++s) {
      const float* zs = a.z + ((size_t)b * S + s) * K;
      __syncthreads();                                        // tables and planes written / the last gather has read spec
      if (STAGED) {
        for (int i = tid; i < nt * g.F; i += IS_S) {
          const double mag = post_mag(plane[i], plane + PF + i, PF, zs, K, sd, mean);
          const double2 u = ph[i];
          spec[i] = make_float2((float)(mag * u.x), (float)(mag * u.y));
        }
      } else {
        for (int e = tid; e < nt * g.F; e += IS_S) {
          const int k = e / nt, j = e % nt;
          const size_t og = (size_t)k * g.T + t_lo + j;
          const double mag = post_mag(pb[og], wb + og, FT, zs, K, sd, mean);
          const double2 u = unit_phasor(cr[og], ci[og]);
          spec[j * g.F + k] = make_float2((float)(mag * u.x), (float)(mag * u.y));
        }
      }
      __syncthreads();
      if (o < g.L) {
        const float y = o < g.Lk ? gather_sample(g, tw, spec, t_lo, t_hi, o + g.N / 2) : 0.f;
        if (a.samples) a.samples[((size_t)b * S + s) * g.L + o] = y;
        if (STATS) {
          sy += (double)y;
          syy += (double)y * (double)y;
        }
      }
    }
  } else if (a.samples && o < g.L) {                          // wholly past the overlap-add: the zero-filled tail
    for (int s = s0; s < s1; ++s) a.samples[((size_t)b * S + s) * g.L + o] = 0.f;
  }
  if (STATS && a.tpart && o < g.L) a.tpart[((size_t)tile * B + b) * g.L + o] = make_double2(sy, syy);
}

// sum over a tile's samples of mag and mag^2, one thread per bin
__global__ __launch_bounds__(256) void inp_post_mag_kernel(InpPostArgs a, size_t FT) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y, B = gridDim.y, tile = blockIdx.z, K = a.K, S = a.S;
  if (e >= FT) return;
  const double mean = (double)*a.mean, sd = (double)*a.sd;
  const float p = a.pred[b * FT + e];
  const float* wb = a.pc + (size_t)b * K * FT + e;
  const int s0 = tile * a.spt, s1 = s0 + a.spt < S ? s0 + a.spt : S;
  double sm = 0.0, smm = 0.0;
  for (int s = s0; s < s1; ++s) {
    const double mag = post_mag(p, wb, FT, a.z + ((size_t)b * S + s) * K, K, sd, mean);
    sm += mag;
    smm = __builtin_fma(mag, mag, smm);
  }
  a.mpart[((size_t)tile * B + b) * FT + e] = make_double2(sm, smm);
}

struct InpPostShape {
  IstftGeom g;
  int tiles, spt, staged;
  size_t lds;
  long work;
};

int inp_post_shape(int B, int S, int K, int T, int nfft, int hop, int L, int stats, int flags, InpPostShape* q) {
  if (B <= 0 || B > 65535 || S < 1 || K < 0 || K > NPPC_INP_POST_MAX_K || (stats & ~3) || (flags & ~NPPC_INP_POST_NO_STAGE))
    return NPPC_EBADARG;
  if (stats && (S < 2 || S > NPPC_INP_POST_MAX_STAT_S)) return NPPC_EBADARG;
  size_t lds;
  if (istft_geom(T, nfft, hop, L, &q->g, &lds) != NPPC_OK) return NPPC_EBADARG;
  long nt = ceil_div(S, NPPC_INP_POST_TILE);
  if (stats) {                                         // partial sums cost memory per tile: only as many as fill the chip
    long fill = ceil_div((long)NPPC_INP_POST_FILL, (long)B * ceil_div(L, IS_S));
    fill = fill < 1 ? 1 : (fill > NPPC_INP_POST_MAX_STAT_TILES ? NPPC_INP_POST_MAX_STAT_TILES : fill);
    nt = nt < fill ? nt : fill;
  }
  const int per = (int)ceil_div((long)S, nt);
  nt = ceil_div((long)S, (long)per);
  if (nt > 65535) return NPPC_EBADARG;
  q->tiles = (int)nt, q->spt = per;
  const size_t PF = (size_t)q->g.nfr * q->g.F;
  const size_t staged = lds + (sizeof(double2) + sizeof(float) * (K + 1)) * PF;
  q->staged = !(flags & NPPC_INP_POST_NO_STAGE) && staged <= NPPC_INP_POST_LDS_STAGE;
  q->lds = q->staged ? staged : lds;
  q->work = 16 * nt * B * (((stats & 1) ? (long)L : 0) + ((stats & 2) ? (long)q->g.F * T : 0));
  return NPPC_OK;
}

}  // namespace

extern "C" {

int nppc_inp_post_sample_shape(int B, int S, int K, int T, int nfft, int hop, int L, int stats, int flags, int* tiles,
                               int* tile_samples, long* work_bytes, int* staged, long* lds_bytes) {
  InpPostShape q;
  const int rc = inp_post_shape(B, S, K, T, nfft, hop, L, stats, flags, &q);
  if (rc != NPPC_OK) return rc;
  if (tiles) *tiles = q.tiles;
  if (tile_samples) *tile_samples = q.spt;
  if (work_bytes) *work_bytes = q.work;
  if (staged) *staged = q.staged;
  if (lds_bytes) *lds_bytes = (long)q.lds;
  return NPPC_OK;
}

int nppc_inp_post_sample(const float* pred, const float* pc, const float* clean_spec, const float* mean_p, const float* stdev,
                         const float* z, int B, int S, int K, int T, int nfft, int hop, int L, int flags, float* samples,
                         float* mean, float* std, float* mag_mean, float* mag_std, double* work, long work_bytes, void* stream) {
  if (!pred || !clean_spec || !mean_p || !stdev || (K > 0 && (!pc || !z)) || (!mean) != (!std) || (!mag_mean) != (!mag_std))
    return NPPC_EBADARG;
  const int stats = (mean ? 1 : 0) | (mag_mean ? 2 : 0);
  if (!samples && !stats) return NPPC_EBADARG;
  InpPostShape q;
  const int rc = inp_post_shape(B, S, K, T, nfft, hop, L, stats, flags, &q);
  if (rc != NPPC_OK) return rc;
  if (stats && (!work || work_bytes < q.work || ((uintptr_t)work & 15))) return NPPC_EBADARG;
  InpPostArgs a;
  a.pred = pred, a.pc = pc, a.clean = clean_spec, a.mean = mean_p, a.sd = stdev, a.z = z, a.samples = samples;
  a.tpart = mean ? (double2*)work : nullptr;
  a.mpart = mag_mean ? (double2*)work + (mean ? (size_t)q.tiles * B * L : 0) : nullptr;
  a.K = K, a.S = S, a.spt = q.spt;
  hipStream_t st = (hipStream_t)stream;
  const size_t FT = (size_t)q.g.F * T;
  if (samples || mean) {
    const dim3 grid(ceil_div(L, IS_S), B, q.tiles);
    if (q.staged && mean)
      hipLaunchKernelGGL((inp_post_kernel<true, true>), grid, dim3(IS_S), q.lds, st, a, q.g);
    else if (q.staged)
      hipLaunchKernelGGL((inp_post_kernel<true, false>), grid, dim3(IS_S), q.lds, st, a, q.g);
    else if (mean)
      hipLaunchKernelGGL((inp_post_kernel<false, true>), grid, dim3(IS_S), q.lds, st, a, q.g);
    else
      hipLaunchKernelGGL((inp_post_kernel<false, false>), grid, dim3(IS_S), q.lds, st, a, q.g);
    NPPC_CHECK_LAUNCH();
  }
  if (mag_mean) {
    hipLaunchKernelGGL(inp_post_mag_kernel, dim3((unsigned)ceil_div((long)FT, 256L), B, q.tiles), dim3(256), 0, st, a, FT);
    NPPC_CHECK_LAUNCH();
  }
  if (mean) post_finish(a.tpart, (size_t)B * L, q.tiles, S, mean, std, st);
  if (mag_mean) post_finish(a.mpart, FT * B, q.tiles, S, mag_mean, mag_std, st);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
