// BSS-eval SDR of ragged batches for gfx950 (mir_eval.separation.bss_eval_sources for one source, audio_zen/metrics.py:56-58)
// and the sums of _scale_bss_eval (audio_zen/metrics.py:8-53); the contract is DESIGN.md section 7d "BSS-eval SDR".
//
// Per item (s = reference, e = estimate, n samples, P = filter length <= 512, M = n + P - 1):
//   r[t] = sum_m s[m] s[m - t], d[t] = sum_m e[m] s[m - t]   (corr kernel: per-chunk partials, no atomics)
//   toeplitz(r) c = d                                          (solve kernel: adds the chunks in ascending order, then
//                                                               Levinson-Durbin in LDS, one workgroup per item)
//   proj[m] = sum_t c[t] s[m - t], num = sum proj^2, den = sum (e - proj)^2 over all M samples (project kernel: per-tile
//                                                               partials; finish kernel: ascending order, SDR)
// Everything after the fp32 input samples is fp64.  Which thread adds what, and in which order, depends on the item's own
// (n, P) only: a value is bit-identical alone or in any batch and from run to run.  No sample at or past an item's length
// is read.
#include "common.h"
#include "nppc_hip.h"

namespace {

constexpr int MAXP = 512;                // longest filter: the Levinson vectors and the windows are sized for it
constexpr int CORR_TILE = 1024;          // samples of m a corr workgroup stages in LDS at a time
constexpr int CORR_CHUNK = 8192;         // samples of m per corr workgroup (8 tiles): one row of partials each
constexpr int PROJ_CHUNK = 1024;         // output samples per project workgroup (4 per thread)
constexpr int PROJ_PER_THREAD = PROJ_CHUNK / 256;

// ---- correlations ------------------------------------------------------------------------------------------------------
// grid (chunk, item), 256 threads; thread tid owns lags tid and tid + 256.  Per tile the workgroup stages, as fp64,
// s[m0 - (P - 1) .. m0 + tile) (zeros before the signal and past its end) and e[m0 .. m0 + tile).  In the inner loop
// s[m] and e[m] are broadcast reads and s[m - t] is stride-1 across the lanes (ds_read_b64 of consecutive doubles: every
// bank once per 32 lanes).  part [B][nchunks][2][P]: row 0 = r, row 1 = d of this chunk.
__global__ __launch_bounds__(256) void bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                       const int* __restrict__ lengths, long ld, int P, long nchunks,
                                                       double* __restrict__ part) {
  __shared__ double sW[CORR_TILE + MAXP - 1];
  __shared__ double eW[CORR_TILE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long n = min((long)lengths[b], ld);
  const long c0 = (long)blockIdx.x * CORR_CHUNK;
  if (c0 >= n) return;                                  // uniform over the workgroup
  const long c1 = min(c0 + CORR_CHUNK, n);
  const float* s = ref + (long)b * ld;
  const float* e = est + (long)b * ld;
  const int H = P - 1;
  const int t0 = tid, t1 = tid + 256;
  const bool on0 = t0 < P, on1 = t1 < P;
  double r0 = 0.0, d0 = 0.0, r1 = 0.0, d1 = 0.0;
  for (long m0 = c0; m0 < c1; m0 += CORR_TILE) {
    const int len = (int)min((long)CORR_TILE, c1 - m0);
    __syncthreads();                                    // the previous tile has been consumed
    for (int i = tid; i < len + H; i += 256) {
      const long m = m0 - H + i;
      sW[i] = (m >= 0 && m < n) ? (double)s[m] : 0.0;
    }
    for (int i = tid; i < len; i += 256) eW[i] = (double)e[m0 + i];
    __syncthreads();
    if (on1) {
      const double* w0 = sW + (H - t0);
      const double* w1 = sW + (H - t1);
#pragma unroll 4
      for (int i = 0; i < len; ++i) {
        const double sv = sW[H + i], ev = eW[i], a = w0[i], c = w1[i];
        r0 = fma(sv, a, r0);
        d0 = fma(ev, a, d0);
        r1 = fma(sv, c, r1);
        d1 = fma(ev, c, d1);
      }
    } else if (on0) {
      const double* w0 = sW + (H - t0);
#pragma unroll 4
      for (int i = 0; i < len; ++i) {
        const double a = w0[i];
        r0 = fma(sW[H + i], a, r0);
        d0 = fma(eW[i], a, d0);
      }
    }
  }
  double* o = part + ((long)b * nchunks + blockIdx.x) * 2 * P;
  if (on0) {
    o[t0] = r0;
    o[P + t0] = d0;
  }
  if (on1) {
    o[t1] = r1;
    o[P + t1] = d1;
  }
}

// ---- Toeplitz solve ----------------------------------------------------------------------------------------------------
// one workgroup of 512 threads per item; thread j owns element j of every vector.  Prologue: r[j], d[j] = the item's
// chunk partials added in ascending chunk order.  Then Levinson-Durbin for toeplitz(r) x = d: with a = the prediction
// polynomial of order k - 1 (a[0] = 1, toeplitz_k(r) a = (E, 0, .., 0)),
//   kappa = -sum_{j<k} a[j] r[k - j] / E,  a'[j] = a[j] + kappa a[k - j] (j <= k),  E' = E (1 - kappa^2),
//   mu = (d[k] - sum_{j<k} x[j] r[k - j]) / E',  x[j] += mu a'[k - j] (j <= k).
// a[j] and x[j] live in thread j's registers; a copy of a sits in LDS (double-buffered) for the reversed reads, r and d in LDS
// for r[k - j] and d[k]; the two dot products of a step share one block reduction.  Two barriers per step.  status[b] = 1 when
// r[0] <= 0 (an all-zero reference), a prediction error E' <= 0 or anything non-finite: the item's SDR is NaN.
__global__ __launch_bounds__(MAXP) void bss_solve_kernel(const double* __restrict__ part, const int* __restrict__ lengths,
                                                         long ld, int P, long nchunks, double* __restrict__ r_out,
                                                         double* __restrict__ d_out, double* __restrict__ c_out,
                                                         int* __restrict__ status) {
  __shared__ double rL[MAXP], dL[MAXP];
  __shared__ double aL[2][MAXP];
  __shared__ double red[2][MAXP / 64];
  const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wid = j >> 6;
  const long n = min((long)lengths[b], ld);
  const long nch = (n + CORR_CHUNK - 1) / CORR_CHUNK;
  double rj = 0.0, dj = 0.0;
  if (j < P) {
    const double* p = part + (long)b * nchunks * 2 * P + j;
    for (long c = 0; c < nch; ++c) {
      rj += p[c * 2 * P];
      dj += p[c * 2 * P + P];
    }
    r_out[(long)b * P + j] = rj;
    d_out[(long)b * P + j] = dj;
  }
  rL[j] = rj;                                           // 0 at j >= P
  dL[j] = dj;
  aL[0][j] = j == 0 ? 1.0 : 0.0;
  aL[1][j] = 0.0;
  __syncthreads();
  double E = rL[0];
  bool bad = !(E > 0.0) || !(E < HUGE_VAL);
  double aj = j == 0 ? 1.0 : 0.0;
  double xj = (j == 0 && !bad) ? dj / E : 0.0;
  int cur = 0;
  for (int k = 1; k < P && !bad; ++k) {                 // bad is uniform: every thread computes E from the same LDS words
    const double rk = j < k ? rL[k - j] : 0.0;
    double pa = wave_sum(aj * rk);
    double px = wave_sum(xj * rk);
    if (lane == 0) {
      red[0][wid] = pa;
      red[1][wid] = px;
    }
    __syncthreads();                                    // (A) the wave sums are in LDS
    double acc = red[0][0], sx = red[1][0];
#pragma unroll
    for (int w = 1; w < MAXP / 64; ++w) {
      acc += red[0][w];
      sx += red[1][w];
    }
    const double kappa = -acc / E;
    const double an = aj + kappa * aL[cur][k - (j <= k ? j : k)];      // a[k - j]; threads j > k read a[0] and drop it
    E = E * (1.0 - kappa * kappa);
    bad = !(E > 0.0) || !(E < HUGE_VAL);
    if (j <= k) aj = an;
    aL[cur ^ 1][j] = aj;
    __syncthreads();                                    // (B) a' is in LDS; every read of red and of aL[cur] is done
    cur ^= 1;
    if (!bad) {
      const double mu = (dL[k] - sx) / E;
      if (j <= k) xj = fma(mu, aL[cur][k - j], xj);
    }
  }
  if (!(xj == xj) || !(fabs(xj) < HUGE_VAL)) bad = true;     // per thread; folded below
  const int anybad = __syncthreads_or(bad ? 1 : 0);
  if (j < P) c_out[(long)b * P + j] = xj;
  if (j == 0) status[b] = anybad ? 1 : 0;
}

// ---- projection --------------------------------------------------------------------------------------------------------
// grid (tile, item), 256 threads; thread tid owns the outputs m0 + tid + 256 q, q < 4, so one broadcast read of c[t]
// feeds four FMAs; s[m - t] is stride-1 across the lanes.  t ascends.  The tile's proj^2 and (e - proj)^2, e = 0 at
// m >= n, are folded in a fixed order (q ascending per thread, wave butterfly, waves in index order) into
// part [B][nchunks][2].
__global__ __launch_bounds__(256) void bss_project_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                          const int* __restrict__ lengths, long ld, int P,
                                                          const double* __restrict__ cvec, const int* __restrict__ status,
                                                          long nchunks, double* __restrict__ part) {
  __shared__ double sW[PROJ_CHUNK + MAXP - 1];
  __shared__ double cL[MAXP];
  __shared__ double red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long n = min((long)lengths[b], ld);
  const long M = n + P - 1;
  const long m0 = (long)blockIdx.x * PROJ_CHUNK;
  if (m0 >= M || status[b] != 0) return;                // uniform over the workgroup
  const float* s = ref + (long)b * ld;
  const float* e = est + (long)b * ld;
  const int H = P - 1;
  const int len = (int)min((long)PROJ_CHUNK, M - m0);
  for (int i = tid; i < PROJ_CHUNK + H; i += 256) {
    const long m = m0 - H + i;
    sW[i] = (i < len + H && m >= 0 && m < n) ? (double)s[m] : 0.0;
  }
  for (int t = tid; t < P; t += 256) cL[t] = cvec[(long)b * P + t];
  __syncthreads();
  double acc[PROJ_PER_THREAD];
#pragma unroll
  for (int q = 0; q < PROJ_PER_THREAD; ++q) acc[q] = 0.0;
  const double* w = sW + H + tid;
#pragma unroll 2
  for (int t = 0; t < P; ++t) {
    const double ct = cL[t];
#pragma unroll
    for (int q = 0; q < PROJ_PER_THREAD; ++q) acc[q] = fma(ct, w[256 * q - t], acc[q]);
  }
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int q = 0; q < PROJ_PER_THREAD; ++q) {
    const long m = m0 + tid + 256 * q;
    if (m < M) {
      const double ev = m < n ? (double)e[m] : 0.0;
      const double res = ev - acc[q];
      num = fma(acc[q], acc[q], num);
      den = fma(res, res, den);
    }
  }
  num = block_sum_waves<4>(num, red);
  den = block_sum_waves<4>(den, red);
  if (tid == 0) {
    double* o = part + ((long)b * nchunks + blockIdx.x) * 2;
    o[0] = num;
    o[1] = den;
  }
}

// one wave per item: lane l adds tiles l, l + 64, .. in ascending order, then the butterfly; SDR = 10 log10(num / den),
// +inf when den == 0, NaN (num, den and SDR) when the solve broke down
__global__ __launch_bounds__(64) void bss_finish_kernel(const double* __restrict__ part, const int* __restrict__ lengths,
                                                        long ld, int P, const int* __restrict__ status, long nchunks,
                                                        double* __restrict__ num_out, double* __restrict__ den_out,
                                                        double* __restrict__ sdr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (status[b] != 0) {                                 // uniform
    if (lane == 0) num_out[b] = den_out[b] = sdr[b] = qnan;
    return;
  }
  const long n = min((long)lengths[b], ld);
  const long nch = (n + P - 1 + PROJ_CHUNK - 1) / PROJ_CHUNK;
  const double* p = part + (long)b * nchunks * 2;
  double num = 0.0, den = 0.0;
  for (long c = lane; c < nch; c += 64) {
    num += p[2 * c];
    den += p[2 * c + 1];
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) {
    num_out[b] = num;
    den_out[b] = den;
    sdr[b] = den == 0.0 ? HUGE_VAL : 10.0 * log10(num / den);
  }
}

// ---- _scale_bss_eval ---------------------------------------------------------------------------------------------------
// one workgroup per item, two passes, every energy summed directly: pass 1 |s|^2, <s, e>, |e - s|^2 -> alpha; pass 2
// |e - alpha s|^2.  out [B][4] = si_sdr, sd_sdr, snr, srr.
__global__ __launch_bounds__(256) void bss_scale_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                        const int* __restrict__ lengths, long ld, double* __restrict__ sums,
                                                        double* __restrict__ out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const long n = min((long)lengths[b], ld);
  const float* s = ref + (long)b * ld;
  const float* e = est + (long)b * ld;
  double sss = 0.0, sse = 0.0, srs = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double a = s[i], c = e[i], d = c - a;
    sss = fma(a, a, sss);
    sse = fma(a, c, sse);
    srs = fma(d, d, srs);
  }
  sss = block_sum_waves<4>(sss, red);
  sse = block_sum_waves<4>(sse, red);
  srs = block_sum_waves<4>(srs, red);
  const double alpha = sse / sss;
  double ra = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double d = (double)e[i] - alpha * (double)s[i];
    ra = fma(d, d, ra);
  }
  ra = block_sum_waves<4>(ra, red);
  if (threadIdx.x == 0) {
    if (sums) {
      double* o = sums + 4L * b;
      o[0] = sss; o[1] = sse; o[2] = srs; o[3] = ra;
    }
    const double snr = 10.0 * log10(sss / srs);
    const double inv = 1.0 - 1.0 / alpha;
    double* o = out + 4L * b;
    o[0] = 10.0 * log10(alpha * alpha * sss / ra);
    o[1] = snr + 10.0 * log10(alpha * alpha);
    o[2] = snr;
    o[3] = -10.0 * log10(inv * inv);
  }
}

bool bad_shape(int B, long ld, int P) { return B <= 0 || ld <= 0 || P < 1 || P > MAXP; }
long corr_chunks(long ld) { return (ld + CORR_CHUNK - 1) / CORR_CHUNK; }
long proj_chunks(long ld, int P) { return (ld + P - 1 + PROJ_CHUNK - 1) / PROJ_CHUNK; }

}  // namespace

extern "C" {

int nppc_bss_shape(long ld, int P, int* corr_chunk, int* corr_tile, int* proj_chunk, long* corr_elems_per_item,
                   long* proj_elems_per_item) {
  if (ld <= 0 || P < 1) return NPPC_EBADARG;
  if (P > MAXP) return NPPC_EUNSUPPORTED;
  if (corr_chunk) *corr_chunk = CORR_CHUNK;
  if (corr_tile) *corr_tile = CORR_TILE;
  if (proj_chunk) *proj_chunk = PROJ_CHUNK;
  if (corr_elems_per_item) *corr_elems_per_item = corr_chunks(ld) * 2 * P;
  if (proj_elems_per_item) *proj_elems_per_item = proj_chunks(ld, P) * 2;
  return NPPC_OK;
}

int nppc_bss_corr(const float* ref, const float* est, const int* lengths, int B, long ld, int P, double* part,
                  long part_elems, void* stream) {
  if (!ref || !est || !lengths || !part || B <= 0 || ld <= 0 || P < 1) return NPPC_EBADARG;
  if (bad_shape(B, ld, P) || B > 65535 || corr_chunks(ld) >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const long nch = corr_chunks(ld);
  if (part_elems < (long)B * nch * 2 * P) return NPPC_EBADARG;
  hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, (hipStream_t)stream, ref, est, lengths,
                     ld, P, nch, part);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_bss_solve(const double* part, const int* lengths, int B, long ld, int P, double* r, double* d, double* c,
                   int* status, void* stream) {
  if (!part || !lengths || !r || !d || !c || !status || B <= 0 || ld <= 0 || P < 1) return NPPC_EBADARG;
  if (bad_shape(B, ld, P)) return NPPC_EUNSUPPORTED;
  hipLaunchKernelGGL(bss_solve_kernel, dim3(B), dim3(MAXP), 0, (hipStream_t)stream, part, lengths, ld, P, corr_chunks(ld), r,
                     d, c, status);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_bss_project(const float* ref, const float* est, const int* lengths, int B, long ld, int P, const double* c,
                     const int* status, double* part, long part_elems, double* num, double* den, double* sdr,
                     void* stream) {
  if (!ref || !est || !lengths || !c || !status || !part || !num || !den || !sdr || B <= 0 || ld <= 0 || P < 1)
    return NPPC_EBADARG;
  if (bad_shape(B, ld, P) || B > 65535 || proj_chunks(ld, P) >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const long nch = proj_chunks(ld, P);
  if (part_elems < (long)B * nch * 2) return NPPC_EBADARG;
  hipLaunchKernelGGL(bss_project_kernel, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, (hipStream_t)stream, ref, est,
                     lengths, ld, P, c, status, nch, part);
  NPPC_CHECK_LAUNCH();
  hipLaunchKernelGGL(bss_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, part, lengths, ld, P, status, nch, num,
                     den, sdr);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_bss_scale(const float* ref, const float* est, const int* lengths, int B, long ld, double* sums, double* out,
                   void* stream) {
  if (!ref || !est || !lengths || !out || B <= 0 || ld <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(bss_scale_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ref, est, lengths, ld, sums, out);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
