// Gap-constrained Griffin-Lim for spans longer than the resident kernel's cap: the same algorithm as
// gl_gap.hip, through the same per-element helpers (gl_gap_common.h), with the span's state (C, P for momentum, M, the time segment x) in a workspace in
// HBM / L2 instead of one workgroup's LDS, and one launch per half-iteration over many workgroups.
//   nppc_gl_gap_long_shape   argument rules, both caps and the workspace size; runs without a GPU
//   nppc_gl_gap_long         target magnitudes [B][V][F][T]
//   nppc_gl_gap_pc_long      magnitudes exp((pred + alpha_a pc_k) std + mean) formed on the fly, plus the alpha = 0 prediction
// mode 1 routes by item: spans within the resident cap run gl_gap_kernel as nppc_gl_gap does, spans over it run here; mode 2
// sends every item here.  Launches of one call, all on the caller's stream, no host read, 2 n_iter + O(1) of them:
//   gl_span_kernel, istft_any_kernel, gl_fill_kernel, gl_base_kernel   the known part, the kernels of gl_gap.hip
//   (mode 1: gl_base_kernel and gl_gap_kernel for the resident items)
//   gl_long_live_kernel      per item: gap / neighbour flag of every span frame and the ascending list of flagged frames
//   gl_long_setup_kernel     M and C_0 = M exp(i phi0) on the gap frames, P = 0; one |M|^2 partial per workgroup
//   n_iter x { gl_long_synth_kernel     x_n = istft(C_n) on the span: one thread per padded-coordinate sample
//              gl_long_analysis_kernel  R_n = stft(x_n) on gap and neighbour frames, the projection, one partial per workgroup }
//   gl_long_synth_kernel     x of the last C
//   gl_long_finish_kernel    partials folded in ascending order into dist and target_norm; the span's samples into out
// No kernel waits for another workgroup: the launch boundary is the only synchronisation.  No atomics.  Every sample and
// every bin is one thread's sequential fp64 sum in the order gl_gap_kernel uses, so a waveform equals the resident path's bit
// for bit; dist and target_norm are folded across workgroups in another order than across the resident kernel's strides.
#include "gl_gap_common.h"

using namespace nppc_gl;

namespace {

struct GlLong {
  int cap;      // span cap of the tiled path (gap bounding range + 2 r)
  int span;     // min(cap, T): span frames that can exist
  int G;        // min(cap - 2 r, T): frame slots of C, P, M
  int Pmax;     // (span - 1) hop + N
  int nA, nS;   // workgroups per waveform of the analysis and of the set-up launch
  int nfr;      // gap frames a synthesis tile stages at most
};

struct GlLongWork {
  double *base, *den;          // [B][Pmax]
  int *nlive, *live, *flag;    // [B], [B][span], [B][span]: per span frame 1 gap, 2 neighbour, 0 neither
  float2 *C, *P;               // [B V][G F]
  float *M, *x;                // [B V][G F], [B V][Pmax]
  double *dpart, *tpart;       // [B V][n_iter][nA], [B V][nS]
};

int gl_long_geom(const GlGeom& g, int B, int V, int long_max_span, GlLong* q, size_t* work) {
  if (long_max_span < 0 || (long_max_span != 0 && long_max_span <= 2 * g.r)) return NPPC_EBADARG;
  q->cap = long_max_span ? long_max_span : g.T + 2 * g.r;           // default: no gap of the clip is refused
  q->span = q->cap < g.T ? q->cap : g.T;
  q->G = q->cap - 2 * g.r < g.T ? q->cap - 2 * g.r : g.T;
  q->Pmax = (q->span - 1) * g.hop + g.N;
  q->nA = ceil_div((long)((q->span + 1) / 2) * g.F, GL_T);
  q->nS = ceil_div((long)q->G * g.F, GL_T);
  // a tile's 256 samples lie within 257 padded coordinates of each other, mirrored ones included
  const int nfr = (GL_T + g.N - 1) / g.hop + 2;
  q->nfr = nfr < q->G ? nfr : q->G;
  const size_t BV = (size_t)B * V, GF = (size_t)q->G * g.F;
  *work = 2 * al256(sizeof(double) * (size_t)B * q->Pmax) + al256(sizeof(int) * (size_t)B) +
          2 * al256(sizeof(int) * (size_t)B * q->span) + (g.mom ? 2 : 1) * al256(sizeof(float2) * BV * GF) +
          al256(sizeof(float) * BV * GF) + al256(sizeof(float) * BV * q->Pmax) +
          al256(sizeof(double) * BV * (size_t)g.n_iter * q->nA) + al256(sizeof(double) * BV * q->nS);
  return NPPC_OK;
}

GlLongWork gl_long_carve(void* work, const GlGeom& g, const GlLong& q, int B, int V) {
  char* p = (char*)work;
  const size_t BV = (size_t)B * V, GF = (size_t)q.G * g.F;
  GlLongWork w;
  w.base = (double*)p, p += al256(sizeof(double) * (size_t)B * q.Pmax);
  w.den = (double*)p, p += al256(sizeof(double) * (size_t)B * q.Pmax);
  w.nlive = (int*)p, p += al256(sizeof(int) * (size_t)B);
  w.live = (int*)p, p += al256(sizeof(int) * (size_t)B * q.span);
  w.flag = (int*)p, p += al256(sizeof(int) * (size_t)B * q.span);
  w.C = (float2*)p, p += al256(sizeof(float2) * BV * GF);
  w.P = nullptr;
  if (g.mom) w.P = (float2*)p, p += al256(sizeof(float2) * BV * GF);
  w.M = (float*)p, p += al256(sizeof(float) * BV * GF);
  w.x = (float*)p, p += al256(sizeof(float) * BV * q.Pmax);
  w.dpart = (double*)p, p += al256(sizeof(double) * BV * (size_t)g.n_iter * q.nA);
  w.tpart = (double*)p;
  return w;
}

size_t gl_synth_lds(const GlGeom& g, const GlLong& q) { return sizeof(double2) * g.N + sizeof(float2) * (size_t)q.nfr * g.F; }
int gl_pairs_per_group(const GlGeom& g) { return (GL_T - 1) / g.F + 2; }   // pairs that 256 consecutive (pair, bin) meet
size_t gl_analysis_lds(const GlGeom& g) {
  return sizeof(double2) * g.N + sizeof(double) * 2 * GL_WAVES + sizeof(float) * 2 * (size_t)gl_pairs_per_group(g) * g.N;
}

// ------------------------------------------------------------------------------------------------ per-item frame lists
__global__ __launch_bounds__(GL_T) void gl_long_live_kernel(const float* __restrict__ mask, const int* __restrict__ info,
                                                             int* __restrict__ nlive, int* __restrict__ live,
                                                             int* __restrict__ flag, GlGeom g, GlLong q) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* it = info + b * GL_INFO;
  if (it[4] != GL_TILED) return;
  const int s_lo = it[2], ns = it[3] - s_lo + 1;               // ns <= q.span: t_hi - t_lo + 1 + 2 r <= q.cap, and ns <= T
  const float* m = mask + (size_t)b * g.T;
  int* fl = flag + (size_t)b * q.span;
  for (int j = tid; j < ns; j += GL_T) fl[j] = gl_frame_flag(m, s_lo + j, g.r, g.T);
  __syncthreads();
  if (tid == 0) {                                              // the frames the forward transform visits, in ascending order
    int* lv = live + (size_t)b * q.span;
    int nl = 0;
    for (int j = 0; j < ns; ++j)
      if (fl[j]) lv[nl++] = j;
    nlive[b] = nl;
  }
}

// ---------------------------------------------------------------------------------------------------- M, C_0, P = 0
__global__ __launch_bounds__(GL_T) void gl_long_setup_kernel(GlMag ms, const float* __restrict__ mask,
                                                              const float* __restrict__ phase, int phase_per_v,
                                                              const int* __restrict__ info, GlLongWork w, int V, GlGeom g,
                                                              GlLong q) {
  __shared__ double red[2 * GL_WAVES];
  const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  const int* it = info + b * GL_INFO;
  if (it[4] != GL_TILED) return;
  const int F = g.F, t_lo = it[0], G = it[1] - t_lo + 1;
  if ((long)blockIdx.x * GL_T >= (long)G * F) return;
  const size_t FT = (size_t)F * g.T, bv = (size_t)b * V + v, GF = (size_t)q.G * F;
  const float* m = mask + (size_t)b * g.T;
  float2* C = w.C + bv * GF;
  float* M = w.M + bv * GF;
  const GlMagRow src = gl_mag_row(ms, phase, phase_per_v, b, v, V, FT);
  double tn = 0.0;
  const int e = blockIdx.x * GL_T + tid;
  if (e < G * F) {
    const int k = e / G, j = e % G;
    float2 c0;
    float mg;
    tn = gl_init_bin(tn, src, m, k, t_lo + j, g.T, c0, mg);
    C[j * F + k] = c0;
    M[j * F + k] = mg;
    if (g.mom) w.P[bv * GF + j * F + k] = make_float2(0.f, 0.f);
  }
  tn = block_sum_waves<GL_WAVES>(tn, red);
  if (tid == 0) w.tpart[bv * q.nS + blockIdx.x] = tn;
}

// ------------------------------------------------------------------------------------------------------- x = istft(C)
// One thread per padded-coordinate sample of the span, gl_gap_kernel's gl_synth_sample.  A mirrored head or tail sample
// whose original lies in the span is that original: gl_gap_kernel copies it after a barrier, here the thread evaluates the
// original's expression itself (the same bits), because the original may belong to another workgroup.
__global__ __launch_bounds__(GL_T) void gl_long_synth_kernel(const float* __restrict__ mask, const int* __restrict__ info,
                                                              GlLongWork w, int V, GlGeom g, GlLong q) {
  extern __shared__ double2 gl_lds[];
  __shared__ int ta_s[GL_WAVES], tb_s[GL_WAVES];
  const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  const int* it = info + b * GL_INFO;
  if (it[4] != GL_TILED) return;
  const int N = g.N, F = g.F, hop = g.hop;
  const int t_lo = it[0], t_hi = it[1], s_lo = it[2], s_hi = it[3];
  const int Lp = (s_hi - s_lo) * hop + N, p_lo = s_lo * hop;
  if ((int)blockIdx.x * GL_T >= Lp) return;
  double2* tw = gl_lds;
  float2* Cs = reinterpret_cast<float2*>(tw + N);
  dft_twiddles(tw, N, GL_T);
  const size_t bv = (size_t)b * V + v;
  const float* m = mask + (size_t)b * g.T;
  const double* bs = w.base + (size_t)b * q.Pmax;
  const double* dn = w.den + (size_t)b * q.Pmax;
  const int i = blockIdx.x * GL_T + tid;
  int ii = i, p = 0, t0 = 1, t1 = 0;                           // t0 > t1: no gap frame to add
  double d = 0.0;
  if (i < Lp) {
    const int o = p_lo + i - g.pad;
    if (o < 0 || o >= g.L) {
      const int mi = reflect_index(p_lo + i, g.pad, g.L) + g.pad - p_lo;
      if (mi >= 0 && mi < Lp) ii = mi;
    }
    d = dn[ii];
    if (d != 0.0) {
      p = reflect_index(p_lo + ii, g.pad, g.L) + g.pad;
      gl_reach(p, N, hop, t_lo, t_hi, t0, t1);
    }
  }
  // the gap frames this tile reads: [ta, tb]
  int ta = t0 <= t1 ? t0 : t_hi + 1, tb = t0 <= t1 ? t1 : t_lo - 1;
  for (int o = 32; o > 0; o >>= 1) {
    const int a2 = __shfl_xor(ta, o, 64), b2 = __shfl_xor(tb, o, 64);
    ta = a2 < ta ? a2 : ta;
    tb = b2 > tb ? b2 : tb;
  }
  if ((tid & 63) == 0) ta_s[tid >> 6] = ta, tb_s[tid >> 6] = tb;
  __syncthreads();
  for (int wv = 0; wv < GL_WAVES; ++wv) {
    ta = ta_s[wv] < ta ? ta_s[wv] : ta;
    tb = tb_s[wv] > tb ? tb_s[wv] : tb;
  }
  if (tb - ta + 1 > q.nfr) tb = ta + q.nfr - 1;                // cannot happen (gl_long_geom); never past the staging area
  const float2* C = w.C + bv * (size_t)q.G * F;
  const int ne = tb >= ta ? (tb - ta + 1) * F : 0;
  for (int e = tid; e < ne; e += GL_T) Cs[e] = C[(size_t)(ta - t_lo) * F + e];
  __syncthreads();
  if (i >= Lp) return;
  float x = 0.f;
  if (d != 0.0)                                                // a known frame between two gaps is in `base`
    x = gl_synth_sample(
        tw, N, hop, p, t0, t1, bs[ii], d, [&](int t) { return m[t] == 0.f && t <= tb; },
        [&](int t) { return Cs + (size_t)(t - ta) * F; });
  w.x[bv * q.Pmax + i] = x;
}

// ------------------------------------------------------------------------------ R = stft(x), the projections, one partial
__global__ __launch_bounds__(GL_T) void gl_long_analysis_kernel(const float* __restrict__ known, const int* __restrict__ info,
                                                                 GlLongWork w, int V, int n, GlGeom g, GlLong q) {
  extern __shared__ double2 gl_lds[];
  const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  const int* it = info + b * GL_INFO;
  if (it[4] != GL_TILED) return;
  const int N = g.N, F = g.F, hop = g.hop;
  const int nlive = w.nlive[b], npair = (nlive + 1) / 2;
  const int q0 = blockIdx.x * GL_T;
  if (q0 >= npair * F) return;
  const int t_lo = it[0], s_lo = it[2];
  double2* tw = gl_lds;
  double* red = reinterpret_cast<double*>(tw + N);
  float* xs = reinterpret_cast<float*>(red + 2 * GL_WAVES);    // [pair of this workgroup][2][N]
  const size_t bv = (size_t)b * V + v, GF = (size_t)q.G * F, FT = (size_t)F * g.T;
  const int* live = w.live + (size_t)b * q.span;
  const int* flag = w.flag + (size_t)b * q.span;
  const float* xg = w.x + bv * q.Pmax;
  dft_twiddles(tw, N, GL_T);
  const int pr_a = q0 / F;
  int q1 = q0 + GL_T - 1;
  q1 = q1 > npair * F - 1 ? npair * F - 1 : q1;
  const int npr = q1 / F - pr_a + 1;                           // <= gl_pairs_per_group
  for (int e = tid; e < npr * 2 * N; e += GL_T) {
    const int nn = e % N, h = (e / N) & 1, pr = 2 * (pr_a + e / (2 * N));
    const int j = h && pr + 1 < nlive ? live[pr + 1] : live[pr];
    xs[e] = xg[(size_t)j * hop + nn];
  }
  __syncthreads();
  float2* C = w.C + bv * GF;
  float2* P = g.mom ? w.P + bv * GF : nullptr;
  const float* M = w.M + bv * GF;
  const float* kre = known + (size_t)b * 2 * FT;
  const float* kim = kre + FT;
  double dacc = 0.0;
  const int qq = q0 + tid;
  if (qq < npair * F) {
    const int k = qq % F, pr = 2 * (qq / F);
    const int j0 = live[pr], j1 = pr + 1 < nlive ? live[pr + 1] : j0;
    const int f0 = flag[j0], f1 = pr + 1 < nlive ? flag[j1] : 0;
    const float* x0 = xs + (size_t)(qq / F - pr_a) * 2 * N;
    const GlBinPair R = gl_dft_pair(tw, N, k, x0, x0 + N);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = s_lo + (h ? j1 : j0);
      dacc = gl_project(dacc, h ? f1 : f0, h ? R.r1 : R.r0, h ? R.i1 : R.i0, (t - t_lo) * F + k, (size_t)k * g.T + t, C, P, M, kre,
                        kim, g.mom, g.c);
    }
  }
  dacc = block_sum_waves<GL_WAVES>(dacc, red);
  if (tid == 0) w.dpart[(bv * g.n_iter + n) * q.nA + blockIdx.x] = dacc;
}

// ------------------------------------------------------------------------------------- partials -> dist, tnorm; x -> out
__global__ __launch_bounds__(GL_T) void gl_long_finish_kernel(const int* __restrict__ info, GlLongWork w,
                                                               float* __restrict__ out, double* __restrict__ dist,
                                                               double* __restrict__ tnorm, int V, int all, GlGeom g, GlLong q) {
  const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  const int* it = info + b * GL_INFO;
  const size_t bv = (size_t)b * V + v;
  if (it[4] != GL_TILED) {                                     // mode 2: refused items are NaN, items without a gap 0
    if (!all || blockIdx.x != 0) return;
    const double val = it[4] == GL_REFUSED ? (double)__builtin_nanf("") : 0.0;
    for (int n = tid; n < g.n_iter; n += GL_T) dist[bv * g.n_iter + n] = val;
    if (tid == 0) tnorm[bv] = val;
    return;
  }
  const int o = it[6] + blockIdx.x * GL_T + tid;
  if (o < it[7]) out[bv * g.L + o] = w.x[bv * q.Pmax + o + g.pad - it[2] * g.hop];
  if (blockIdx.x != 0) return;
  const int nblk = (((w.nlive[b] + 1) / 2) * g.F + GL_T - 1) / GL_T;
  for (int n = tid; n < g.n_iter; n += GL_T) {
    const double* pp = w.dpart + (bv * g.n_iter + n) * q.nA;
    double s = pp[0];
    for (int j = 1; j < nblk; ++j) s += pp[j];
    dist[bv * g.n_iter + n] = sqrt(s);
  }
  if (tid == 0) {
    const int ns = ((it[1] - it[0] + 1) * g.F + GL_T - 1) / GL_T;
    const double* pp = w.tpart + bv * q.nS;
    double s = pp[0];
    for (int j = 1; j < ns; ++j) s += pp[j];
    tnorm[bv] = sqrt(s);
  }
}

int gl_long_run(const GlMag& ms, const float* known, const float* mask, const float* phase, int phase_per_v, float* out,
                double* dist, double* tnorm, int* status, void* work, long work_bytes, int B, int V, int T, int nfft, int hop,
                int L, int n_iter, double momentum, int max_span, int long_max_span, int mode, void* stream) {
  if (!known || !mask || !phase || !out || !tnorm || !status || !work || (n_iter > 0 && !dist) || (mode != 1 && mode != 2))
    return NPPC_EBADARG;
  GlGeom g;
  GlLong q;
  size_t lds, need, need_long;
  int why;
  int rc = gl_geom(B, V, nfft / 2 + 1, T, nfft, hop, L, n_iter, momentum, max_span, &g, &lds, &need, &why);
  if (rc != NPPC_OK) return rc;
  if ((rc = gl_long_geom(g, B, V, long_max_span, &q, &need_long)) != NPPC_OK) return rc;
  if (work_bytes < (long)(need + need_long)) return NPPC_EBADARG;
  const size_t lds_s = gl_synth_lds(g, q), lds_a = gl_analysis_lds(g);
  if (lds_s > 64 * 1024 || lds_a > 64 * 1024) return NPPC_EUNSUPPORTED;     // 35 KB / 17 KB at most under the n_fft limits
  const GlWork w = gl_carve(work, g, B);
  const GlLongWork lw = gl_long_carve((char*)work + need, g, q, B, V);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = gl_launch_known(known, mask, w, out, status, B, V, g, mode == 2 ? GL_ROUTE_ALL : GL_ROUTE_OVER, q.cap, stream)) != NPPC_OK)
    return rc;
  if (mode == 1) {                                             // the items within the resident cap, as nppc_gl_gap runs them
    if ((rc = gl_launch_base(w.kspec, mask, w.info, w.base, w.den, B, g, GL_RESIDENT, stream)) != NPPC_OK) return rc;
    if ((rc = gl_launch_resident(ms, known, mask, phase, phase_per_v, w, out, dist, tnorm, B, V, g, lds, stream)) != NPPC_OK)
      return rc;
  }
  GlGeom gb = g;
  gb.Pmax = q.Pmax;                                            // rows of the tiled path's base and den
  if ((rc = gl_launch_base(w.kspec, mask, w.info, lw.base, lw.den, B, gb, GL_TILED, stream)) != NPPC_OK) return rc;
  hipLaunchKernelGGL(gl_long_live_kernel, dim3(B), dim3(GL_T), 0, s, mask, w.info, lw.nlive, lw.live, lw.flag, g, q);
  NPPC_CHECK_LAUNCH();
  hipLaunchKernelGGL(gl_long_setup_kernel, dim3(q.nS, V, B), dim3(GL_T), 0, s, ms, mask, phase, phase_per_v, w.info, lw, V, g, q);
  NPPC_CHECK_LAUNCH();
  const dim3 grid_s(ceil_div(q.Pmax, GL_T), V, B), grid_a(q.nA, V, B);
  for (int n = 0;; ++n) {
    hipLaunchKernelGGL(gl_long_synth_kernel, grid_s, dim3(GL_T), lds_s, s, mask, w.info, lw, V, g, q);
    NPPC_CHECK_LAUNCH();
    if (n == n_iter) break;
    hipLaunchKernelGGL(gl_long_analysis_kernel, grid_a, dim3(GL_T), lds_a, s, known, w.info, lw, V, n, g, q);
    NPPC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(gl_long_finish_kernel, grid_s, dim3(GL_T), 0, s, w.info, lw, out, dist, tnorm, V, mode == 2, g, q);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // namespace

extern "C" {

int nppc_gl_gap_long_shape(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                           int long_max_span, int* why, int* r, int* span_cap, int* long_span_cap, long* lds_bytes,
                           long* work_bytes) {
  GlGeom g;
  GlLong q;
  size_t lds, work, work_long = 0;
  int y = 0;
  int rc = gl_geom(B, V, F, T, nfft, hop, L, n_iter, momentum, max_span, &g, &lds, &work, &y);
  if (rc == NPPC_OK && (rc = gl_long_geom(g, B, V, long_max_span, &q, &work_long)) != NPPC_OK) y = 5;
  if (why) *why = rc == NPPC_OK ? 0 : y;
  if (rc != NPPC_OK) return rc;
  if (r) *r = g.r;
  if (span_cap) *span_cap = g.cap;
  if (long_span_cap) *long_span_cap = q.cap;
  if (lds_bytes) *lds_bytes = (long)lds;
  if (work_bytes) *work_bytes = (long)(work + work_long);
  return NPPC_OK;
}

int nppc_gl_gap_long(const float* target_mag, const float* known_spec, const float* mask, const float* init_phase,
                     int phase_per_variation, float* out, double* dist, double* target_norm, int* status, void* work,
                     long work_bytes, int B, int V, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                     int long_max_span, int mode, void* stream) {
  GlMag ms;
  if (gl_mag_target(target_mag, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_long_run(ms, known_spec, mask, init_phase, phase_per_variation != 0, out, dist, target_norm, status, work, work_bytes,
                     B, V, T, nfft, hop, L, n_iter, momentum, max_span, long_max_span, mode, stream);
}

int nppc_gl_gap_pc_long(const float* pred, const float* pc, const float* mean, const float* stdev, const float* alphas,
                        const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                        double* target_norm, int* status, void* work, long work_bytes, int B, int K, int A, int T, int nfft,
                        int hop, int L, int n_iter, double momentum, int max_span, int long_max_span, int mode, void* stream) {
  GlMag ms;
  if (gl_mag_pc(pred, pc, mean, stdev, alphas, K, A, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_long_run(ms, known_spec, mask, init_phase, 0, out, dist, target_norm, status, work, work_bytes, B, K * A + 1, T, nfft,
                     hop, L, n_iter, momentum, max_span, long_max_span, mode, stream);
}

int nppc_gl_gap_post_long(const float* pred, const float* pc, const float* mean, const float* stdev, const float* z,
                          const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                          double* target_norm, int* status, void* work, long work_bytes, int B, int K, int S, int T, int nfft,
                          int hop, int L, int n_iter, double momentum, int max_span, int long_max_span, int mode, void* stream) {
  GlMag ms;
  if (gl_mag_post(pred, pc, mean, stdev, z, K, S, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_long_run(ms, known_spec, mask, init_phase, 0, out, dist, target_norm, status, work, work_bytes, B, S + 1, T, nfft, hop,
                     L, n_iter, momentum, max_span, long_max_span, mode, stream);
}

}  // extern "C"
