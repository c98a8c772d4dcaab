// Gap-constrained Griffin-Lim for gfx950: the phase of the gap frames of an inpainted spectrogram is
// iterated against a target magnitude while the complex STFT of every known frame is held fixed.
//   nppc_gl_gap_shape   argument rules, effective span cap, LDS and workspace sizes; runs without a GPU
//   nppc_gl_phase_init  phase_advance_init: the phase of the known frame next to a gap run, advanced by 2 pi f hop / n_fft
//   nppc_gl_gap         target magnitudes [B][V][F][T]
//   nppc_gl_gap_pc      magnitudes exp((pred + alpha_a pc_k) std + mean) formed on the fly, plus the alpha = 0 prediction
// Launches of one call, all on the caller's stream, no host synchronisation:
//   gl_span_kernel   per item: bounding gap frames, span, status; the known spectrum with its gap frames zeroed
//   istft_any_kernel (nppc_istft_any) of that spectrum -> the samples no gap frame reaches, bit for bit what istft_any gives
//   gl_base_kernel   per item and padded-coordinate sample of the span: fp64 overlap-add of the KNOWN frames and the envelope
//   gl_fill_kernel   copies the known waveform to every variation outside the gap's reach (NaN for an item over the cap)
//   gl_gap_kernel    one workgroup per (item, variation): all iterations with the gap spectra C, the previous transform P
//                    (momentum only), the target magnitudes, the span's time segment and the twiddles resident in LDS
// What this file shares with the tiled path for spans over the cap (gl_gap_long.hip, section 8g: nppc_gl_gap_long_shape,
// nppc_gl_gap_long, nppc_gl_gap_pc_long) is in gl_gap_common.h, the per-element expressions of gl_gap_kernel included;
// gl_span_kernel, gl_base_kernel and gl_fill_kernel serve both.
// Both transforms are direct DFTs out of LDS as in inpaint_validator.hip / frontend.hip: twiddles exp(2 pi i j / N) in fp64
// indexed by (k n) mod N in integers, fp64 accumulation, fp32 state.  Every sum has one writer and a fixed order: no
// atomics; a waveform does not depend on the batch or on the run.
#include "gl_gap_common.h"

using namespace nppc_gl;

namespace {

constexpr size_t GL_LDS_BUDGET = 160 * 1024;     // LDS of one CU
constexpr int GL_NLIVE = 2 * NPPC_GL_MAX_SPAN_FRAMES;   // byte of the flag area that holds the number of live frames
static_assert(GL_NLIVE < 256, "the flag area is al256(cap) >= 256 bytes");

size_t gl_lds_bytes(int N, int F, int hop, int r, int cap, int mom) {
  const size_t G = cap - 2 * r;
  return sizeof(double2) * N + sizeof(double) * 2 * GL_WAVES + G * F * (sizeof(float2) * (mom ? 2 : 1) + sizeof(float)) +
         sizeof(float) * ((size_t)(cap - 1) * hop + N) + al256(cap);
}

}  // namespace

int nppc_gl::gl_geom(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span, GlGeom* g,
            size_t* lds, size_t* work, int* why) {
  *why = 5;
  if (B <= 0 || B > 65535 || V <= 0 || V > 65535 || T <= 0 || nfft < 2 || hop < 1 || hop > nfft || L <= 0 || max_span < 0)
    return NPPC_EBADARG;
  *why = 3;
  if (nfft > 512 || (nfft + hop - 1) / hop > 8) return NPPC_EUNSUPPORTED;
  *why = 1;
  if (F != nfft / 2 + 1) return NPPC_EBADARG;
  *why = 2;
  if (1 + L / hop != T) return NPPC_EBADARG;
  *why = 4;
  if (n_iter < 0 || !(momentum >= 0.0) || !(momentum < 1e30)) return NPPC_EBADARG;
  *why = 5;
  if (L < nfft) return NPPC_EBADARG;                                        // one reflection reaches every padded sample
  g->N = nfft, g->F = F, g->hop = hop, g->T = T, g->L = L;
  const long full = (long)nfft + (long)hop * (T - 1) - nfft / 2;
  g->Lk = (int)(L < full ? L : full);
  g->pad = nfft / 2;
  g->r = (nfft + hop - 1) / hop - 1;
  g->n_iter = n_iter;
  g->mom = momentum > 0.0;
  g->c = momentum / (1.0 + momentum);
  int cap = max_span == 0 || max_span > NPPC_GL_MAX_SPAN_FRAMES ? NPPC_GL_MAX_SPAN_FRAMES : max_span;
  while (cap > 2 * g->r && gl_lds_bytes(nfft, F, hop, g->r, cap, g->mom) > GL_LDS_BUDGET) --cap;
  if (cap <= 2 * g->r) return max_span == 0 ? NPPC_EUNSUPPORTED : NPPC_EBADARG;
  g->cap = cap;
  g->Gmax = cap - 2 * g->r;
  g->Pmax = (cap - 1) * hop + nfft;
  *lds = gl_lds_bytes(nfft, F, hop, g->r, cap, g->mom);
  *work = al256(sizeof(int) * GL_INFO * (size_t)B) + al256(sizeof(float) * 2 * (size_t)B * F * T) +
          al256(sizeof(float) * (size_t)B * L) + 2 * al256(sizeof(double) * (size_t)B * g->Pmax);
  return NPPC_OK;
}

GlWork nppc_gl::gl_carve(void* work, const GlGeom& g, int B) {
  char* p = (char*)work;
  GlWork w;
  w.info = (int*)p, p += al256(sizeof(int) * GL_INFO * (size_t)B);
  w.kspec = (float*)p, p += al256(sizeof(float) * 2 * (size_t)B * g.F * g.T);
  w.kwave = (float*)p, p += al256(sizeof(float) * (size_t)B * g.L);
  w.base = (double*)p, p += al256(sizeof(double) * (size_t)B * g.Pmax);
  w.den = (double*)p;
  return w;
}

namespace {

// ---------------------------------------------------------------------------------------------------- per-item set-up
__global__ __launch_bounds__(256) void gl_span_kernel(const float* __restrict__ known, const float* __restrict__ mask,
                                                       int* __restrict__ info, float* __restrict__ kspec,
                                                       int* __restrict__ status, GlGeom g, int route, int long_cap) {
  __shared__ int lo_s[4], hi_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* m = mask + (size_t)b * g.T;
  int lo = g.T, hi = -1;
  for (int t = tid; t < g.T; t += 256)
    if (m[t] == 0.f) {
      lo = t < lo ? t : lo;
      hi = t > hi ? t : hi;
    }
  for (int o = 32; o > 0; o >>= 1) {
    const int l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((tid & 63) == 0) lo_s[tid >> 6] = lo, hi_s[tid >> 6] = hi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      lo = lo_s[w] < lo ? lo_s[w] : lo;
      hi = hi_s[w] > hi ? hi_s[w] : hi;
    }
    int* o = info + b * GL_INFO;
    const int has = hi >= 0;
    int bad = has && hi - lo + 1 + 2 * g.r > g.cap;           // GL_REFUSED; with a route, GL_TILED where the tiled path takes it
    if (has && (bad || route == GL_ROUTE_ALL) && route != GL_ROUTE_OFF)
      bad = hi - lo + 1 + 2 * g.r > long_cap ? GL_REFUSED : GL_TILED;
    const int s_lo = has ? (lo - g.r > 0 ? lo - g.r : 0) : 0;
    const int s_hi = has ? (hi + g.r < g.T - 1 ? hi + g.r : g.T - 1) : 0;
    int oa = lo * g.hop - g.pad, ob = hi * g.hop + g.N - g.pad;
    oa = oa < 0 ? 0 : oa;
    ob = ob > g.L ? g.L : ob;
    o[0] = lo, o[1] = hi, o[2] = s_lo, o[3] = s_hi, o[4] = bad, o[5] = has, o[6] = has ? oa : 0, o[7] = has ? ob : 0;
    status[b] = bad == GL_REFUSED;
  }
  const size_t FT = (size_t)g.F * g.T;
  const float* src = known + (size_t)b * 2 * FT;
  float* dst = kspec + (size_t)b * 2 * FT;
  for (size_t e = tid; e < 2 * FT; e += 256) dst[e] = m[e % g.T] == 0.f ? 0.f : src[e];   // gap frames are never read
}

__global__ __launch_bounds__(256) void gl_base_kernel(const float* __restrict__ kspec, const float* __restrict__ mask,
                                                       const int* __restrict__ info, double* __restrict__ base,
                                                       double* __restrict__ den, GlGeom g, int mine) {
  extern __shared__ double2 gl_lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int* it = info + b * GL_INFO;
  if (it[4] != mine || !it[5]) return;                         // another path's item: nothing is written
  const int s_lo = it[2], s_hi = it[3];
  const int Lp = (s_hi - s_lo) * g.hop + g.N;
  if ((int)blockIdx.x * 256 >= Lp) return;
  dft_twiddles(gl_lds, g.N, 256);
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  if (i >= Lp) return;
  const int o = reflect_index(s_lo * g.hop + i, g.pad, g.L);
  double num = 0.0, dn = 0.0;
  if (o < g.Lk) {
    const int p = o + g.pad, a = p - g.N + 1;
    const int t0 = a <= 0 ? 0 : (a + g.hop - 1) / g.hop;
    int t1 = p / g.hop;
    t1 = t1 > g.T - 1 ? g.T - 1 : t1;
    const float* m = mask + (size_t)b * g.T;
    const float* re = kspec + (size_t)b * 2 * g.F * g.T;
    const float* im = re + (size_t)g.F * g.T;
    for (int t = t0; t <= t1; ++t) {
      const int n = p - t * g.hop;
      const double w = 0.5 - 0.5 * gl_lds[n].x;
      dn += w * w;
      if (m[t] == 0.f) continue;
      num += w * idft_sample(gl_lds, g.N, n, [&](int k) { return make_float2(re[(size_t)k * g.T + t], im[(size_t)k * g.T + t]); });
    }
  }
  base[(size_t)b * g.Pmax + i] = num;
  den[(size_t)b * g.Pmax + i] = dn * (double)g.N;
}

__global__ __launch_bounds__(256) void gl_fill_kernel(const float* __restrict__ kwave, const int* __restrict__ info,
                                                       float* __restrict__ out, int V, GlGeom g) {
  const int b = blockIdx.z, v = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= g.L) return;
  const int* it = info + b * GL_INFO;
  float* row = out + ((size_t)b * V + v) * g.L;
  if (it[4] == GL_REFUSED)
    row[o] = __builtin_nanf("");
  else if (!it[5] || o < it[6] || o >= it[7])
    row[o] = kwave[(size_t)b * g.L + o];
}

// ------------------------------------------------------------------------------------------------------ the iterations
__global__ __launch_bounds__(GL_T) void gl_gap_kernel(GlMag ms, const float* __restrict__ known, const float* __restrict__ mask,
                                                       const float* __restrict__ phase, int phase_per_v,
                                                       const int* __restrict__ info, const double* __restrict__ base,
                                                       const double* __restrict__ den, float* __restrict__ out,
                                                       double* __restrict__ dist, double* __restrict__ tnorm, int V, GlGeom g) {
  extern __shared__ double2 gl_lds[];
  const int tid = threadIdx.x, v = blockIdx.x, b = blockIdx.y;
  const int N = g.N, F = g.F, hop = g.hop;
  const int* it = info + b * GL_INFO;
  double* drow = dist + ((size_t)b * V + v) * g.n_iter;
  if (it[4] || !it[5]) {                                       // over the cap: NaN; no gap: the known waveform, d = 0
    const double val = it[4] ? (double)__builtin_nanf("") : 0.0;
    for (int n = tid; n < g.n_iter; n += GL_T) drow[n] = val;
    if (tid == 0) tnorm[(size_t)b * V + v] = val;
    return;
  }
  const int t_lo = it[0], t_hi = it[1], s_lo = it[2], s_hi = it[3], o_a = it[6], o_b = it[7];
  const int G = t_hi - t_lo + 1, ns = s_hi - s_lo + 1, Lp = (ns - 1) * hop + N, p_lo = s_lo * hop;

  double2* tw = gl_lds;
  double* red = reinterpret_cast<double*>(tw + N);
  float2* C = reinterpret_cast<float2*>(red + 2 * GL_WAVES);
  float2* P = C + (size_t)g.Gmax * F;
  float* M = reinterpret_cast<float*>(P + (g.mom ? (size_t)g.Gmax * F : 0));
  float* xp = M + (size_t)g.Gmax * F;
  unsigned char* flag = reinterpret_cast<unsigned char*>(xp + g.Pmax);   // per span frame: 1 gap, 2 neighbour, 0 neither
  unsigned char* live = flag + NPPC_GL_MAX_SPAN_FRAMES;        // span frames with a flag; their count at flag[GL_NLIVE]

  const size_t FT = (size_t)F * g.T;
  const float* m = mask + (size_t)b * g.T;
  const float* kre = known + (size_t)b * 2 * FT;
  const float* kim = kre + FT;
  dft_twiddles(tw, N, GL_T);
  for (int j = tid; j < ns; j += GL_T) flag[j] = (unsigned char)gl_frame_flag(m, s_lo + j, g.r, g.T);
  __syncthreads();
  if (tid == 0) {                                              // the frames the forward transform visits, in ascending order
    int nl = 0;
    for (int j = 0; j < ns; ++j)
      if (flag[j]) live[nl++] = (unsigned char)j;
    flag[GL_NLIVE] = (unsigned char)nl;
  }
  // C_0 = M exp(i phi0) on the gap frames
  const GlMagRow src = gl_mag_row(ms, phase, phase_per_v, b, v, V, FT);
  double tn = 0.0;
  for (int e = tid; e < G * F; e += GL_T) {
    const int k = e / G, j = e % G;
    float2 c0;
    float mg;
    tn = gl_init_bin(tn, src, m, k, t_lo + j, g.T, c0, mg);
    C[j * F + k] = c0;
    M[j * F + k] = mg;
    if (g.mom) P[j * F + k] = make_float2(0.f, 0.f);
  }
  tn = block_sum_waves<GL_WAVES>(tn, red);                                  // its barriers also publish tw, flag, C, M, P
  if (tid == 0) tnorm[(size_t)b * V + v] = sqrt(tn);

  const double* bs = base + (size_t)b * g.Pmax;
  const double* dn = den + (size_t)b * g.Pmax;
  for (int n = 0;; ++n) {
    // x_n = istft(C_n) on the span, in padded coordinates: known frames from `base`, gap frames from C in ascending order
    for (int i = tid; i < Lp; i += GL_T) {
      const int o = p_lo + i - g.pad;
      if (o < 0 || o >= g.L) {                                 // a reflected sample whose mirror is in the span: copied below
        const int mi = reflect_index(p_lo + i, g.pad, g.L) + g.pad - p_lo;
        if (mi >= 0 && mi < Lp) continue;
      }
      const double d = dn[i];
      float x = 0.f;
      if (d != 0.0) {
        const int p = reflect_index(p_lo + i, g.pad, g.L) + g.pad;
        int t0, t1;
        gl_reach(p, N, hop, t_lo, t_hi, t0, t1);
        x = gl_synth_sample(
            tw, N, hop, p, t0, t1, bs[i], d, [&](int t) { return flag[t - s_lo] == 1; },
            [&](int t) { return C + (size_t)(t - t_lo) * F; });
      }
      xp[i] = x;
    }
    __syncthreads();
    for (int i = tid; i < Lp; i += GL_T) {                      // the mirrored head and tail from their in-span originals
      const int o = p_lo + i - g.pad;
      if (o >= 0 && o < g.L) continue;
      const int mi = reflect_index(p_lo + i, g.pad, g.L) + g.pad - p_lo;
      if (mi >= 0 && mi < Lp) xp[i] = xp[mi];
    }
    __syncthreads();
    if (n == g.n_iter) break;
    // R_n = stft(x_n) on the gap and neighbour frames, two live frames per thread on one twiddle stream; then the projections
    double dacc = 0.0;
    const int nlive = flag[GL_NLIVE], npair = (nlive + 1) / 2;
    for (int q = tid; q < npair * F; q += GL_T) {
      const int k = q % F, pr = 2 * (q / F);
      const int j0 = live[pr], j1 = pr + 1 < nlive ? live[pr + 1] : j0;
      const int f0 = flag[j0], f1 = pr + 1 < nlive ? flag[j1] : 0;
      const GlBinPair R = gl_dft_pair(tw, N, k, xp + (size_t)j0 * hop, xp + (size_t)j1 * hop);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int t = s_lo + (h ? j1 : j0);
        dacc = gl_project(dacc, h ? f1 : f0, h ? R.r1 : R.r0, h ? R.i1 : R.i0, (t - t_lo) * F + k, (size_t)k * g.T + t, C, P, M, kre,
                          kim, g.mom, g.c);
      }
    }
    dacc = block_sum_waves<GL_WAVES>(dacc, red);                            // its barriers also publish C and P
    if (tid == 0) drow[n] = sqrt(dacc);
  }
  float* row = out + ((size_t)b * V + v) * g.L;
  for (int o = o_a + tid; o < o_b; o += GL_T) row[o] = xp[o + g.pad - p_lo];
}

__global__ __launch_bounds__(256) void gl_phase_init_kernel(const float* __restrict__ known, const float* __restrict__ mask,
                                                             float* __restrict__ phase, int F, int T, int N, int hop) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F * T) return;
  const int k = e / T, t = e % T;
  const float* m = mask + (size_t)b * T;
  float out = 0.f;
  if (m[t] == 0.f) {
    int t0 = t - 1;
    while (t0 >= 0 && m[t0] == 0.f) --t0;
    if (t0 < 0) {                                              // the run starts at frame 0: the known frame to its right
      t0 = t + 1;
      while (t0 < T && m[t0] == 0.f) ++t0;
    }
    if (t0 < T) {
      const size_t FT = (size_t)F * T;
      const float* re = known + (size_t)b * 2 * FT;
      const double a0 = atan2((double)re[FT + (size_t)k * T + t0], (double)re[(size_t)k * T + t0]);
      long q = ((long)k * hop % N) * (long)(t - t0) % N;       // f hop (t - t0) mod N, exact
      if (q < 0) q += N;
      double a = a0 + 2.0 * M_PI * (double)q / (double)N;
      if (a > M_PI) a -= 2.0 * M_PI;
      out = (float)a;
    }
  }
  phase[(size_t)b * F * T + e] = out;
}

}  // namespace

int nppc_gl::gl_launch_known(const float* known, const float* mask, const GlWork& w, float* out, int* status, int B, int V,
                             const GlGeom& g, int route, int long_cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gl_span_kernel, dim3(B), dim3(256), 0, s, known, mask, w.info, w.kspec, status, g, route, long_cap);
  NPPC_CHECK_LAUNCH();
  const long FT = (long)g.F * g.T;
  const int rk = nppc_istft_any(w.kspec, w.kspec + FT, 2 * FT, w.kwave, g.L, B, g.T, g.N, g.hop, g.L, stream);
  if (rk != NPPC_OK) return rk;
  hipLaunchKernelGGL(gl_fill_kernel, dim3(ceil_div(g.L, 256), V, B), dim3(256), 0, s, w.kwave, w.info, out, V, g);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gl::gl_launch_base(const float* kspec, const float* mask, const int* info, double* base, double* den, int B,
                            const GlGeom& g, int mine, void* stream) {
  hipLaunchKernelGGL(gl_base_kernel, dim3(ceil_div(g.Pmax, 256), B), dim3(256), sizeof(double2) * g.N, (hipStream_t)stream, kspec,
                     mask, info, base, den, g, mine);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gl::gl_launch_resident(const GlMag& ms, const float* known, const float* mask, const float* phase, int phase_per_v,
                                const GlWork& w, float* out, double* dist, double* tnorm, int B, int V, const GlGeom& g,
                                size_t lds, void* stream) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)gl_gap_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return NPPC_ELAUNCH;
  hipLaunchKernelGGL(gl_gap_kernel, dim3(V, B), dim3(GL_T), lds, (hipStream_t)stream, ms, known, mask, phase, phase_per_v, w.info,
                     w.base, w.den, out, dist, tnorm, V, g);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

namespace {

int gl_run(const GlMag& ms, const float* known, const float* mask, const float* phase, int phase_per_v, float* out, double* dist,
           double* tnorm, int* status, void* work, long work_bytes, int B, int V, int T, int nfft, int hop, int L, int n_iter,
           double momentum, int max_span, void* stream) {
  if (!known || !mask || !phase || !out || !tnorm || !status || !work || (n_iter > 0 && !dist)) return NPPC_EBADARG;
  GlGeom g;
  size_t lds, need;
  int why;
  int rc = gl_geom(B, V, nfft / 2 + 1, T, nfft, hop, L, n_iter, momentum, max_span, &g, &lds, &need, &why);
  if (rc != NPPC_OK) return rc;
  if (work_bytes < (long)need) return NPPC_EBADARG;
  const GlWork w = gl_carve(work, g, B);
  // the launch order of before the tiled path existed: span, known waveform, base, fill, iterations (base and fill are
  // independent of each other)
  if ((rc = gl_launch_known(known, mask, w, out, status, B, V, g, GL_ROUTE_OFF, 0, stream)) != NPPC_OK) return rc;
  if ((rc = gl_launch_base(w.kspec, mask, w.info, w.base, w.den, B, g, GL_RESIDENT, stream)) != NPPC_OK) return rc;
  return gl_launch_resident(ms, known, mask, phase, phase_per_v, w, out, dist, tnorm, B, V, g, lds, stream);
}

}  // namespace

extern "C" {

int nppc_gl_gap_shape(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span, int* why,
                      int* r, int* span_cap, long* lds_bytes, long* work_bytes) {
  GlGeom g;
  size_t lds, work;
  int y = 0;
  const int rc = gl_geom(B, V, F, T, nfft, hop, L, n_iter, momentum, max_span, &g, &lds, &work, &y);
  if (why) *why = rc == NPPC_OK ? 0 : y;
  if (rc != NPPC_OK) return rc;
  if (r) *r = g.r;
  if (span_cap) *span_cap = g.cap;
  if (lds_bytes) *lds_bytes = (long)lds;
  if (work_bytes) *work_bytes = (long)work;
  return NPPC_OK;
}

int nppc_gl_phase_init(const float* known_spec, const float* mask, float* phase, int B, int T, int nfft, int hop, void* stream) {
  if (!known_spec || !mask || !phase || B <= 0 || B > 65535 || T <= 0 || nfft < 2 || nfft > 512 || hop < 1 || hop > nfft)
    return NPPC_EBADARG;
  const int F = nfft / 2 + 1;
  hipLaunchKernelGGL(gl_phase_init_kernel, dim3(ceil_div((long)F * T, 256), B), dim3(256), 0, (hipStream_t)stream, known_spec,
                     mask, phase, F, T, nfft, hop);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gl_gap(const float* target_mag, const float* known_spec, const float* mask, const float* init_phase,
                int phase_per_variation, float* out, double* dist, double* target_norm, int* status, void* work,
                long work_bytes, int B, int V, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                void* stream) {
  GlMag ms;
  if (gl_mag_target(target_mag, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_run(ms, known_spec, mask, init_phase, phase_per_variation != 0, out, dist, target_norm, status, work, work_bytes, B, V,
                T, nfft, hop, L, n_iter, momentum, max_span, stream);
}

int nppc_gl_gap_pc(const float* pred, const float* pc, const float* mean, const float* stdev, const float* alphas,
                   const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                   double* target_norm, int* status, void* work, long work_bytes, int B, int K, int A, int T, int nfft, int hop,
                   int L, int n_iter, double momentum, int max_span, void* stream) {
  GlMag ms;
  if (gl_mag_pc(pred, pc, mean, stdev, alphas, K, A, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_run(ms, known_spec, mask, init_phase, 0, out, dist, target_norm, status, work, work_bytes, B, K * A + 1, T, nfft, hop,
                L, n_iter, momentum, max_span, stream);
}

int nppc_gl_gap_post(const float* pred, const float* pc, const float* mean, const float* stdev, const float* z,
                     const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                     double* target_norm, int* status, void* work, long work_bytes, int B, int K, int S, int T, int nfft, int hop,
                     int L, int n_iter, double momentum, int max_span, void* stream) {
  GlMag ms;
  if (gl_mag_post(pred, pc, mean, stdev, z, K, S, &ms) != NPPC_OK) return NPPC_EBADARG;
  return gl_run(ms, known_spec, mask, init_phase, 0, out, dist, target_norm, status, work, work_bytes, B, S + 1, T, nfft, hop, L,
                n_iter, momentum, max_span, stream);
}

}  // extern "C"
