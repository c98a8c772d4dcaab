// What the two execution paths of gap-constrained Griffin-Lim share (DESIGN.md sections 8c and 8g): the geometry and
// workspace of the known part, the host launchers of the kernels that stay in gl_gap.hip, the GlMag set-up of the entry
// points, and (device section below) every per-element expression of the iterations (the per-sample helpers of the
// direct DFTs are in stft_core.h).  gl_gap.hip holds the resident path (one workgroup per waveform, the span in LDS),
// gl_gap_long.hip the tiled path (the span in a workspace, one launch per half-iteration).  The tiled path's waveform
// equals the resident path's bit for bit because both kernels of a pair call the helpers below: the order of the
// operations in them is a contract.
#pragma once
#include "common.h"
#include "nppc_hip.h"
#include "stft_core.h"

#include <math.h>

namespace nppc_gl {

constexpr int GL_T = 256;                        // threads of gl_gap_kernel and of every tiled kernel
constexpr int GL_WAVES = GL_T / 64;
constexpr int GL_INFO = 8;                       // ints per item: t_lo, t_hi, s_lo, s_hi, status, has_gap, o_a, o_b
// info[4] names the path that owns the item: GL_RESIDENT (0), GL_REFUSED (1: NaN, status 1) or GL_TILED (2)
constexpr int GL_RESIDENT = 0, GL_REFUSED = 1, GL_TILED = 2;
// how gl_span_kernel routes: by the resident cap alone (the default call), items over it to the tiled path, or every item
constexpr int GL_ROUTE_OFF = 0, GL_ROUTE_OVER = 1, GL_ROUTE_ALL = 2;

struct GlGeom {
  int N, F, hop, T, L;
  int Lk;        // samples the overlap-add reaches, min(L, N + hop (T - 1) - N / 2); [Lk, L) is zero as in torch.istft
  int pad, r;    // N / 2; ceil(N / hop) - 1
  int cap;       // effective span cap (gap bounding range + 2 r)
  int Gmax;      // cap - 2 r: frame slots of C, P, M
  int Pmax;      // (cap - 1) hop + N: padded-coordinate samples of the largest span
  int n_iter, mom;
  double c;      // momentum / (1 + momentum)
};

struct GlWork {
  int* info;       // [B][GL_INFO]
  float* kspec;    // [B][2][F][T]: known spectrum, gap frames zeroed
  float* kwave;    // [B][L]
  double* base;    // [B][Pmax]
  double* den;     // [B][Pmax]: envelope * N; 0 = the sample is zero (past Lk)
};

// where the target magnitude of (item, variation) comes from
struct GlMag {
  const float* target;                       // [B][V][F][T], or null:
  const float *pred, *pc, *mean, *stdev, *alphas;
  int K, A;
  const float* z;                            // [B][S][K] posterior coefficients, or null; then V = S + 1
  int S;
};

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// GlMag and its argument checks for the two routes of the entry points: target magnitudes, or magnitudes formed from a
// prediction and K directions at A alphas (V = K A + 1 variations, the last one alpha = 0)
inline int gl_mag_target(const float* target_mag, GlMag* ms) {
  if (!target_mag) return NPPC_EBADARG;
  *ms = {};
  ms->target = target_mag;
  return NPPC_OK;
}
inline int gl_mag_pc(const float* pred, const float* pc, const float* mean, const float* stdev, const float* alphas, int K, int A,
                     GlMag* ms) {
  if (!pred || !pc || !mean || !stdev || !alphas || K <= 0 || A <= 0 || (long)K * A + 1 > 65535) return NPPC_EBADARG;
  *ms = {};
  ms->pred = pred, ms->pc = pc, ms->mean = mean, ms->stdev = stdev, ms->alphas = alphas, ms->K = K, ms->A = A;
  return NPPC_OK;
}

// magnitudes of posterior samples (csrc/inpaint_posterior.hip states the rule): V = S + 1, v < S:
// exp((pred + sum_k z[b][v][k] pc[b][k]) stdev + mean), v = S: the prediction (z = 0)
inline int gl_mag_post(const float* pred, const float* pc, const float* mean, const float* stdev, const float* z, int K, int S,
                       GlMag* ms) {
  if (!pred || !pc || !mean || !stdev || !z || K <= 0 || K > NPPC_INP_POST_MAX_K || S <= 0 || (long)S + 1 > 65535)
    return NPPC_EBADARG;
  *ms = {};
  ms->pred = pred, ms->pc = pc, ms->mean = mean, ms->stdev = stdev, ms->z = z, ms->K = K, ms->S = S;
  return NPPC_OK;
}

// ---- host side, defined in gl_gap.hip
// -> NPPC_OK or an error with *why: 1 F, 2 frame count, 3 overlap / n_fft limit, 4 n_iter or momentum, 5 anything else
int gl_geom(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span, GlGeom* g,
            size_t* lds, size_t* work, int* why);
GlWork gl_carve(void* work, const GlGeom& g, int B);
// gl_span_kernel (route: GL_ROUTE_*; long_cap: the tiled path's span cap), the known waveform, gl_fill_kernel
int gl_launch_known(const float* known, const float* mask, const GlWork& w, float* out, int* status, int B, int V,
                    const GlGeom& g, int route, int long_cap, void* stream);
// gl_base_kernel for the items whose info[4] == mine, rows of g.Pmax doubles
int gl_launch_base(const float* kspec, const float* mask, const int* info, double* base, double* den, int B, const GlGeom& g,
                   int mine, void* stream);
// gl_gap_kernel
int gl_launch_resident(const GlMag& ms, const float* known, const float* mask, const float* phase, int phase_per_v,
                       const GlWork& w, float* out, double* dist, double* tnorm, int B, int V, const GlGeom& g, size_t lds,
                       void* stream);

// ---- device side: one definition of what gl_gap_kernel and the gl_long_* kernels both compute
// frame t: 1 gap frame, 2 known frame within r frames of a gap frame (the forward transform is compared there), 0 neither
__device__ __forceinline__ int gl_frame_flag(const float* m, int t, int r, int T) {
  int f = 1;
  if (m[t] != 0.f) {
    f = 0;
    const int a = t - r < 0 ? 0 : t - r, e = t + r > T - 1 ? T - 1 : t + r;
    for (int u = a; u <= e; ++u) f = m[u] == 0.f ? 2 : f;
  }
  return f;
}

// GlMag resolved for one (item, variation): rows [F][T]
struct GlMagRow {
  const float* tm;     // target magnitude, or (form) the prediction
  const float* dir;    // PC direction, or null
  const float* ph;     // initial phase
  double alpha, mean, sd;
  bool form;           // magnitude = exp((tm + alpha dir) sd + mean)
  const float* z;      // posterior sample: K coefficients, dir = direction 0 of K rows FT apart; null otherwise
  int K;
  size_t FT;
};

__device__ __forceinline__ GlMagRow gl_mag_row(const GlMag& ms, const float* phase, int phase_per_v, int b, int v, int V, size_t FT) {
  GlMagRow s;
  s.ph = phase + (phase_per_v ? ((size_t)b * V + v) * FT : (size_t)b * FT);
  s.dir = nullptr;
  s.alpha = 0.0, s.mean = 0.0, s.sd = 1.0;
  s.form = !ms.target;
  s.z = nullptr;
  s.K = 0, s.FT = FT;
  if (ms.target)
    s.tm = ms.target + ((size_t)b * V + v) * FT;
  else if (ms.z) {
    s.tm = ms.pred + (size_t)b * FT;
    s.mean = (double)*ms.mean, s.sd = (double)*ms.stdev;
    if (v < ms.S) {
      s.dir = ms.pc + (size_t)b * ms.K * FT;
      s.z = ms.z + ((size_t)b * ms.S + v) * ms.K;
      s.K = ms.K;
    }
  } else {
    s.tm = ms.pred + (size_t)b * FT;
    s.mean = (double)*ms.mean, s.sd = (double)*ms.stdev;
    if (v < ms.K * ms.A) {
      s.dir = ms.pc + ((size_t)b * ms.K + v / ms.A) * FT;
      s.alpha = (double)ms.alphas[v % ms.A];
    }
  }
  return s;
}

// bin k of frame t: the magnitude mg and C_0 = mg exp(i phi0) on a gap frame, zeros on a known one; returns tn + mg^2.
// (The running sum goes in and out by value, here and in gl_project: the product is added where it is formed, so the
// compiler contracts it into the same fused multiply-add in every caller.)
__device__ __forceinline__ double gl_init_bin(double tn, const GlMagRow& s, const float* m, int k, int t, int T, float2& c0,
                                              float& mg) {
  c0 = make_float2(0.f, 0.f);
  mg = 0.f;
  if (m[t] == 0.f) {
    const size_t o = (size_t)k * T + t;
    double mag = (double)s.tm[o];
    if (s.z) {                                                 // the posterior rule: k ascending, fused as the line below compiles
      for (int j = 0; j < s.K; ++j) mag = __builtin_fma((double)s.z[j], (double)s.dir[j * s.FT + o], mag);
      mag = exp(__builtin_fma(mag, s.sd, s.mean));
    } else if (s.form) mag = exp((mag + (s.dir ? s.alpha * (double)s.dir[o] : 0.0)) * s.sd + s.mean);
    mg = (float)mag;
    double sn, cs;
    sincos((double)s.ph[o], &sn, &cs);
    c0 = make_float2((float)((double)mg * cs), (float)((double)mg * sn));
    tn += (double)mg * (double)mg;
  }
  return tn;
}

// frames [t0, t1] of [t_lo, t_hi] whose window reaches padded position p (t0 > t1: none)
__device__ __forceinline__ void gl_reach(int p, int N, int hop, int t_lo, int t_hi, int& t0, int& t1) {
  const int a = p - N + 1;
  t0 = a <= 0 ? 0 : (a + hop - 1) / hop, t1 = p / hop;
  t0 = t0 < t_lo ? t_lo : t0;
  t1 = t1 > t_hi ? t_hi : t1;
}

// the sample at padded position p: (base + sum over the gap frames t of [t0, t1], ascending, of hann * idft) / den;
// is_gap(t) says whether frame t is summed here (known frames are in base), spectrum(t) gives its F bins
template <typename IsGap, typename Spectrum>
__device__ __forceinline__ float gl_synth_sample(const double2* tw, int N, int hop, int p, int t0, int t1, double base, double den,
                                                 IsGap is_gap, Spectrum spectrum) {
  double num = base;
  for (int t = t0; t <= t1; ++t) {
    if (!is_gap(t)) continue;
    const int nn = p - t * hop;
    const float2* sp = spectrum(t);
    num += hann_tw(tw, nn) * idft_sample(tw, N, nn, [&](int k) { return sp[k]; });
  }
  return (float)(num / den);
}

// bin k of the windowed DFT of two frames x0, x1 (N samples each, in LDS) on one twiddle stream: (r0, i0), (r1, i1)
struct GlBinPair { double r0, i0, r1, i1; };

__device__ __forceinline__ GlBinPair gl_dft_pair(const double2* tw, int N, int k, const float* x0, const float* x1) {
  GlBinPair R = {0.0, 0.0, 0.0, 0.0};
  int idx = 0;
  for (int nn = 0; nn < N; ++nn) {
    const double2 w = tw[idx];
    const double hw = hann_tw(tw, nn);
    const double a0 = hw * (double)x0[nn], a1 = hw * (double)x1[nn];
    R.r0 += a0 * w.x;
    R.i0 -= a0 * w.y;
    R.r1 += a1 * w.x;
    R.i1 -= a1 * w.y;
    idx += k;
    if (idx >= N) idx -= N;
  }
  return R;
}

// the projection of R = (rr, ri), bin k of frame t with flag f.  Gap frame (slot s = (t - t_lo) F + k of C, P, M): C takes
// the target magnitude on the phase of R - c P, P takes R (momentum only); known neighbour (element o = k T + t of the
// known spectrum): nothing is written.  Returns dacc + the bin's contribution to d^2.
__device__ __forceinline__ double gl_project(double dacc, int f, double rr, double ri, int s, size_t o, float2* C, float2* P,
                                             const float* M, const float* kre, const float* kim, int mom, double c) {
  if (f == 1) {
    const double mg = (double)M[s];
    const double e = sqrt(rr * rr + ri * ri) - mg;
    dacc += e * e;
    double ar = rr, ai = ri;
    if (mom) {
      const float2 pv = P[s];
      ar -= c * (double)pv.x;
      ai -= c * (double)pv.y;
      P[s] = make_float2((float)rr, (float)ri);
    }
    const double sc = mg / (sqrt(ar * ar + ai * ai) + 1e-16);
    C[s] = make_float2((float)(ar * sc), (float)(ai * sc));
  } else if (f == 2) {
    const double er = rr - (double)kre[o], ei = ri - (double)kim[o];
    dacc += er * er + ei * ei;
  }
  return dacc;
}

}  // namespace nppc_gl
