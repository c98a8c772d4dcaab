// What the two execution paths of gap-constrained Griffin-Lim share (DESIGN.md sections 8c and 8g): the geometry and
// workspace of the known part and the host launchers of the kernels that stay in gl_gap.hip (the per-sample helpers of
// the direct DFTs are in stft_core.h).  gl_gap.hip holds the resident path (one workgroup per waveform, the span in LDS), gl_gap_long.hip
// the tiled path (the span in a workspace, one launch per half-iteration).
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
};

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

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

}  // namespace nppc_gl
