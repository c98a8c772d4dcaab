// What the kernels built on the any-N inverse STFT share (inpaint_validator.hip: nppc_istft_any and the PC variations;
// inpaint_posterior.hip: the posterior sampler): the geometry of a workgroup's block of output samples, the frames that
// cover it, the per-sample gather and the host-side geometry / envelope check.  A sampled waveform at a one-hot
// coefficient equals the PC variation bit for bit because both kernels gather through the code below.
#pragma once
#include "common.h"
#include "nppc_hip.h"
#include "stft_core.h"

#include <math.h>
#include <vector>

namespace nppc_isany {

constexpr int IS_S = 256;                 // output samples (= threads) per workgroup
constexpr size_t IS_LDS_MAX = 64 * 1024;

struct IstftGeom {
  int N, F, hop, T;
  int L;      // samples written per item
  int Lk;     // samples that come from the overlap-add, min(L, N + hop (T - 1) - N / 2); [Lk, L) is zero-filled
  int nfr;    // frames a workgroup stages at most
};

// frames [t_lo, t_hi] that cover a padded-coordinate sample of [p0, pend)
__device__ __forceinline__ void frame_range(const IstftGeom& g, int p0, int pend, int* t_lo, int* t_hi) {
  const int a = p0 - g.N + 1;
  *t_lo = a <= 0 ? 0 : (a + g.hop - 1) / g.hop;
  const int b = (pend - 1) / g.hop;
  *t_hi = b < g.T - 1 ? b : g.T - 1;
}

// sample p (padded coordinates) of the overlap-add of the staged spectra spec[t - t_lo][F], divided by the envelope
__device__ __forceinline__ float gather_sample(const IstftGeom& g, const double2* tw, const float2* spec, int t_lo, int t_hi,
                                               int p) {
  const int N = g.N, F = g.F, hop = g.hop;
  const int a = p - N + 1;
  int t0 = a <= 0 ? 0 : (a + hop - 1) / hop;
  int t1 = p / hop;
  t0 = t0 < t_lo ? t_lo : t0;
  t1 = t1 > t_hi ? t_hi : t1;
  double num = 0.0, den = 0.0;
  for (int t = t0; t <= t1; ++t) {
    const int n = p - t * hop;
    const float2* sp = spec + (size_t)(t - t_lo) * F;
    const double x = idft_sample(tw, N, n, [&](int k) { return sp[k]; });
    const double w = hann_tw(tw, n);
    num += w * x;
    den += w * w;
  }
  return (float)(num / (den * (double)N));
}

// geometry + torch's envelope check (window_envelop.abs().min() < 1e-11 inside the kept range raises), on the host
inline int istft_geom(int T, int nfft, int hop, int L, IstftGeom* g, size_t* lds) {
  if (T <= 0 || nfft < 2 || hop < 1 || hop > nfft || L <= 0) return NPPC_EBADARG;
  if (nfft > 512 || (nfft + hop - 1) / hop > 8) return NPPC_EUNSUPPORTED;
  const long full = (long)nfft + (long)hop * (T - 1) - nfft / 2;       // samples the overlap-add reaches after the centre cut
  if (full <= 0) return NPPC_EBADARG;
  g->N = nfft;
  g->F = nfft / 2 + 1;
  g->hop = hop;
  g->T = T;
  g->L = L;
  g->Lk = (int)(L < full ? L : full);
  g->nfr = (IS_S + nfft - 2) / hop + 1;
  *lds = sizeof(double2) * nfft + sizeof(float2) * (size_t)g->nfr * g->F;
  if (*lds > IS_LDS_MAX) return NPPC_EUNSUPPORTED;
  std::vector<double> w2(nfft);
  for (int n = 0; n < nfft; ++n) {
    const double w = 0.5 - 0.5 * cos(2.0 * M_PI * n / nfft);
    w2[n] = w * w;
  }
  // The envelope of a sample depends on p mod hop alone once all ceil-or-floor(N / hop) frames around it exist
  // (N - 1 <= p <= hop (T - 1)), so the first N + hop and the last N + hop kept samples hold every distinct value.
  const long pbeg = nfft / 2, pend = nfft / 2 + g->Lk, span = (long)nfft + hop;
  for (int part = 0; part < 2; ++part) {
    long a = part == 0 ? pbeg : (pend - span > pbeg + span ? pend - span : pbeg + span);
    long b = part == 0 ? (pbeg + span < pend ? pbeg + span : pend) : pend;
    for (long p = a; p < b; ++p) {
      const long lo = p - nfft + 1;
      long t0 = lo <= 0 ? 0 : (lo + hop - 1) / hop, t1 = p / hop;
      if (t1 > T - 1) t1 = T - 1;
      double den = 0.0;
      for (long t = t0; t <= t1; ++t) den += w2[p - t * hop];
      if (den < 1e-11) return NPPC_EBADARG;
    }
  }
  return NPPC_OK;
}

}  // namespace nppc_isany
