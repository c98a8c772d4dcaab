// Per-sample helpers of the direct (any-N) inverse DFT, shared by the any-N iSTFT (inpaint_validator.hip) and both
// Griffin-Lim paths (gl_gap.hip, gl_gap_long.hip).  Those paths are required to agree bit for bit on what they have in
// common; they do because they call these, so the order of the additions below is a contract.
#pragma once
#include "common.h"

// tw[j] = exp(2 pi i j / N), j < N, in fp64; the calling threads stride by nthr
__device__ __forceinline__ void dft_twiddles(double2* tw, int N, int nthr) {
  for (int i = threadIdx.x; i < N; i += nthr) {
    double sn, cs;
    sincospi(2.0 * i / N, &sn, &cs);
    tw[i] = make_double2(cs, sn);
  }
}

// periodic hann window at n, read off the twiddle table
__device__ __forceinline__ double hann_tw(const double2* tw, int n) { return 0.5 - 0.5 * tw[n].x; }

// output sample that padded coordinate p holds under torch's reflect padding (pad < L: one reflection is enough)
__device__ __forceinline__ int reflect_index(int p, int pad, int L) {
  int o = p - pad;
  if (o < 0) o = -o;
  if (o >= L) o = 2 * (L - 1) - o;
  return o;
}

// sample n of N * irfft(sp): bins 1 .. (N - 1) / 2 with their conjugates, twiddles indexed by (k n) mod N in integers;
// bin 0 and (N even) the Nyquist bin enter once, real part only
template <typename Load>
__device__ __forceinline__ double idft_sample(const double2* tw, int N, int n, Load sp) {
  const int kmax = (N - 1) / 2;
  double ar = 0.0, ai = 0.0;
  int idx = n;
  for (int k = 1; k <= kmax; ++k) {
    const double2 w = tw[idx];
    const float2 x = sp(k);
    ar += (double)x.x * w.x;
    ai += (double)x.y * w.y;
    idx += n;
    if (idx >= N) idx -= N;
  }
  double x = (double)sp(0).x + 2.0 * (ar - ai);
  if (!(N & 1)) x += (n & 1) ? -(double)sp(N / 2).x : (double)sp(N / 2).x;
  return x;
}
