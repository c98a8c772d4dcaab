// DNS dynamic mixing on the device (fullsubnet_plus/dataset/dataset_train.py): the room-impulse-response convolution of a
// minibatch and Dataset.snr_mix after it.  Plain HIP for gfx950, wave64, no atomics, no host synchronisation.
#include "common.h"
#include "nppc_hip.h"

// ---------------------------------------------------------------- nppc_rir_convolve
// out[b][n] = sum_{k <= min(n, len_b - 1)} rir[b][k] * clean[b][n - k], len_b = min(rir_len[b], L)
// (= scipy.signal.fftconvolve(clean, rir)[:L], dataset_train.py:151).  Direct form, fp64 throughout: the product of two
// fp32 values is exact in fp64, so an output carries one fp32 rounding at the store and no accumulation error worth the
// name (a plain fp32 running sum is 2e-6 of the peak at 16000 taps, ten times scipy's own fp32 error).
//
// A workgroup of RC_THREADS threads owns RC_NT = 8 * RC_THREADS consecutive outputs of one item; a thread owns 8
// consecutive outputs in fp64 registers.  Taps go in chunks of RC_KC: the chunk (as fp64) and the matching window of
// `clean` (RC_NT + RC_KC floats, zero outside [0, L)) are staged in LDS.  Inside a chunk a thread walks groups of 8 taps
// with a 16-sample register window: one group = 8 LDS floats + 8 broadcast taps for 64 FMAs.  Chunks past the triangle
// (k > n) or past len_b are never staged, so a short RIR costs what it should; a dry item (len 0) is a copy.
// The summation order of an output is k = 0, 1, 2, ...: it depends on nothing but the item's own data.
#define RC_THREADS 128
#define RC_NT (8 * RC_THREADS)
#define RC_KC 512

// acc[j] += h[u] * W[8 + j - u], W = lo (samples 0..7) followed by hi (samples 8..15), taps in ascending order
__device__ __forceinline__ void rc_group(double (&acc)[8], const double (&hi)[8], const double (&lo)[8],
                                         const double* __restrict__ h) {
  double hv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) hv[u] = h[u];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = 8 + j - u;
      acc[j] = fma(hv[u], m < 8 ? lo[m] : hi[m - 8], acc[j]);
    }
  }
}

__device__ __forceinline__ void rc_load8(const float* p, double (&w)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__global__ __launch_bounds__(RC_THREADS) void rir_convolve_kernel(const float* __restrict__ clean,
                                                                   const float* __restrict__ rir,
                                                                   const int* __restrict__ rir_len,
                                                                   float* __restrict__ out, int B, int L, int ldr,
                                                                   int ntiles) {
  __shared__ __attribute__((aligned(16))) float xs[RC_NT + RC_KC];
  __shared__ __attribute__((aligned(16))) double hs[RC_KC];
  // the long tiles (late outputs see the most taps) are dispatched first
  const int b = blockIdx.x % B, tile = ntiles - 1 - blockIdx.x / B, tid = threadIdx.x;
  const int n0 = tile * RC_NT;
  const float* x = clean + (size_t)b * L;
  const float* h = rir + (size_t)b * ldr;
  float* o = out + (size_t)b * L;
  int len = rir_len[b];
  len = len < 0 ? 0 : (len > ldr ? ldr : len);
  len = len > L ? L : len;
  const int nend = n0 + RC_NT < L ? n0 + RC_NT : L;     // outputs [n0, nend)
  if (len == 0) {                                        // dry item: bit-exact copy
    for (int n = n0 + tid; n < nend; n += RC_THREADS) o[n] = x[n];
    return;
  }
  const int kend = len < nend ? len : nend;              // taps [0, kend): k <= n for the tile's last output
  double acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  for (int k0 = 0; k0 < kend; k0 += RC_KC) {
    __syncthreads();                                     // the previous chunk's readers are done
    const int base = n0 - k0 - RC_KC;                    // xs[i] = x[base + i]
    for (int i = tid; i < RC_NT + RC_KC; i += RC_THREADS) {
      const int idx = base + i;
      xs[i] = (idx >= 0 && idx < L) ? x[idx] : 0.f;
    }
    for (int u = tid; u < RC_KC; u += RC_THREADS) hs[u] = (k0 + u < kend) ? (double)h[k0 + u] : 0.0;
    __syncthreads();
    const int taps = kend - k0 < RC_KC ? kend - k0 : RC_KC;
    const int ng = ((taps + 7) / 8 + 1) & ~1;            // groups of 8 taps, an even count (hs is zero past kend)
    const float* xp = xs + RC_KC + 8 * tid;
    double wa[8], wb[8];
    rc_load8(xp, wa);
    for (int g = 0; g < ng; g += 2) {
      rc_load8(xp - 8 * (g + 1), wb);
      rc_group(acc, wa, wb, hs + 8 * g);
      rc_load8(xp - 8 * (g + 2), wa);                    // >= xs + 8 * tid (ng <= RC_KC / 8); the last one is not used
      rc_group(acc, wb, wa, hs + 8 * (g + 1));
    }
  }
  const int n = n0 + 8 * tid;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (n + j < nend) o[n + j] = (float)acc[j];
}

// ---------------------------------------------------------------- nppc_dns_snr_mix
// Dataset.snr_mix after the convolution (dataset_train.py:153-182), eps = 1e-6 in all five places:
//   c1 = c / (max|c| + eps);   c2 = c1 * 10^(T/20) / (rms(c1) + eps)           norm_amplitude, tailor_dB_FS
//   n1, n2 the same for the noise;   n3 = n2 * rms(c2) / 10^(snr/20) / (rms(n2) + eps);   y = c2 + n3
//   s = 10^(T_item/20) / (rms(y) + eps);   y *= s;   c3 = c2 * s
//   any |y| > 0.999:   d = max|y| / (0.99 - eps);   y /= d;   c3 /= d
// One workgroup per clip, three passes over the clip (sums + peaks, mix sums + peak, write); every scalar and every sum
// is fp64 in a fixed order (thread-strided, wave butterfly, waves 0..3), every sample is formed in fp64 from the fp32
// inputs and rounded once, so the result sits within one fp32 rounding of the exact recipe.
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void dns_snr_mix_kernel(const float* __restrict__ clean, const float* __restrict__ noise,
                                                          const float* __restrict__ snr_db,
                                                          const float* __restrict__ noisy_target_dbfs, float target_dbfs,
                                                          float* __restrict__ noisy_out, float* __restrict__ clean_out,
                                                          int L) {
  __shared__ double red[4][4];
  __shared__ double bc[2];
  const double eps = 1e-6;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* c = clean + (size_t)b * L;
  const float* n = noise + (size_t)b * L;
  double sc = 0.0, sn = 0.0, mc = 0.0, mn = 0.0;
  for (int i = tid; i < L; i += 256) {
    const double cv = c[i], nv = n[i];
    sc = fma(cv, cv, sc);
    sn = fma(nv, nv, sn);
    mc = fmax(mc, fabs(cv));
    mn = fmax(mn, fabs(nv));
  }
  sc = wave_sum(sc); sn = wave_sum(sn); mc = wave_max(mc); mn = wave_max(mn);
  if (lane == 0) { red[0][wave] = sc; red[1][wave] = sn; red[2][wave] = mc; red[3][wave] = mn; }
  __syncthreads();
  if (tid == 0) {
    const double t = pow(10.0, (double)target_dbfs / 20.0);
    const double pc = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / L;
    const double pn = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / L;
    const double ac = 1.0 / (fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3])) + eps);   // norm_amplitude
    const double an = 1.0 / (fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3])) + eps);
    const double rc1 = sqrt(pc) * ac, rn1 = sqrt(pn) * an;       // rms after norm_amplitude
    const double sc2 = t / (rc1 + eps), sn2 = t / (rn1 + eps);   // tailor_dB_FS
    const double clean_rms = rc1 * sc2, noise_rms = rn1 * sn2;
    const double snr_scalar = clean_rms / pow(10.0, (double)snr_db[b] / 20.0) / (noise_rms + eps);
    bc[0] = ac * sc2;                                            // clean sample -> c2
    bc[1] = an * sn2 * snr_scalar;                               // noise sample -> n3
  }
  __syncthreads();
  const double gc = bc[0], gn = bc[1];
  double sy = 0.0, my = 0.0;
  for (int i = tid; i < L; i += 256) {
    const double y = fma((double)n[i], gn, (double)c[i] * gc);
    sy = fma(y, y, sy);
    my = fmax(my, fabs(y));
  }
  sy = wave_sum(sy); my = wave_max(my);
  __syncthreads();                                               // bc and red are read above by every thread
  if (lane == 0) { red[0][wave] = sy; red[1][wave] = my; }
  __syncthreads();
  if (tid == 0) {
    const double py = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / L;
    double s = pow(10.0, (double)noisy_target_dbfs[b] / 20.0) / (sqrt(py) + eps);
    const double peak = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3])) * s;
    if (peak > 0.999) s /= peak / (0.99 - eps);                  // is_clipped
    bc[0] = s;
  }
  __syncthreads();
  const double s = bc[0];
  for (int i = tid; i < L; i += 256) {
    const double c2 = (double)c[i] * gc;
    const double y = fma((double)n[i], gn, c2);
    noisy_out[(size_t)b * L + i] = (float)(y * s);
    clean_out[(size_t)b * L + i] = (float)(c2 * s);
  }
}

extern "C" {

int nppc_rir_convolve(const float* clean, const float* rir, const int* rir_len, float* out, int B, int L, int ldr,
                      void* stream) {
  if (!clean || !rir || !rir_len || !out || clean == out || B <= 0 || L <= 0 || ldr <= 0) return NPPC_EBADARG;
  const int ntiles = ceil_div(L, RC_NT);
  if ((long)ntiles * B > 0x7fffffffL) return NPPC_EUNSUPPORTED;
  hipLaunchKernelGGL(rir_convolve_kernel, dim3(ntiles * B), dim3(RC_THREADS), 0, (hipStream_t)stream, clean, rir, rir_len,
                     out, B, L, ldr, ntiles);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_dns_snr_mix(const float* clean, const float* noise, const float* snr_db, const float* noisy_target_dbfs,
                     float target_dbfs, float* noisy_out, float* clean_out, int B, int L, void* stream) {
  if (!clean || !noise || !snr_db || !noisy_target_dbfs || !noisy_out || !clean_out || B <= 0 || L <= 0) return NPPC_EBADARG;
  if (noisy_out == clean || noisy_out == noise || clean_out == clean || clean_out == noise) return NPPC_EBADARG;
  hipLaunchKernelGGL(dns_snr_mix_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, clean, noise, snr_db,
                     noisy_target_dbfs, target_dbfs, noisy_out, clean_out, L);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
