// Speech-enhancement metrics for gfx950: SI-SDR (both reference definitions) and classic STOI (Taal et al. 2011,
// extended=False, the pystoi 0.3 algorithm as DESIGN.md "Speech-enhancement metrics" states it).
//
// Every kernel works on a ragged batch: signals are padded [B][ld] rows with a length per item, and no sample past an
// item's length is read.  Each item's values come from a fixed set of threads in a fixed order that depends only on
// that item (one workgroup per item, or one thread per output sample / one workgroup per STFT frame), so a result is
// bit-identical alone or in any batch, and from run to run: no atomics anywhere.  Everything downstream of the fp32
// input samples is fp64: the resampled signals, the frame energies that decide the silence mask, the DFT and band
// energies, the segment correlations and every reduction.
#include "common.h"
#include "nppc_hip.h"

namespace {

constexpr double EPS64 = 2.220446049250313e-16;       // np.finfo(np.float64).eps
constexpr double CLIP1 = 6.623413251903491;           // 1 + 10^(-BETA / 20), BETA = -15
constexpr int NFRAME = 256, HOPF = 128, NBAND = 15, NSEG = 30, DYN_RANGE = 40;
constexpr int BIN_LO = 7, BIN_HI = 219, NBIN = BIN_HI - BIN_LO;   // only bins 7..218 enter the band matrix
constexpr int SISDR_SUMS = 9;
constexpr int RS_PER_THREAD = 4;                       // resampler outputs per thread (1024 per workgroup)
constexpr int BANDS_FPB = 8;                           // STFT frames per workgroup of the band kernel
constexpr int MAX_TAPS = 4096;                         // resampler taps held in LDS (32 KiB of fp64)

// third-octave band k covers bins [kEdge[k], kEdge[k + 1]) (pystoi thirdoct(10000, 512, 15, 150))
__device__ __constant__ int kEdge[NBAND + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// np.hanning(258)[1:-1] in numpy's form: 0.5 + 0.5 cos(pi n / 257), n = 2 (m + 1) - 257
__device__ __forceinline__ double hann256(int m) { return 0.5 + 0.5 * cospi((double)(2 * (m + 1) - 257) / 257.0); }

// ---- SI-SDR --------------------------------------------------------------------------------------------------------------
// one workgroup per item, three passes over its samples (the mean-removed and residual energies are summed directly, not
// taken from a closed form, so no cancellation):
//   pass 1: sum s, sum e, sum s^2, sum e^2, sum s e               -> a1 = sum s e / sum s^2 (audio_zen)
//   pass 2: sum (s - ms)^2, sum (e - me)(s - ms), sum (e - a1 s)^2 -> a2 = <e~, s~> / (|s~|^2 + 1e-6) (ModelValidator)
//   pass 3: sum (a2 s~ - e~)^2
__global__ __launch_bounds__(256) void sisdr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                    const int* __restrict__ lengths, long ld, double* __restrict__ sums,
                                                    double* __restrict__ out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const long n = min((long)lengths[b], ld);
  const float* s = ref + (long)b * ld;
  const float* e = est + (long)b * ld;
  double ss = 0.0, se = 0.0, sss = 0.0, see = 0.0, sse = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double a = s[i], c = e[i];
    ss += a;
    se += c;
    sss += a * a;
    see += c * c;
    sse += a * c;
  }
  ss = block_sum_waves<4>(ss, red);
  se = block_sum_waves<4>(se, red);
  sss = block_sum_waves<4>(sss, red);
  see = block_sum_waves<4>(see, red);
  sse = block_sum_waves<4>(sse, red);
  const double ms = ss / (double)n, me = se / (double)n, a1 = sse / sss;
  double zss = 0.0, zes = 0.0, r1 = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double a = s[i], c = e[i];
    const double za = a - ms, zc = c - me, d = c - a1 * a;
    zss += za * za;
    zes += zc * za;
    r1 += d * d;
  }
  zss = block_sum_waves<4>(zss, red);
  zes = block_sum_waves<4>(zes, red);
  r1 = block_sum_waves<4>(r1, red);
  const double a2 = zes / (zss + 1e-6);
  double r2 = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double d = a2 * ((double)s[i] - ms) - ((double)e[i] - me);
    r2 += d * d;
  }
  r2 = block_sum_waves<4>(r2, red);
  if (threadIdx.x == 0) {
    if (sums) {
      double* o = sums + (long)b * SISDR_SUMS;
      o[0] = ss; o[1] = se; o[2] = sss; o[3] = see; o[4] = sse; o[5] = zss; o[6] = zes; o[7] = r1; o[8] = r2;
    }
    out[2 * b] = 10.0 * log10(a1 * a1 * sss / r1);                         // +inf when e = a1 s exactly
    out[2 * b + 1] = 20.0 * log10(fabs(a2) * sqrt(zss) / (sqrt(r2) + 1e-6));
  }
}

// ---- polyphase resampler -------------------------------------------------------------------------------------------------
// scipy.signal.resample_poly(x, up, down, window=h): y[j] = sum_i x[i] (up h)[j down + off - i up] over the taps in range,
// off = n_pre_remove down - n_pre_pad; only the nonzero taps of output j's phase are visited.  One thread per output.
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                            long ldx, const double* __restrict__ h, int ntaps, int up, int down,
                                                            long off, double* __restrict__ y, long ldy) {
  extern __shared__ double hs[];
  for (int k = threadIdx.x; k < ntaps; k += 256) hs[k] = h[k] * (double)up;      // scipy: h *= up
  __syncthreads();
  const int b = blockIdx.y;
  const long L = min((long)lengths[b], ldx);
  const long nout = min((L * up + down - 1) / down, ldy);
  const float* xb = x + (long)b * ldx;
  double* yb = y + (long)b * ldy;
#pragma unroll
  for (int r = 0; r < RS_PER_THREAD; ++r) {
    const long j = (long)blockIdx.x * (256 * RS_PER_THREAD) + r * 256 + threadIdx.x;
    if (j >= ldy) break;
    if (j >= nout) {
      yb[j] = 0.0;
      continue;
    }
    const long c = j * down + off;                      // tap index that multiplies x[0]
    const long lo = c - (ntaps - 1);
    const long ilo = lo > 0 ? (lo + up - 1) / up : 0;
    const long ihi = min(c / up, L - 1);
    double acc = 0.0;
    for (long i = ilo; i <= ihi; ++i) acc = fma((double)xb[i], hs[c - i * up], acc);
    yb[j] = acc;
  }
}

// ---- STOI step 2: silent-frame mask and compaction -----------------------------------------------------------------------
// one workgroup per item: energies of frames w x[128 f : 128 f + 256], f < ceil((L - 256) / 128) (range(0, L - 256, 128)),
// one wave per frame; then the item's max, the keep flags (max - 40 - e < 0) and their exclusive scan (ballot + popcount
// inside each wave, wave totals in LDS): slot[f] = kept position or -1, kidx[k] = frame of the k-th kept frame, K = count.
__global__ __launch_bounds__(256) void stoi_frames_kernel(const double* __restrict__ xr, const int* __restrict__ lr, long ldr,
                                                          int nfr, double* __restrict__ energy, int* __restrict__ slot,
                                                          int* __restrict__ kidx, int* __restrict__ K) {
  __shared__ double win[NFRAME];
  __shared__ double red[4];
  __shared__ int wcount[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long L = min((long)lr[b], ldr);
  const int nF = L > NFRAME ? (int)min((L - NFRAME + HOPF - 1) / HOPF, (long)nfr) : 0;
  const double* x = xr + (long)b * ldr;
  double* eb = energy + (long)b * nfr;
  win[tid] = hann256(tid);
  __syncthreads();
  for (int f = wid; f < nF; f += 4) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = lane + 64 * q;
      const double v = win[m] * x[(long)f * HOPF + m];
      acc += v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) eb[f] = 20.0 * log10(sqrt(acc) + EPS64);
  }
  for (int f = nF + tid; f < nfr; f += 256) eb[f] = 0.0;
  __syncthreads();                                      // the energies (global, written by this workgroup) are visible
  double mx = -HUGE_VAL;
  for (int f = tid; f < nF; f += 256) mx = fmax(mx, eb[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wid] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double thr = mx - (double)DYN_RANGE;
  int base = 0;
  for (int f0 = 0; f0 < nfr; f0 += 256) {
    const int f = f0 + tid;
    const bool keep = f < nF && (thr - eb[f]) < 0.0;
    const unsigned long long bal = __ballot(keep);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();                                    // wcount of the previous chunk has been read
    if (lane == 0) wcount[wid] = __popcll(bal);
    __syncthreads();
    int pos = base + below;
    for (int w = 0; w < wid; ++w) pos += wcount[w];
    if (f < nfr) {
      slot[(long)b * nfr + f] = keep ? pos : -1;
      if (keep) kidx[(long)b * nfr + pos] = f;
    }
    base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
  }
  for (int k = base + tid; k < nfr; k += 256) kidx[(long)b * nfr + k] = -1;
  if (tid == 0) K[b] = base;
}

// ---- STOI steps 3-4: third-octave band magnitudes of the silence-removed signals -----------------------------------------
// STFT frame t (t < K - 1) of the overlap-added kept frames is, sample n < 128: kept(t-1)[n + 128] + kept(t)[n], sample
// n >= 128: kept(t)[n] + kept(t+1)[n - 128] (the order numpy's += adds them), kept(k)[m] = w[m] x[128 kidx[k] + m]; it is
// windowed again and transformed by a direct DFT (fp64, twiddles cos/sin(2 pi m / 512) in LDS) for bins 7..218 only, one
// thread per bin and both signals per thread; band energies are summed in bin order.  tob [B][15][nfr].
__global__ __launch_bounds__(256) void stoi_bands_kernel(const double* __restrict__ xr, const double* __restrict__ yr, long ldr,
                                                         const int* __restrict__ kidx, const int* __restrict__ K, int nfr,
                                                         double* __restrict__ xt, double* __restrict__ yt) {
  __shared__ double2 tw[512];
  __shared__ double win[NFRAME];
  __shared__ double ux[NFRAME], uy[NFRAME];
  __shared__ double px[NBIN], py[NBIN];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int T = min(K[b] - 1, nfr - 1);
  const int t0 = blockIdx.x * BANDS_FPB;
  if (t0 >= T) return;                                  // uniform over the workgroup
  for (int m = tid; m < 512; m += 256) {
    double sn, cs;
    sincospi((double)m / 256.0, &sn, &cs);
    tw[m] = make_double2(cs, sn);
  }
  win[tid] = hann256(tid);
  const double* xb = xr + (long)b * ldr;
  const double* yb = yr + (long)b * ldr;
  const int* kb = kidx + (long)b * nfr;
  const int t1 = min(t0 + BANDS_FPB, T);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int n = tid;
    double vx, vy;
    if (n < HOPF) {
      const long p1 = (long)kb[t] * HOPF + n;
      vx = win[n] * xb[p1];
      vy = win[n] * yb[p1];
      if (t >= 1) {
        const long p0 = (long)kb[t - 1] * HOPF + n + HOPF;
        vx = win[n + HOPF] * xb[p0] + vx;
        vy = win[n + HOPF] * yb[p0] + vy;
      }
    } else {
      const long p1 = (long)kb[t] * HOPF + n, p2 = (long)kb[t + 1] * HOPF + n - HOPF;
      vx = win[n] * xb[p1] + win[n - HOPF] * xb[p2];
      vy = win[n] * yb[p1] + win[n - HOPF] * yb[p2];
    }
    ux[n] = win[n] * vx;
    uy[n] = win[n] * vy;
    __syncthreads();
    if (tid < NBIN) {
      const int k = BIN_LO + tid;
      double rx = 0.0, ix = 0.0, ry = 0.0, iy = 0.0;
      int idx = 0;
      for (int m = 0; m < NFRAME; ++m) {
        const double2 w = tw[idx];
        rx = fma(ux[m], w.x, rx);
        ix = fma(ux[m], w.y, ix);
        ry = fma(uy[m], w.x, ry);
        iy = fma(uy[m], w.y, iy);
        idx = (idx + k) & 511;
      }
      px[tid] = rx * rx + ix * ix;
      py[tid] = ry * ry + iy * iy;
    }
    __syncthreads();
    if (tid < 2 * NBAND) {
      const int j = tid % NBAND;
      const double* p = tid < NBAND ? px : py;
      double acc = 0.0;
      for (int q = kEdge[j]; q < kEdge[j + 1]; ++q) acc += p[q - BIN_LO];
      (tid < NBAND ? xt : yt)[((long)b * NBAND + j) * nfr + t] = sqrt(acc);
    }
    // the next frame's ux / uy writes come after this barrier; px / py are rewritten only after the next one
    __syncthreads();
  }
}

// ---- STOI step 5: segment correlations -----------------------------------------------------------------------------------
// one workgroup per item; thread p takes the (band, segment) pairs p, p + 256, ...; every 30-frame segment is normalised,
// clipped, mean-removed and correlated in three fp64 passes; the per-thread sums are folded in a fixed order.
__global__ __launch_bounds__(256) void stoi_corr_kernel(const double* __restrict__ xt, const double* __restrict__ yt,
                                                        const int* __restrict__ K, int nfr, double* __restrict__ out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const int T = min(K[b] - 1, nfr - 1);
  if (T < NSEG) {                                       // uniform over the workgroup
    if (threadIdx.x == 0) out[b] = 1e-5;
    return;
  }
  const int J = T - NSEG + 1;
  double acc = 0.0;
  for (int p = threadIdx.x; p < NBAND * J; p += 256) {
    const int j = p / J, m0 = p % J;
    const long base = ((long)b * NBAND + j) * nfr + m0;
    const double* x = xt + base;
    const double* y = yt + base;
    double sxx = 0.0, syy = 0.0;
    for (int i = 0; i < NSEG; ++i) {
      sxx += x[i] * x[i];
      syy += y[i] * y[i];
    }
    const double nc = sqrt(sxx) / (sqrt(syy) + EPS64);
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < NSEG; ++i) {
      sx += x[i];
      sy += fmin(y[i] * nc, x[i] * CLIP1);
    }
    const double mx = sx / NSEG, my = sy / NSEG;
    double dxx = 0.0, dyy = 0.0, dxy = 0.0;
    for (int i = 0; i < NSEG; ++i) {
      const double dx = x[i] - mx, dy = fmin(y[i] * nc, x[i] * CLIP1) - my;
      dxx += dx * dx;
      dyy += dy * dy;
      dxy += dx * dy;
    }
    acc += dxy / ((sqrt(dyy) + EPS64) * (sqrt(dxx) + EPS64));
  }
  acc = block_sum_waves<4>(acc, red);
  if (threadIdx.x == 0) out[b] = acc / ((double)NBAND * J);
}

}  // namespace

extern "C" {

int nppc_sisdr_sums(const float* ref, const float* est, const int* lengths, int B, long ld, double* sums, double* out,
                    void* stream) {
  if (!ref || !est || !lengths || !out || B <= 0 || ld <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(sisdr_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ref, est, lengths, ld, sums, out);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_resample_poly(const float* x, const int* lengths, int B, long ldx, const double* h, int ntaps, int up, int down,
                       double* y, long ldy, void* stream) {
  if (!x || !lengths || !h || !y || B <= 0 || ldx <= 0 || ldy <= 0 || ntaps <= 0 || up <= 0 || down <= 0)
    return NPPC_EBADARG;
  if (ntaps > MAX_TAPS || B > 65535 || (ldy + 256 * RS_PER_THREAD - 1) / (256 * RS_PER_THREAD) >= (1L << 31))
    return NPPC_EUNSUPPORTED;
  // scipy's alignment: half_len = (ntaps - 1) / 2, n_pre_pad = down - half_len % down,
  // n_pre_remove = (half_len + n_pre_pad) / down; output j is centred on padded tap (j + n_pre_remove) down
  const long half = (ntaps - 1) / 2, pre_pad = down - half % down, pre_remove = (half + pre_pad) / down;
  const long off = pre_remove * down - pre_pad;
  if (off < 0) return NPPC_EUNSUPPORTED;
  const dim3 grid((unsigned)((ldy + 256 * RS_PER_THREAD - 1) / (256 * RS_PER_THREAD)), (unsigned)B);
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(256), ntaps * sizeof(double), (hipStream_t)stream, x, lengths, ldx, h,
                     ntaps, up, down, off, y, ldy);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_stoi_frames(const double* xr, const int* lr, int B, long ldr, int nfr, double* energy, int* slot, int* kidx, int* K,
                     void* stream) {
  if (!xr || !lr || !energy || !slot || !kidx || !K || B <= 0 || ldr <= 0 || nfr <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(stoi_frames_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, xr, lr, ldr, nfr, energy, slot, kidx, K);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_stoi_bands(const double* xr, const double* yr, long ldr, const int* kidx, const int* K, int B, int nfr, double* x_tob,
                    double* y_tob, void* stream) {
  if (!xr || !yr || !kidx || !K || !x_tob || !y_tob || B <= 0 || ldr <= 0 || nfr <= 0) return NPPC_EBADARG;
  if (B > 65535) return NPPC_EUNSUPPORTED;
  const dim3 grid((unsigned)((nfr + BANDS_FPB - 1) / BANDS_FPB), (unsigned)B);
  hipLaunchKernelGGL(stoi_bands_kernel, grid, dim3(256), 0, (hipStream_t)stream, xr, yr, ldr, kidx, K, nfr, x_tob, y_tob);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_stoi_corr(const double* x_tob, const double* y_tob, const int* K, int B, int nfr, double* out, void* stream) {
  if (!x_tob || !y_tob || !K || !out || B <= 0 || nfr <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(stoi_corr_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x_tob, y_tob, K, nfr, out);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
