// Batched pYIN f0 tracking (Mauch & Dixon 2014, librosa's parameterisation; specification: tests/pyin_ref.py, DESIGN.md
// section 8b).  Three kernels: cumulative-mean-normalised difference, observation probabilities, Viterbi.  Plain HIP for
// gfx950, wave64, no atomics, no host synchronisation; every sum has one writer and a fixed order, so results repeat bit for
// bit and an item computes the same alone and in a batch.
#include <math.h>

#include "common.h"
#include "nppc_hip.h"

// the restatement's branches are reproduced by doing its fp64 operations one by one: no fused multiply-add unless written
#pragma clang fp contract(off)

#define PY_MAX_FRAME 2048
#define PY_MAX_LAG 1024          // max_period < frame_length - win_length <= 2047, and the scan holds 4 lags per thread
#define PY_MAX_BINS 768          // 2 * bins states: value vectors and tables of the Viterbi kernel stay below 64 KB of LDS
#define PY_MAX_THRESHOLDS 1024
#define PY_TINY 2.2250738585072014e-308

static int py_period_ok(int frame_length, int win_length, int hop_length, int min_period, int max_period) {
  return frame_length >= 2 && frame_length <= PY_MAX_FRAME && win_length >= 1 && win_length < frame_length && hop_length >= 1 &&
         min_period >= 1 && min_period < max_period && max_period < frame_length - win_length && max_period <= PY_MAX_LAG - 1;
}

extern "C" int nppc_pyin_shape(int N, long L, double sr, double fmin, double fmax, int frame_length, int win_length,
                               int hop_length, double resolution, double max_transition_rate, int* T, int* P, int* min_period,
                               int* n_pitch_bins, int* width, long* ws_bytes) {
  if (N < 1 || L < 1 || L > 0x7fffffffL || !(sr > 0.0) || !(fmin > 0.0) || !(fmax > fmin) || !(resolution > 0.0) || !(resolution <= 1.0) ||
      !(max_transition_rate >= 0.0) || frame_length < 2 || frame_length > PY_MAX_FRAME || win_length < 1 || hop_length < 1)
    return NPPC_EBADARG;
  const double lo = floor(sr / fmax), hi = ceil(sr / fmin);
  if (!(lo < 1e9) || !(hi < 1e9)) return NPPC_EBADARG;
  const int minp = lo < 1.0 ? 1 : (int)lo;
  int maxp = (int)hi;
  if (maxp > frame_length - win_length - 1) maxp = frame_length - win_length - 1;
  if (!py_period_ok(frame_length, win_length, hop_length, minp, maxp)) return NPPC_EBADARG;
  const long frames = 1 + L / hop_length;
  if (frames > 0x7fffffffL / 2) return NPPC_EBADARG;
  const int nbps = (int)ceil(1.0 / resolution);
  const double nb = floor(12.0 * nbps * log2(fmax / fmin)) + 1.0;
  if (!(nb >= 1.0) || nb > PY_MAX_BINS) return NPPC_EBADARG;
  const double semis = nearbyint(max_transition_rate * 12.0 * hop_length / sr);   // round half to even
  if (!(semis * nbps < 1e6)) return NPPC_EBADARG;
  if (T) *T = (int)frames;
  if (P) *P = maxp - minp + 1;
  if (min_period) *min_period = minp;
  if (n_pitch_bins) *n_pitch_bins = (int)nb;
  if (width) *width = 2 * (int)semis * nbps + 1;
  if (ws_bytes) *ws_bytes = (long)N * frames * (2 * (long)nb) * (long)sizeof(unsigned short);
  return NPPC_OK;
}

// frames of item n: 1 + len / hop with len = lengths[n] clamped to [0, L] (L where lengths is null), at most T
__device__ __forceinline__ int py_item_len(const int* lengths, int n, long L) {
  if (!lengths) return (int)L;
  const int len = lengths[n];
  return len < 0 ? 0 : (len > L ? (int)L : len);
}

// ---------------------------------------------------------------- nppc_pyin_cmnd
// One workgroup per frame.  The frame (zero padding synthesised) is staged in LDS as fp32; thread `tid` owns the lags
// tid + 1, tid + 257, ...  d(tau) = sum_j (x[j] - x[j + tau])^2: the difference is taken in fp32 (one rounding, relative
// 2^-24 of the difference), squared and accumulated in fp64 in ascending j.  Every term is non-negative, so d(tau) is within
// 2^-23 relative of the exact sum whatever the signal: there is no cancellation to lose digits in, unlike the
// energy-minus-correlation form.  d < 1e-6 -> 0, then the running sum over tau as a workgroup prefix sum in a fixed order
// (4 consecutive lags per thread, Hillis-Steele inside a wave, the waves' totals in ascending order).
#define CM_THREADS 256

__global__ __launch_bounds__(CM_THREADS) void pyin_cmnd_kernel(const float* __restrict__ y, const int* __restrict__ lengths,
                                                                float* __restrict__ dprime, long L, int T, int frame_length,
                                                                int win_length, int hop_length, int min_period,
                                                                int max_period) {
  __shared__ __attribute__((aligned(16))) float xs[PY_MAX_FRAME];
  __shared__ double ds[PY_MAX_LAG];        // ds[tau - 1] = d(tau)
  __shared__ double wtot[CM_THREADS / 64];
  const int n = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
  const int P = max_period - min_period + 1;
  float* out = dprime + ((size_t)n * T + t) * P;
  const int len = py_item_len(lengths, n, L);
  if (t >= 1 + len / hop_length) {         // not a frame of this item
    for (int k = tid; k < P; k += CM_THREADS) out[k] = 0.f;
    return;
  }
  const float* src = y + (size_t)n * L;
  const long s0 = (long)t * hop_length - frame_length / 2;
  const int need = win_length + max_period;                      // < frame_length
  for (int j = tid; j < need; j += CM_THREADS) {
    const long s = s0 + j;
    xs[j] = (s >= 0 && s < len) ? src[s] : 0.f;
  }
  for (int k = tid; k < PY_MAX_LAG; k += CM_THREADS) ds[k] = 0.0;
  __syncthreads();
  for (int tau = tid + 1; tau <= max_period; tau += CM_THREADS) {
    double acc = 0.0;
    const float* xa = xs;
    const float* xb = xs + tau;
#pragma unroll 8
    for (int j = 0; j < win_length; ++j) {
      const double e = (double)(xa[j] - xb[j]);
      acc = fma(e, e, acc);
    }
    ds[tau - 1] = acc < 1e-6 ? 0.0 : acc;
  }
  __syncthreads();
  // inclusive prefix sum of ds[0 .. 1023]
  double v[4];
  double run = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    run += ds[4 * tid + u];
    v[u] = run;
  }
  const int lane = tid & 63, wave = tid >> 6;
  double incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  double base = 0.0;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  base += incl - run;                                            // everything before this thread's 4 lags
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int tau = 4 * tid + u + 1;
    if (tau >= min_period && tau <= max_period) {
      const double d = ds[tau - 1];
      const double mean = (base + v[u]) / (double)tau;
      out[tau - min_period] = (float)(d / (mean + PY_TINY));
    }
  }
}

extern "C" int nppc_pyin_cmnd(const float* y, const int* lengths, float* dprime, int N, long L, int frame_length,
                              int win_length, int hop_length, int min_period, int max_period, void* stream) {
  if (!y || !dprime || N < 1 || L < 1 || L > 0x7fffffffL || !py_period_ok(frame_length, win_length, hop_length, min_period, max_period))
    return NPPC_EBADARG;
  const long T = 1 + L / hop_length;
  if (T * N > 0x7fffffffL) return NPPC_EBADARG;
  pyin_cmnd_kernel<<<dim3((unsigned)(T * N)), dim3(CM_THREADS), 0, (hipStream_t)stream>>>(
      y, lengths, dprime, L, (int)T, frame_length, win_length, hop_length, min_period, max_period);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

// ---------------------------------------------------------------- nppc_pyin_observe
// One wave per frame.  Troughs are compacted in lag order by ballots; trough m's first threshold i_m (the smallest i with
// (double) d' < i / n_thresholds) is found by the same comparison the restatement makes.  For threshold i the troughs below
// it are those with i_m <= i: their count n_i comes from a counting pass, their ranks from a ballot prefix, and the trough of
// rank r adds w_i (1 - e^-l) e^(-l r) / (1 - e^(-l n_i)) to its own accumulator, thresholds ascending.  Thresholds below
// every trough give no_trough_prob w_i to the lowest trough.  Lane 0 then adds the troughs into the pitch-bin histogram in
// lag order.  All of it in fp64; the outputs are rounded to fp32 once.
#define OB_THREADS 64

static size_t ob_lds_bytes_host(int P, int nb, int nth) {
  const int MT = (P + 1) / 2;
  return sizeof(double) * ((size_t)nb + 2 * MT + 1) + sizeof(int) * ((size_t)3 * MT + nth + 1) + sizeof(float) * (size_t)P;
}

__global__ __launch_bounds__(OB_THREADS) void pyin_observe_kernel(const float* __restrict__ dprime,
                                                                   const int* __restrict__ lengths,
                                                                   const double* __restrict__ beta_w, float* __restrict__ obs,
                                                                   float* __restrict__ voiced_prob, int T, long L,
                                                                   int hop_length, int P, int min_period, int nth, int nb,
                                                                   int nbps, double sr, double fmin, double lambda,
                                                                   double no_trough_prob) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ob_smem[];
  const int MT = (P + 1) / 2;
  double* hist = reinterpret_cast<double*>(ob_smem);   // [nb]
  double* prob = hist + nb;                            // [MT]
  double* en = prob + MT;                              // [MT + 1]: e^(-lambda r)
  int* tidx = reinterpret_cast<int*>(en + MT + 1);     // [MT] lag index of trough m
  int* ifirst = tidx + MT;                             // [MT]
  int* tbin = ifirst + MT;                             // [MT]
  int* ncnt = tbin + MT;                               // [nth + 1]
  float* dp = reinterpret_cast<float*>(ncnt + nth + 1);  // [P]

  const int n = blockIdx.x / T, t = blockIdx.x % T, lane = threadIdx.x;
  const size_t row = (size_t)n * T + t;
  float* o = obs + row * (size_t)(2 * nb);
  const int len = py_item_len(lengths, n, L);
  if (t >= 1 + len / hop_length) {
    for (int k = lane; k < 2 * nb; k += OB_THREADS) o[k] = 0.f;
    if (lane == 0) voiced_prob[row] = 0.f;
    return;
  }
  const float* src = dprime + row * (size_t)P;
  for (int k = lane; k < P; k += OB_THREADS) dp[k] = src[k];
  for (int k = lane; k < nb; k += OB_THREADS) hist[k] = 0.0;
  for (int k = lane; k <= MT; k += OB_THREADS) en[k] = exp(-lambda * (double)k);
  __syncthreads();

  // troughs in lag order
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  int ntr = 0;
  for (int base = 0; base < P; base += OB_THREADS) {
    const int k = base + lane;
    bool is = false;
    if (k < P) {
      const float c = dp[k];
      if (k == 0) is = c < dp[1];
      else if (k == P - 1) is = c < dp[k - 1];
      else is = c < dp[k - 1] && c <= dp[k + 1];
    }
    const unsigned long long m = __ballot(is);
    if (is) tidx[ntr + __popcll(m & lt_mask)] = k;
    ntr += __popcll(m);
  }
  __syncthreads();

  // first threshold of every trough, and the lowest trough (lowest lag among equals)
  double hmin = INFINITY;
  int mmin = 0x7fffffff;
  for (int m = lane; m < ntr; m += OB_THREADS) {
    const double h = (double)dp[tidx[m]];
    int i = (int)floor(h * (double)nth) + 1;
    i = i < 1 ? 1 : (i > nth + 1 ? nth + 1 : i);
    while (i > 1 && h < (double)(i - 1) / (double)nth) --i;
    while (i <= nth && !(h < (double)i / (double)nth)) ++i;
    ifirst[m] = i;                                     // nth + 1: below no threshold
    prob[m] = 0.0;
    if (h < hmin) { hmin = h; mmin = m; }              // m ascends per lane: the first minimum stays
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oh = __shfl_xor(hmin, off, 64);
    const int om = __shfl_xor(mmin, off, 64);
    if (oh < hmin || (oh == hmin && om < mmin)) { hmin = oh; mmin = om; }
  }
  __syncthreads();
  for (int i = 1 + lane; i <= nth; i += OB_THREADS) {
    int c = 0;
    for (int m = 0; m < ntr; ++m) c += ifirst[m] <= i ? 1 : 0;
    ncnt[i] = c;
  }
  __syncthreads();

  if (ntr > 0) {
    const double c0 = 1.0 - exp(-lambda);
    double extra = 0.0;
    for (int i = 1; i <= nth; ++i) {
      const int cnt = ncnt[i];
      const double w = beta_w[i - 1];
      if (cnt == 0) { extra += w; continue; }
      const double sc = w / (1.0 - en[cnt]);
      int carry = 0;
      for (int base = 0; base < ntr; base += OB_THREADS) {
        const int m = base + lane;
        const bool below = m < ntr && ifirst[m] <= i;
        const unsigned long long mk = __ballot(below);
        if (below) prob[m] += c0 * en[carry + __popcll(mk & lt_mask)] * sc;
        carry += __popcll(mk);
      }
    }
    // pitch bin of every trough
    for (int m = lane; m < ntr; m += OB_THREADS) {
      const int k = tidx[m];
      double shift = 0.0;
      if (k > 0 && k < P - 1) {
        const double a = (double)dp[k - 1], b = (double)dp[k], c = (double)dp[k + 1];
        const double den = a - 2.0 * b + c;
        if (den != 0.0) {
          shift = (a - c) / (2.0 * den);
          shift = shift < -1.0 ? -1.0 : (shift > 1.0 ? 1.0 : shift);
        }
      }
      const double period = (double)(min_period + k) + shift;
      const double f0 = sr / period;
      double bn = rint((double)(12 * nbps) * log2(f0 / fmin));
      bn = !(bn >= 0.0) ? 0.0 : (bn > (double)(nb - 1) ? (double)(nb - 1) : bn);
      tbin[m] = (int)bn;
      if (m == mmin) prob[m] += no_trough_prob * extra;
    }
    __syncthreads();
    if (lane == 0)
      for (int m = 0; m < ntr; ++m) hist[tbin[m]] += prob[m];
    __syncthreads();
  }
  double part = 0.0;
  for (int k = lane; k < nb; k += OB_THREADS) part += hist[k];
  double vp = wave_sum(part);
  vp = vp < 0.0 ? 0.0 : (vp > 1.0 ? 1.0 : vp);
  const float unv = (float)((1.0 - vp) / (double)nb);
  for (int k = lane; k < nb; k += OB_THREADS) {
    o[k] = (float)hist[k];
    o[nb + k] = unv;
  }
  if (lane == 0) voiced_prob[row] = (float)vp;
}

extern "C" int nppc_pyin_observe(const float* dprime, const int* lengths, const double* beta_w, float* obs, float* voiced_prob,
                                 int N, int T, long L, int hop_length, int P, int min_period, int n_thresholds, int n_pitch_bins,
                                 int bins_per_semitone, double sr, double fmin, double boltzmann, double no_trough_prob,
                                 void* stream) {
  if (!dprime || !beta_w || !obs || !voiced_prob || N < 1 || T < 1 || L < 1 || hop_length < 1 || P < 2 || P > PY_MAX_LAG ||
      min_period < 1 || n_thresholds < 1 || n_thresholds > PY_MAX_THRESHOLDS || n_pitch_bins < 1 ||
      n_pitch_bins > PY_MAX_BINS || bins_per_semitone < 1 || !(sr > 0.0) || !(fmin > 0.0) || !(boltzmann > 0.0) ||
      !(no_trough_prob >= 0.0) || (long)N * T > 0x7fffffffL)
    return NPPC_EBADARG;
  pyin_observe_kernel<<<dim3((unsigned)(N * T)), dim3(OB_THREADS), ob_lds_bytes_host(P, n_pitch_bins, n_thresholds),
                        (hipStream_t)stream>>>(dprime, lengths, beta_w, obs, voiced_prob, T, L, hop_length, P, min_period,
                                               n_thresholds, n_pitch_bins, bins_per_semitone, sr, fmin, boltzmann,
                                               no_trough_prob);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

// ---------------------------------------------------------------- nppc_pyin_viterbi
// One workgroup per waveform, a thread per state (v, j), v = 0 voiced.  The transition matrix is the Kronecker product of
// the 2 x 2 voicing switch and the row-normalised triangular pitch window, so a step factors into
//   a[v, i]  = value[v, i] - log rowsum_i
//   M_v[j]   = max_i (a[v, i] + log tri[j - i + half])      (lowest i among equals)
//   value'[v', j] = max_v (M_v[j] + log switch(v, v')) + log(obs + tiny)   (v = 1 only if strictly larger)
// with additions only: the restatement does the same additions in the same order and so decodes the same path.  The tables
// come from the host in fp64 (hmm_tab = log tri [width], log rowsum [bins], log stay, log switch, log init).
#define VT_MAX_THREADS 1024

static size_t vt_lds_bytes(int nb, int heff) {
  return sizeof(double) * ((size_t)3 * 2 * nb + (2 * heff + 1) + nb) + sizeof(unsigned short) * (size_t)(2 * nb);
}

__global__ __launch_bounds__(VT_MAX_THREADS) void pyin_viterbi_kernel(const float* __restrict__ obs,
                                                                       const int* __restrict__ lengths,
                                                                       const double* __restrict__ hmm_tab,
                                                                       unsigned short* __restrict__ backptr,
                                                                       float* __restrict__ f0, unsigned char* __restrict__ flag,
                                                                       int T, long L, int hop_length, int nb, int nbps, int width,
                                                                       int heff, double fmin) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vt_smem[];
  const int S = 2 * nb, half = width / 2, W = 2 * heff + 1;
  double* val = reinterpret_cast<double*>(vt_smem);    // [S]
  double* av = val + S;                                // [S]
  double* Mv = av + S;                                 // [S]
  double* lt = Mv + S;                                 // [W]: log tri[half - heff ..]
  double* lrow = lt + W;                               // [nb]
  unsigned short* argM = reinterpret_cast<unsigned short*>(lrow + nb);   // [S]

  const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int len = py_item_len(lengths, n, L);
  int Ti = 1 + len / hop_length;
  Ti = Ti > T ? T : Ti;
  const float* ob = obs + (size_t)n * T * S;
  unsigned short* bp = backptr + (size_t)n * T * S;
  const double lstay = hmm_tab[width + nb], lsw = hmm_tab[width + nb + 1], linit = hmm_tab[width + nb + 2];
  for (int k = tid; k < W; k += nthr) lt[k] = hmm_tab[half - heff + k];
  for (int k = tid; k < nb; k += nthr) lrow[k] = hmm_tab[width + k];
  for (int q = tid; q < S; q += nthr) val[q] = linit + log((double)ob[q] + PY_TINY);
  for (int tt = Ti + tid; tt < T; tt += nthr) {        // frames that are not part of this item's chain
    f0[(size_t)n * T + tt] = __builtin_nanf("");
    flag[(size_t)n * T + tt] = 0;
  }
  __syncthreads();
  for (int t = 1; t < Ti; ++t) {
    const float* obt = ob + (size_t)t * S;
    const float ob0 = tid < S ? obt[tid] : 0.f;          // in flight while the maxima are formed
    for (int p = tid; p < S; p += nthr) av[p] = val[p] - lrow[p >= nb ? p - nb : p];
    __syncthreads();
    for (int p = tid; p < S; p += nthr) {
      const int v = p >= nb ? 1 : 0, j = p - v * nb;
      const int ilo = j - heff < 0 ? 0 : j - heff, ihi = j + heff > nb - 1 ? nb - 1 : j + heff;
      const double* a = av + v * nb;
      const double* l = lt + (j + heff);                 // l[-i] = log tri[j - i + half]
      double best = -INFINITY;
      int arg = ilo;
      for (int i = ilo; i <= ihi; ++i) {
        const double c = a[i] + l[-i];
        if (c > best) { best = c; arg = i; }
      }
      Mv[p] = best;
      argM[p] = (unsigned short)arg;
    }
    __syncthreads();
    for (int q = tid; q < S; q += nthr) {
      const int v = q >= nb ? 1 : 0, j = q - v * nb;
      const double c0 = Mv[j] + (v == 0 ? lstay : lsw);
      const double c1 = Mv[nb + j] + (v == 0 ? lsw : lstay);
      const bool take1 = c1 > c0;
      const float o = q == tid ? ob0 : obt[q];
      val[q] = (take1 ? c1 : c0) + log((double)o + PY_TINY);
      bp[(size_t)t * S + q] = (unsigned short)(take1 ? nb + argM[nb + j] : argM[j]);
    }
    // val[q] and av[q] belong to the same thread; Mv is next written after the barrier that follows the av pass
  }
  __syncthreads();                                       // back-pointers and values of every thread are visible
  if (tid == 0) {
    int state = 0;
    double best = val[0];
    for (int q = 1; q < S; ++q)
      if (val[q] > best) { best = val[q]; state = q; }
    const double step = 1.0 / (double)(12 * nbps);
    for (int t = Ti - 1; t >= 0; --t) {
      const bool voiced = state < nb;
      const int b = voiced ? state : state - nb;
      f0[(size_t)n * T + t] = voiced ? (float)(fmin * exp2((double)b * step)) : __builtin_nanf("");
      flag[(size_t)n * T + t] = voiced ? 1 : 0;
      if (t > 0) state = bp[(size_t)t * S + state];
    }
  }
}

extern "C" int nppc_pyin_viterbi(const float* obs, const int* lengths, const double* hmm_tab, unsigned short* backptr,
                                 float* f0, unsigned char* voiced_flag, int N, int T, long L, int hop_length, int n_pitch_bins,
                                 int bins_per_semitone, int width, double fmin, void* stream) {
  if (!obs || !hmm_tab || !backptr || !f0 || !voiced_flag || N < 1 || T < 1 || L < 1 || hop_length < 1 || n_pitch_bins < 1 ||
      n_pitch_bins > PY_MAX_BINS || bins_per_semitone < 1 || width < 1 || (width & 1) == 0 || !(fmin > 0.0))
    return NPPC_EBADARG;
  const int half = width / 2, heff = half < n_pitch_bins - 1 ? half : n_pitch_bins - 1;
  int threads = round_up(2 * n_pitch_bins, 64);
  threads = threads > VT_MAX_THREADS ? VT_MAX_THREADS : threads;
  pyin_viterbi_kernel<<<dim3((unsigned)N), dim3(threads), vt_lds_bytes(n_pitch_bins, heff), (hipStream_t)stream>>>(
      obs, lengths, hmm_tab, backptr, f0, voiced_flag, T, L, hop_length, n_pitch_bins, bins_per_semitone, width, heff, fmin);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}
