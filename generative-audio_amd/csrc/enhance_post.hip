// Posterior samples of a whole recording (nppc_audio/enhance.py sample_chunks; the rule: item 4 of
// csrc/enhance_core.h; specification tests/enhance_posterior_ref.py): the mask build in slot order, the true complex
// product, the centred inverse STFT of the (at most two) chunks under a block and the cross-fade, for S samples, in one launch.
//
// One workgroup = one block of ISTFT_FR * hop output samples of the recording (blockIdx.x) and one tile of consecutive
// samples s (blockIdx.y).  H % (ISTFT_FR * hop) == 0 and nfft / hop in {2, 4, 8} (nfft / 2 is then a multiple of hop): a
// block lies in one half-chunk region and starts on the frame grid of both chunks that reach it.  Per sample the workgroup
// inverts the frames of chunk cur - 1 that reach the block (where that chunk is blended in) through the one LDS transform
// buffer, keeps each thread's outputs in registers, does the same for chunk cur, blends and writes.  perm and sign are read
// from device memory.  No atomics, no workgroup waits for another, every sum in a fixed order: two runs give identical bits.
#include "common.h"
#include "enhance_core.h"
#include "fft_core.h"
#include "nppc_hip.h"
#include "post_core.h"
#include "post_stats.h"

#include <type_traits>

namespace {

static_assert(NPPC_POST_MAX_K == ENH_MAX_K, "the samplers and the chain agree on the most directions");

struct EnhPostArgs {
  const float* pred;           // [n][2][F][T]
  const float* w_mat;          // [n][K][2][F][T]
  const float* re;             // [n][F][T]
  const float* im;
  const float* z;              // [S][K][2]
  const int* perm;             // [n][K]
  const int* sign;
  const float* w;              // [C / 2], hann_table
  float* samples;              // [S][ldo] or null
  double2* tpart;              // [tiles][L] (sum y, sum y^2) or null
  long L, ldo;
  int n, K, S, C, T, hop, spt, domain;
};

template <int LOGN, bool STATS>
__global__ __launch_bounds__(256) void enh_post_kernel(EnhPostArgs a) {
  constexpr int N = 1 << LOGN;
  constexpr int F = N / 2 + 1;
  constexpr int OPT = (ISTFT_FR * (N / 2) + 255) / 256;  // output samples a thread owns at most (hop <= N / 2)
  __shared__ float2 buf[ISTFT_MAXFR][N + 1];
  __shared__ float2 tw[N / 2];
  __shared__ float win[N];
  __shared__ int pm[2][ENH_MAX_K], sg[2][ENH_MAX_K];     // slot -> direction and sign; [0]: chunk cur - 1, [1]: chunk cur
  const int tid = threadIdx.x, tile = blockIdx.y;
  const int T = a.T, hop = a.hop, K = a.K, H = a.C / 2;
  const int ov = N / hop, nfr = ISTFT_FR + ov - 1, BS = ISTFT_FR * hop;
  const long m0 = (long)blockIdx.x * BS;
  const size_t FT = (size_t)F * T;
  int cur, i0;
  const bool blend = enh_locate(m0, H, a.n, &cur, &i0);
  const int s0 = tile * a.spt, s1 = min(a.S, s0 + a.spt);

  fft_tables<LOGN>(tw, win, 1.0);                        // inverse transform: +i
  if (tid < 2 * K) {
    const int side = tid / K, k = tid - side * K, c = cur - 1 + side;
    if (side || blend) {
      pm[side][k] = enh_dir(a.perm[(size_t)c * K + k], K);
      sg[side][k] = a.sign[(size_t)c * K + k];
    }
  }
  float wt[OPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) {
    const int e = tid + i * 256;
    wt[i] = blend && e < BS ? a.w[i0 + e] : 0.f;
  }

  // samples ioff .. ioff + BS - 1 of chunk c, sample zs: the frames that reach them through buf, this thread's outputs to y
  auto invert = [&](int side, int c, int ioff, const float* zs, float (&y)[OPT]) {
    const long len = c == a.n - 1 ? a.L - (long)(a.n - 1) * H : a.C;
    const int Tb = 1 + len / hop < T ? (int)(1 + len / hop) : T;
    const int p0 = ioff + N / 2;                         // first padded-coordinate sample
    const int tfirst = p0 / hop - (ov - 1);              // first frame that can touch [p0, p0 + BS)
    const float* pred = a.pred + (size_t)c * 2 * FT;
    const float* wm = a.w_mat + (size_t)c * K * 2 * FT;
    const float* n_re = a.re + (size_t)c * FT;
    const float* n_im = a.im + (size_t)c * FT;
    __syncthreads();                                     // tables and slots written / the last overlap-add has read buf
    for (int e = tid; e < nfr * F; e += 256) {           // frame fastest: T is the contiguous axis of the planes
      const int j = e % nfr, f = e / nfr, t = tfirst + j;
      float xr = 0.f, xi = 0.f;
      if (t >= 0 && t < Tb) {
        const size_t o = (size_t)f * T + t;
        float dr[ENH_MAX_K], di[ENH_MAX_K];              // the directions of this bin in slot order, signed
#pragma unroll
        for (int k = 0; k < ENH_MAX_K; ++k) {
          if (k < K) {
            const float* d = wm + (size_t)pm[side][k] * 2 * FT + o;
            const bool neg = sg[side][k] < 0;
            dr[k] = neg ? -d[0] : d[0];
            di[k] = neg ? -d[FT] : d[FT];
          }
        }
        float Mr, Mi;
        post_mask(pred[o], pred[FT + o], dr, di, 1, zs, K, a.domain, &Mr, &Mi);
        cirm_apply_true(Mr, Mi, n_re[o], n_im[o], &xr, &xi);
      }
      const bool edge = f == 0 || f == N / 2;            // irfft ignores the imaginary part of DC / Nyquist
      buf[j][__brev((unsigned)f) >> (32 - LOGN)] = make_float2(xr, edge ? 0.f : xi);
      if (!edge) buf[j][__brev((unsigned)(N - f)) >> (32 - LOGN)] = make_float2(xr, -xi);
    }
    __syncthreads();
    fft_stages<LOGN>(buf, tw, nfr);
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
      const int e = tid + i * 256;
      y[i] = e < BS && m0 + e < a.L ? istft_ola<LOGN>(buf, win, p0 + e, tfirst, nfr, Tb, hop) : 0.f;
    }
  };

  double sy[OPT], syy[OPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) sy[i] = syy[i] = 0.0;
  for (int s = s0; s < s1; ++s) {
    const float* zs = a.z + (size_t)s * K * 2;
    float yp[OPT], yc[OPT];
    if (blend) invert(0, cur - 1, i0 + H, zs, yp);
    invert(1, cur, i0, zs, yc);
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
      const int e = tid + i * 256;
      if (e >= BS || m0 + e >= a.L) continue;
      const float y = blend ? enh_blend(yp[i], yc[i], wt[i]) : yc[i];
      if (a.samples) a.samples[(size_t)s * a.ldo + m0 + e] = y;
      if (STATS) {
        sy[i] += (double)y;
        syy[i] += (double)y * (double)y;
      }
    }
  }
  if (!STATS) return;
#pragma unroll
  for (int i = 0; i < OPT; ++i) {
    const int e = tid + i * 256;
    if (e < BS && m0 + e < a.L) a.tpart[(size_t)tile * a.L + m0 + e] = make_double2(sy[i], syy[i]);
  }
}

int enh_post_shape(int n, int S, int K, int C, long L, int T, int nfft, int hop, int stats, long* blocks, int* tiles, int* spt,
                   long* work_bytes) {
  if (!enh_plan_ok(n, K, C, L) || S < 1 || T <= 0 || !post_config_ok(nfft, hop) || nfft / hop < 2 ||
      !enh_block_ok(C, ISTFT_FR * hop) || (stats & ~1))
    return NPPC_EBADARG;
  if (stats && (S < 2 || S > NPPC_POST_MAX_STAT_S)) return NPPC_EBADARG;
  const long nb = (L + ISTFT_FR * hop - 1) / (ISTFT_FR * hop);
  if (nb > 0x7fffffffL) return NPPC_EBADARG;
  int per;
  const long nt = post_tiles(S, nb, stats, &per);
  if (nt > 65535) return NPPC_EBADARG;
  if (blocks) *blocks = nb;
  if (tiles) *tiles = (int)nt;
  if (spt) *spt = per;
  if (work_bytes) *work_bytes = stats ? 16 * nt * L : 0;
  return NPPC_OK;
}

}  // namespace

extern "C" {

int nppc_enh_post_sample_shape(int n, int S, int K, int C, long L, int T, int nfft, int hop, int stats, int* tiles,
                               int* tile_samples, long* work_bytes) {
  return enh_post_shape(n, S, K, C, L, T, nfft, hop, stats, nullptr, tiles, tile_samples, work_bytes);
}

int nppc_enh_post_sample(const float* pred_crm, const float* w_mat, const float* re, const float* im, const float* z,
                         const int* perm, const int* sign, const float* w, int domain, int n, int S, int K, int C, long L,
                         int T, int nfft, int hop, float* samples, long ldo, float* mean, float* std, double* work,
                         long work_bytes, void* stream) {
  if (!pred_crm || !re || !im || (K > 0 && (!w_mat || !z || !perm || !sign)) || (n > 1 && !w) || (!mean) != (!std) ||
      (!samples && !mean) || (samples && ldo < L) || (domain != NPPC_POST_COMPRESSED && domain != NPPC_POST_DECOMPRESSED))
    return NPPC_EBADARG;
  const int stats = mean ? 1 : 0;
  int tiles, spt;
  long blocks, need;
  const int rc = enh_post_shape(n, S, K, C, L, T, nfft, hop, stats, &blocks, &tiles, &spt, &need);
  if (rc != NPPC_OK) return rc;
  if (stats && (!work || work_bytes < need || ((uintptr_t)work & 15))) return NPPC_EBADARG;
  EnhPostArgs a;
  a.pred = pred_crm, a.w_mat = w_mat, a.re = re, a.im = im, a.z = z, a.perm = perm, a.sign = sign, a.w = w;
  a.samples = samples, a.tpart = stats ? (double2*)work : nullptr;
  a.L = L, a.ldo = ldo, a.n = n, a.K = K, a.S = S, a.C = C, a.T = T, a.hop = hop, a.spt = spt, a.domain = domain;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)tiles);
  auto launch = [&](auto logn) {
    if (stats)
      hipLaunchKernelGGL((enh_post_kernel<decltype(logn)::value, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((enh_post_kernel<decltype(logn)::value, false>), grid, dim3(256), 0, st, a);
  };
  switch (nfft) {
    case 64: launch(std::integral_constant<int, 6>()); break;
    case 128: launch(std::integral_constant<int, 7>()); break;
    case 256: launch(std::integral_constant<int, 8>()); break;
    default: launch(std::integral_constant<int, 9>()); break;
  }
  NPPC_CHECK_LAUNCH();
  if (stats) {
    post_finish(a.tpart, (size_t)L, tiles, S, mean, std, st);
    NPPC_CHECK_LAUNCH();
  }
  return NPPC_OK;
}

}  // extern "C"
