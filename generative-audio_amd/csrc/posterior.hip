// Posterior samples from the NPPC directions (nppc_audio/posterior.py; specification
// tests/posterior_ref.py): mask build, true complex product and centred inverse STFT of S samples per item in one launch.
//
// The rule.  pred_crm [B][2][F][T] compressed, w_mat [B][K][2][F][T], noisy re / im [B][F][T], z [B][S][K][2] (a real
// and an imaginary coefficient per direction).  Sample s, bin (f, t), fp32, k ascending, every multiply and add of the
// mask rounded on its own (post_mask below is compiled with contraction off):
//   compressed:    mr = pred_r; mi = pred_i; for k: mr = mr + (zr_k wr_k - zi_k wi_k); mi = mi + (zr_k wi_k + zi_k wr_k);
//                  Mr = decompress_cirm(mr); Mi = decompress_cirm(mi)
//   decompressed:  Mr = decompress_cirm(pred_r); Mi = decompress_cirm(pred_i);
//                  for k: Mr = Mr + (zr_k D(wr_k) - zi_k D(wi_k)); Mi = Mi + (zr_k D(wi_k) + zi_k D(wr_k)),  D = decompress_cirm
// then X = M * noisy by cirm_apply_true (the operations decompress_apply_kernel compiles to, conj_mask = 0) and the inverse
// STFT of istft_kernel: the transform, the overlap-add and the ragged rule are the shared code of fft_core.h.
//
// One workgroup = one block of ISTFT_FR * hop output samples of one item (blockIdx.x, blockIdx.y) and one tile of
// consecutive samples s (blockIdx.z), which it runs one after the other through the one LDS transform buffer.
#include "common.h"
#include "fft_core.h"
#include "nppc_hip.h"
#include "post_core.h"
#include "post_stats.h"

#include <type_traits>

namespace {

constexpr int POST_MAX_K = NPPC_POST_MAX_K;

struct PostArgs {
  const float* pred;
  const float* w;
  const float* re;
  const float* im;
  const float* z;
  const int* lengths;          // null: every item is ld samples long
  float* samples;              // [B][S][ld] or null
  double2* tpart;              // [tiles][B][ld] (sum y, sum y^2) or null
  double2* mpart;              // [tiles][B][F][T] (sum |X|, sum |X|^2) or null
  long ld;
  int K, S, T, hop, spt, domain;
};

template <int LOGN, bool STATS>
__global__ __launch_bounds__(256) void post_sample_kernel(PostArgs a) {
  constexpr int N = 1 << LOGN;
  constexpr int F = N / 2 + 1;
  constexpr int OPT = (ISTFT_FR * N + 255) / 256;      // output samples a thread owns at most (hop <= N)
  constexpr int MPT = (ISTFT_FR * F + 255) / 256;      // bins of the workgroup's own frames a thread owns at most
  __shared__ float2 buf[ISTFT_MAXFR][N + 1];
  __shared__ float2 tw[N / 2];
  __shared__ float win[N];
  const int tid = threadIdx.x, b = blockIdx.y, B = gridDim.y, tile = blockIdx.z;
  const int T = a.T, hop = a.hop, K = a.K, S = a.S;
  const long ld = a.ld;
  const int L = a.lengths ? clampi(a.lengths[b], 0, (int)ld) : (int)ld;
  const int Tb = min(1 + L / hop, T);
  const int ov = N / hop;                              // frames overlapping one sample
  const int nfr = ISTFT_FR + ov - 1;
  const int p0 = blockIdx.x * ISTFT_FR * hop;          // first padded-coordinate sample of this block
  const int tfirst = p0 / hop - (ov - 1);              // first frame that can touch [p0, p0 + FR*hop)
  const int town = tfirst + ov - 1;                    // the ISTFT_FR frames this workgroup owns: town .. town + FR - 1
  const int s0 = tile * a.spt, s1 = min(S, s0 + a.spt);
  const size_t FT = (size_t)F * T;
  const bool dead = p0 - N / 2 >= L && town >= Tb;     // nothing of the item reaches this block

  double sy[OPT], syy[OPT], sm[MPT], smm[MPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) sy[i] = syy[i] = 0.0;
#pragma unroll
  for (int i = 0; i < MPT; ++i) sm[i] = smm[i] = 0.0;

  if (!dead) {
    fft_tables<LOGN>(tw, win, 1.0);                    // inverse transform: +i
    const float* pred_r = a.pred + (size_t)b * 2 * FT;
    const float* w_r = a.w + (size_t)b * K * 2 * FT;
    const float* n_re = a.re + (size_t)b * FT;
    const float* n_im = a.im + (size_t)b * FT;
    // bin f of frame row j of sample s into the transform buffer, Hermitian-extended; returns |X|
    auto build = [&](const float* zs, int j, int f) -> float {
      const int t = tfirst + j;
      float xr = 0.f, xi = 0.f;
      if (t >= 0 && t < Tb) {
        const size_t o = (size_t)f * T + t;
        float Mr, Mi;
        post_mask(pred_r[o], pred_r[FT + o], w_r + o, w_r + FT + o, 2 * FT, zs, K, a.domain, &Mr, &Mi);
        cirm_apply_true(Mr, Mi, n_re[o], n_im[o], &xr, &xi);
      }
      const bool edge = f == 0 || f == N / 2;          // irfft ignores the imaginary part of DC / Nyquist
      buf[j][__brev((unsigned)f) >> (32 - LOGN)] = make_float2(xr, edge ? 0.f : xi);
      if (!edge) buf[j][__brev((unsigned)(N - f)) >> (32 - LOGN)] = make_float2(xr, -xi);
      return spec_mag(xr, xi);
    };
    for (int s = s0; s < s1; ++s) {
      const float* zs = a.z + ((size_t)b * S + s) * K * 2;
      __syncthreads();                                 // tables written / the last sample's overlap-add has read buf
      // the workgroup's own frames, frame fastest (T is the contiguous axis of the planes), then the ov - 1 before them
#pragma unroll
      for (int i = 0; i < MPT; ++i) {
        const int e = tid + i * 256;
        if (e < ISTFT_FR * F) {
          const float m = build(zs, ov - 1 + e % ISTFT_FR, e / ISTFT_FR);
          if (STATS) {
            sm[i] += (double)m;
            smm[i] += (double)m * (double)m;
          }
        }
      }
      for (int e = tid; e < (ov - 1) * F; e += 256) build(zs, e % (ov - 1), e / (ov - 1));
      __syncthreads();
      fft_stages<LOGN>(buf, tw, nfr);
#pragma unroll
      for (int i = 0; i < OPT; ++i) {
        const int e = tid + i * 256;
        const int p = p0 + e, nidx = p - N / 2;
        if (e >= ISTFT_FR * hop || nidx < 0 || nidx >= ld) continue;
        const float y = nidx < L ? istft_ola<LOGN>(buf, win, p, tfirst, nfr, Tb, hop) : 0.f;
        if (a.samples) a.samples[((size_t)b * S + s) * ld + nidx] = y;
        if (STATS) {
          sy[i] += (double)y;
          syy[i] += (double)y * (double)y;
        }
      }
    }
  } else if (a.samples) {
    for (int s = s0; s < s1; ++s)
      for (int e = tid; e < ISTFT_FR * hop; e += 256) {
        const int nidx = p0 + e - N / 2;
        if (nidx >= 0 && nidx < ld) a.samples[((size_t)b * S + s) * ld + nidx] = 0.f;
      }
  }
  if (!STATS) return;
  // this tile's partial sums (zeros where the item has ended: the sums above never left 0 there)
  if (a.tpart) {
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
      const int e = tid + i * 256;
      const int nidx = p0 + e - N / 2;
      if (e < ISTFT_FR * hop && nidx >= 0 && nidx < ld)
        a.tpart[((size_t)tile * B + b) * ld + nidx] = make_double2(sy[i], syy[i]);
    }
  }
  if (a.mpart) {
#pragma unroll
    for (int i = 0; i < MPT; ++i) {
      const int e = tid + i * 256;
      const int t = town + e % ISTFT_FR, f = e / ISTFT_FR;
      if (e < ISTFT_FR * F && t < T) a.mpart[((size_t)tile * B + b) * FT + (size_t)f * T + t] = make_double2(sm[i], smm[i]);
    }
  }
}

// blocks along x: every output sample and every frame has an owner
int post_blocks(int T, int nfft, int hop, long ld) {
  const int by_samples = ceil_div(ld + nfft / 2, (long)ISTFT_FR * hop), by_frames = ceil_div(T, ISTFT_FR);
  return by_samples > by_frames ? by_samples : by_frames;
}

int post_shape(int B, int S, int K, int T, int nfft, int hop, long ld, int stats, int* tiles, int* spt, long* work_bytes) {
  if (B <= 0 || B > 65535 || S < 1 || K < 0 || K > POST_MAX_K || T <= 0 || ld <= 0 || ld > 0x7fffffffL - nfft ||
      !post_config_ok(nfft, hop) || (stats & ~3))
    return NPPC_EBADARG;
  if (stats && (S < 2 || S > NPPC_POST_MAX_STAT_S)) return NPPC_EBADARG;
  int per;
  const long nt = post_tiles(S, (long)B * post_blocks(T, nfft, hop, ld), stats, &per);
  if (nt > 65535) return NPPC_EBADARG;
  if (tiles) *tiles = (int)nt;
  if (spt) *spt = per;
  if (work_bytes) {
    const long F = nfft / 2 + 1;
    *work_bytes = 16 * nt * B * (((stats & 1) ? ld : 0) + ((stats & 2) ? F * T : 0));
  }
  return NPPC_OK;
}

}  // namespace

extern "C" {

int nppc_post_sample_shape(int B, int S, int K, int T, int nfft, int hop, long ld, int stats, int* tiles, int* tile_samples,
                           long* work_bytes) {
  return post_shape(B, S, K, T, nfft, hop, ld, stats, tiles, tile_samples, work_bytes);
}

int nppc_post_sample(const float* pred_crm, const float* w_mat, const float* re, const float* im, const float* z,
                     const int* lengths, int domain, int B, int S, int K, int T, int nfft, int hop, long ld, float* samples,
                     float* mean, float* std, float* mag_mean, float* mag_std, double* work, long work_bytes, void* stream) {
  if (!pred_crm || !re || !im || (K > 0 && (!w_mat || !z)) || (!mean) != (!std) || (!mag_mean) != (!mag_std) ||
      (domain != NPPC_POST_COMPRESSED && domain != NPPC_POST_DECOMPRESSED))
    return NPPC_EBADARG;
  const int stats = (mean ? 1 : 0) | (mag_mean ? 2 : 0);
  if (!samples && !stats) return NPPC_EBADARG;
  int tiles, spt;
  long need;
  const int rc = post_shape(B, S, K, T, nfft, hop, ld, stats, &tiles, &spt, &need);
  if (rc != NPPC_OK) return rc;
  if (stats && (!work || work_bytes < need || ((uintptr_t)work & 15))) return NPPC_EBADARG;
  const long F = nfft / 2 + 1;
  PostArgs a;
  a.pred = pred_crm, a.w = w_mat, a.re = re, a.im = im, a.z = z, a.lengths = lengths, a.samples = samples;
  a.tpart = mean ? (double2*)work : nullptr;
  a.mpart = mag_mean ? (double2*)work + (mean ? (size_t)tiles * B * ld : 0) : nullptr;
  a.ld = ld, a.K = K, a.S = S, a.T = T, a.hop = hop, a.spt = spt, a.domain = domain;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(post_blocks(T, nfft, hop, ld), B, tiles);
  auto launch = [&](auto logn) {
    if (stats)
      hipLaunchKernelGGL((post_sample_kernel<decltype(logn)::value, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((post_sample_kernel<decltype(logn)::value, false>), grid, dim3(256), 0, st, a);
  };
  switch (nfft) {
    case 64: launch(std::integral_constant<int, 6>()); break;
    case 128: launch(std::integral_constant<int, 7>()); break;
    case 256: launch(std::integral_constant<int, 8>()); break;
    default: launch(std::integral_constant<int, 9>()); break;
  }
  NPPC_CHECK_LAUNCH();
  if (mean) post_finish(a.tpart, (size_t)B * ld, tiles, S, mean, std, st);
  if (mag_mean) post_finish(a.mpart, (size_t)B * F * T, tiles, S, mag_mean, mag_std, st);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
