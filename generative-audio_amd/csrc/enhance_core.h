// Whole-recording enhancement core (nppc_audio/enhance.py; specification tests/enhance_ref.py): plain
// C++ that compiles as __host__ __device__ under hipcc and as ordinary inline functions under any host compiler, so the
// kernels (csrc/enhance_rec.hip), the serial host implementation and the sanitizer program
// (tools/check/enhance_host_check.cc) take every decision with the same text.
//
// A recording of L samples is cut into n chunks of C samples at a hop of H = C / 2 (the last one shorter, but longer than
// H); chunk c comes back from the nets as an enhanced waveform e_c and K direction waveforms p_{c,k}.
//
// 1. Boundary Gram.  Boundary c (1 <= c < n), rows a_j = p_{c-1,j}[H : 2H], b_k = p_{c,k}[0 : H]:
//      G[j][k] = sum a_j b_k, na[j] = sum a_j^2, nb[k] = sum b_k^2, in fp64 (a product of two fp32 values is exact there);
//      cos[j][k] = G / sqrt(na nb), 0 where na nb == 0.  One boundary's sums are ENH_E(K) = K (K + 2) doubles: G row-major,
//      then na, then nb.
// 2. Chain.  perm[0][s] = s, sign[0][s] = +1.  For a later chunk the slots s = 0 .. K - 1 are served in that order; slot s,
//      with j = perm[c-1][s], takes the not-yet-taken k of largest |cos[j][k]| (ties: the lowest k; match "sign": k = j),
//      sign[c][s] = sign[c-1][s] (G[j][k] >= 0 ? +1 : -1), continuity[c-1][s] = |cos[j][k]|.
// 3. Splice, every fp32 operation rounded on its own (no contraction).  Row 0 of the output is y_c = e_c, row 1 + s A + a is
//      y_c = e_c + (alpha_a sign[c][s]) p_{c,perm[c][s]}.  Output sample m: cur = min(m / H, n - 1), i = m - cur H;
//      cur >= 1 and i < H: out = y_prev[i + H] (1 - w[i]) + y_cur[i] w[i]; otherwise out = y_cur[i].
//      w[i] = 0.5 - 0.5 cos(2 pi i / C), i < H, is a table made in fp64 on the host and rounded to fp32.
// 4. Posterior samples (csrc/enhance_post.hip; specification tests/enhance_posterior_ref.py).  Chunk c keeps its planes:
//      pred_crm[c] [2][F][T], w_mat[c] [K][2][F][T], the noisy re[c] / im[c] [F][T] and its length len[c] (C, the last chunk
//      L - (n - 1) H).  The coefficients z [S][K][2] are drawn once for the recording and indexed by slot.  Sample s:
//      mask of chunk c = post_mask (csrc/post_core.h) with the directions in slot order, k ascending over the slots,
//      direction k = sign[c][k] w_mat[c][enh_dir(perm[c][k])] (the negation is exact), in either domain; then
//      cirm_apply_true and the centred inverse STFT of fft_core.h with the ragged rule at len[c] -> y_{c,s}[i].
//      Output sample m, (cur, i) by enh_locate: out = enh_blend(y_{cur-1,s}[i + H], y_{cur,s}[i], w[i]) where the chunk
//      before is blended in, otherwise y_{cur,s}[i].  The sum runs over slots, so a signed permutation of a chunk's raw
//      directions together with the tables the chain then gives performs the same operations on the same values.
//      A workgroup owns a block of `block` consecutive output samples, block dividing H (enh_block_ok): by enh_locate every
//      sample of a block then has the chunk and the blend of the block's first sample, at consecutive i.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ENH_HD __host__ __device__ inline
#else
#define ENH_HD inline
#endif

#define ENH_MAX_K 16           // the engine's cap on the directions
#define ENH_MATCH_GREEDY 0
#define ENH_MATCH_SIGN 1

ENH_HD int ENH_E(int K) { return K * (K + 2); }

// the roundings of the splice: one operation each, never fused with a neighbour into a multiply-add.  clang (hipcc on both
// sides, and as a host compiler): contraction off for these operations, which inlining keeps; any other host compiler: a
// volatile result.
ENH_HD float enh_mul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return a * b;
#else
  volatile float r = a * b;
  return r;
#endif
}
ENH_HD float enh_add(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return a + b;
#else
  volatile float r = a + b;
  return r;
#endif
}

ENH_HD double enh_cos(double g, double na, double nb) {
  const double d = na * nb;
  return d == 0.0 ? 0.0 : g / sqrt(d);
}

// an entry of perm as an index that can be followed: the table comes from device memory, nothing has looked at it
ENH_HD int enh_dir(int k, int K) { return k < 0 ? 0 : (k >= K ? K - 1 : k); }

// one step of the chain.  g: the ENH_E(K) sums of the boundary in front of this chunk; pperm / psign: the chunk before.
ENH_HD void enh_chain_step(const double* g, int K, int match, const int* pperm, const int* psign, int* perm, int* sign,
                           double* cont) {
  const double* na = g + K * K;
  const double* nb = na + K;
  unsigned taken = 0;
  for (int s = 0; s < K; ++s) {
    const int j = enh_dir(pperm[s], K);
    int best = -1;
    double bc = 0.0;
    if (match == ENH_MATCH_SIGN) {
      best = j;
      bc = fabs(enh_cos(g[j * K + j], na[j], nb[j]));
    } else {
      for (int k = 0; k < K; ++k) {
        if ((taken >> k) & 1u) continue;
        const double c = fabs(enh_cos(g[j * K + k], na[j], nb[k]));
        if (best < 0 || c > bc) best = k, bc = c;                  // a NaN never wins, and never leaves best unset
      }
    }
    taken |= 1u << best;
    perm[s] = best;
    sign[s] = g[j * K + best] >= 0.0 ? psign[s] : -psign[s];
    cont[s] = bc;
  }
}

// where output sample m comes from: chunk *cur at sample *i; returns whether chunk *cur - 1 (at *i + H) is blended in
ENH_HD bool enh_locate(long m, int H, int n, int* cur, int* i) {
  long c = m / H;
  if (c > n - 1) c = n - 1;
  *cur = (int)c;
  *i = (int)(m - c * H);
  return c >= 1 && *i < H;
}

// blocks of `block` output samples from m = 0 never straddle a half-chunk: the samples m0 .. m0 + block - 1 of the block at
// m0 (a multiple of block) share cur and the blend of enh_locate(m0), with i = i0, i0 + 1, ...
ENH_HD bool enh_block_ok(int C, int block) { return block > 0 && C >= 2 && !(C & 1) && (C / 2) % block == 0; }

ENH_HD float enh_vary(float e, float as, float p) { return enh_add(e, enh_mul(as, p)); }
ENH_HD float enh_blend(float yp, float yc, float w) { return enh_add(enh_mul(yp, enh_add(1.f, -w)), enh_mul(yc, w)); }

// the arguments the entry points of nppc_enh_splice share (true of the plan: 0 < L - (n - 1) H <= C)
ENH_HD bool enh_plan_ok(int n, int K, int C, long L) {
  if (n < 1 || K < 0 || K > ENH_MAX_K || C < 2 || (C & 1)) return false;
  const long start = (long)(n - 1) * (C / 2);
  return L > start && L - start <= C;
}

struct EnhChunks {
  const float* enh;            // e_c at enh + c e_cs
  const float* pcs;            // p_{c,k} at pcs + c p_cs + k p_ks
  long e_cs, p_cs, p_ks;
  int n, K, C;
  long L;
};

// output sample m of row v (0: enhanced; 1 + s A + a: slot s at alpha a).  perm / sign [n][K], w [C / 2].
ENH_HD float enh_sample(const EnhChunks& q, const float* alphas, int A, const float* w, const int* perm, const int* sign, int v,
                        long m) {
  const int H = q.C / 2;
  int cur, i;
  const bool blend = enh_locate(m, H, q.n, &cur, &i);
  float yc = q.enh[cur * q.e_cs + i];
  float yp = blend ? q.enh[(cur - 1) * q.e_cs + i + H] : 0.f;
  if (v > 0) {
    const int s = (v - 1) / A, a = (v - 1) % A;
    const int kc = enh_dir(perm[cur * q.K + s], q.K);
    yc = enh_vary(yc, enh_mul(alphas[a], (float)sign[cur * q.K + s]), q.pcs[cur * q.p_cs + kc * q.p_ks + i]);
    if (blend) {
      const int kp = enh_dir(perm[(cur - 1) * q.K + s], q.K);
      yp = enh_vary(yp, enh_mul(alphas[a], (float)sign[(cur - 1) * q.K + s]), q.pcs[(cur - 1) * q.p_cs + kp * q.p_ks + i + H]);
    }
  }
  return blend ? enh_blend(yp, yc, w[i]) : yc;
}

// the serial host forms ---------------------------------------------------------------------------------------------------
// the ENH_E(K) sums of boundary c, samples in ascending order
inline void enh_gram_serial(const float* pcs, long p_cs, long p_ks, int K, int C, int c, double* g) {
  const int H = C / 2;
  for (int e = 0; e < ENH_E(K); ++e) g[e] = 0.0;
  for (int j = 0; j < K; ++j) {
    const float* a = pcs + (c - 1) * p_cs + j * p_ks + H;
    for (int k = 0; k < K; ++k) {
      const float* b = pcs + c * p_cs + k * p_ks;
      double acc = 0.0;
      for (int i = 0; i < H; ++i) acc += (double)a[i] * (double)b[i];
      g[j * K + k] = acc;
    }
    const float* b = pcs + c * p_cs + j * p_ks;
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < H; ++i) sa += (double)a[i] * (double)a[i], sb += (double)b[i] * (double)b[i];
    g[K * K + j] = sa;
    g[K * K + K + j] = sb;
  }
}

// perm, sign [n][K]; continuity [n - 1][K]; gram (nullable) [n - 1][ENH_E(K)]
inline void enh_chain_serial(const float* pcs, long p_cs, long p_ks, int n, int K, int C, int match, int* perm, int* sign,
                             double* continuity, double* gram) {
  double g[ENH_MAX_K * (ENH_MAX_K + 2)];
  for (int s = 0; s < K; ++s) perm[s] = s, sign[s] = 1;
  for (int c = 1; c < n; ++c) {
    enh_gram_serial(pcs, p_cs, p_ks, K, C, c, g);
    if (gram)
      for (int e = 0; e < ENH_E(K); ++e) gram[(long)(c - 1) * ENH_E(K) + e] = g[e];
    enh_chain_step(g, K, match, perm + (c - 1) * K, sign + (c - 1) * K, perm + c * K, sign + c * K, continuity + (c - 1) * K);
  }
}

// out [1 + K A][ldo], the first L samples of every row
inline void enh_splice_serial(const EnhChunks& q, const float* alphas, int A, const float* w, const int* perm, const int* sign,
                              float* out, long ldo) {
  const int V = 1 + q.K * A;
  for (int v = 0; v < V; ++v)
    for (long m = 0; m < q.L; ++m) out[v * ldo + m] = enh_sample(q, alphas, A, w, perm, sign, v, m);
}
