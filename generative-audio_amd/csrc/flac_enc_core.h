// FLAC encoder core (specification tests/flac_enc_ref.py, which feeds the rule below to
// tests/flac_ref.py's encoder): plain C++ that compiles as __host__ __device__ under hipcc and as ordinary inline functions
// under any host compiler, so the serial host encoder, the device kernels (csrc/flac_enc.hip) and the sanitizer program
// (tools/check/flac_enc_host_check.cc) take every decision with the same text.
//
// The stream: fLaC, one STREAMINFO (last), frames of a fixed block size (the last one shorter).  Lossless, fixed predictors
// (and, on request, LPC: below), no escape partitions, no wasted bits.  The decision rule, a function of the samples alone:
//   subframe of width b: constant when all samples are equal; else for o = 0..min(4, bs) and p = 0..min(8, ctz(bs)) with
//   (bs >> p) >= o, every partition takes the Rice parameter k (0..14 method 0, 0..30 method 1; lowest on ties) of the
//   smallest exact bit count sum(u >> k) + cnt (1 + k), u = zigzag(residual); cost = 8 + o b + 6 + sum(pbits + bits);
//   cheapest (o, p), ties to the lower o then the lower p; verbatim when that cost >= 8 + bs b.
//   stereo: L, R, M = (L + R) >> 1, S = L - R costed as above; cheapest of 0 (L,R), 1 (L,S), 2 (S,R), 3 (M,S), lowest on ties.
// sum(u >> k) is additive over sub-partitions: the sums of the finest partition order are merged upward.
//
// predictor "lpc" (specification tests/flac_lpc_ref.py) adds candidates of order m = 1..min(M, bs),
// 1 <= M <= 12, to the fixed ones of a non-constant subframe of block bs:
//   1. window, integers only: N = bs + 1, d_i = 2 i - (bs - 1), w_i = floor(2^15 (N^2 - d_i^2) / N^2) (Welch, Q15),
//      x_i = (s_i w_i) >> 15, an arithmetic shift in int64
//   2. r_l = sum_i x_i x_{i+l} in int64, l = 0..M (an empty sum, l >= bs, is 0); r_0 == 0: no LPC candidates
//   3. Levinson-Durbin in fp64 on (double) r_l, every product, sum and quotient rounded on its own (contraction off):
//        err = r_0;  order m:  acc = r_m;  for j = 0..m-2: acc = acc - a_j r_{m-1-j};  k = acc / err
//        k not finite or |k| >= 1: this order and every higher one are no candidates
//        t_j = a_j - k a_{m-2-j} (j = 0..m-2), t_{m-1} = k;  err = err (1 - k k)
//        err not finite or <= 0: this order and every higher one are no candidates;  a = t, the coefficients of order m
//   4. precision P = 12 (bps <= 16) or 15; shift = the largest s in 0..15 with floor(max|a_j| 2^s + 0.5) <= 2^(P-1) - 1, none:
//      the order is no candidate; q_j = floor(a_j 2^shift + 0.5) clamped to [-2^(P-1), 2^(P-1) - 1], no error feedback
//   5. e_i = s_i - ((sum_j q_j s_{i-1-j}) >> shift), the sum in int64, as the decoder forms it; any e_i outside
//      [-2^28, 2^28): the order is no candidate
//   6. partition orders and parameters as for the fixed orders; cost = 8 + m b + 4 + 5 + m P + 6 + sum(pbits + bits)
//   7. the cheapest of all fixed (o, p) and LPC (m, p); ties to fixed before LPC, then the lower order, then the lower p;
//      constant and the verbatim comparison as above; stereo costs L, R, M, S with the larger candidate set.
// The fixed candidates stay in the set: an LPC frame is never longer than the fixed frame of the same samples.
//
// Safety rules: the bit writer ORs into a zero-filled buffer and touches only bytes that receive a one bit, all of which
// lie inside the frame's exact length; every loop is bounded by the block size, 256 partitions or 31 parameters.
#pragma once
#include <stdint.h>

#include "flac_core.h"
#include "md5_core.h"

#define FLAC_ENC_MIN_BS 16
#define FLAC_ENC_MAX_BS 4608
#define FLAC_ENC_PARTS 256       // 2^8: the finest partition order tried
#define FLAC_ENC_STREAM_HEAD 42  // fLaC + block header + STREAMINFO
#define FLAC_ENC_MAX_LPC 12      // the subset's limit up to 48 kHz
#define FLAC_ENC_LAGS (FLAC_ENC_MAX_LPC + 1)
#define FLAC_ENC_CANDS (5 + FLAC_ENC_MAX_LPC)      // fixed 0..4, then LPC 1..12

struct FlacEncSub {
  int type;                      // 0 constant, 1 verbatim, 2 fixed, 3 LPC
  int order, porder;
  long bits;                     // the subframe's exact length
  int shift, precision;          // LPC only
  int qlp[FLAC_ENC_MAX_LPC];
};

// the LPC candidates of one subframe: shift[m - 1] < 0: order m is no candidate
struct FlacEncLpcTab {
  int shift[FLAC_ENC_MAX_LPC];
  int qlp[FLAC_ENC_MAX_LPC][FLAC_ENC_MAX_LPC];
};

FLAC_HD bool flac_enc_bps_ok(int bps) { return bps == 8 || bps == 12 || bps == 16 || bps == 20 || bps == 24; }
FLAC_HD int flac_enc_kmax(int method) { return method ? 30 : 14; }
FLAC_HD int flac_enc_pbits(int method) { return method ? 5 : 4; }
FLAC_HD int flac_enc_pmax(int bs) {
  int p = 0;
  while (p < 8 && !((bs >> p) & 1)) ++p;
  return p;
}

// s points AT sample i; reads s[-1 .. -o].  |s| <= 2^24 keeps every residual inside 2^28.
FLAC_HD int32_t flac_enc_residual(const int32_t* s, int o) {
  switch (o) {
    case 0: return s[0];
    case 1: return s[0] - s[-1];
    case 2: return s[0] - 2 * s[-1] + s[-2];
    case 3: return s[0] - 3 * s[-1] + 3 * s[-2] - s[-3];
    default: return s[0] - 4 * s[-1] + 6 * s[-2] - 4 * s[-3] + s[-4];
  }
}
// the LPC residual as the decoder forms it (flac_core.h: flac_predict), in int64
FLAC_HD int64_t flac_enc_lpc_residual(const int32_t* s, int m, const int* q, int shift) {
  int64_t sum = 0;
  for (int j = 0; j < m; ++j) sum += (int64_t)q[j] * (int64_t)s[-1 - j];
  return (int64_t)s[0] - (sum >> shift);
}
FLAC_HD bool flac_enc_residual_ok(int64_t e) { return e >= -((int64_t)1 << 28) && e < ((int64_t)1 << 28); }
FLAC_HD uint32_t flac_enc_zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// the parameter of one partition from its sums[k * stride] = sum(u >> k): the exact bit count, lowest k on ties
FLAC_HD uint64_t flac_enc_best_k(const uint64_t* sums, int stride, int cnt, int kmax, int* kbest) {
  uint64_t best = 0;
  int kb = 0;
  for (int k = 0; k <= kmax; ++k) {
    const uint64_t bits = sums[(long)k * stride] + (uint64_t)cnt * (uint64_t)(1 + k);
    if (k == 0 || bits < best) best = bits, kb = k;
  }
  *kbest = kb;
  return best;
}

// rice[o * 9 + p] = sum over the partitions of (pbits + partition bits), for every valid (o, p) -> the subframe
FLAC_HD void flac_enc_pick(const uint64_t* rice, int bs, int b, FlacEncSub* out) {
  const int maxo = bs < 4 ? bs : 4, pmax = flac_enc_pmax(bs);
  uint64_t best = 0;
  int have = 0;
  for (int o = 0; o <= maxo; ++o)
    for (int p = 0; p <= pmax; ++p) {
      if ((bs >> p) < o) continue;
      const uint64_t cost = 8 + (uint64_t)o * b + 6 + rice[o * 9 + p];
      if (!have || cost < best) best = cost, out->order = o, out->porder = p, have = 1;
    }
  const uint64_t verbatim = 8 + (uint64_t)bs * b;
  if (best >= verbatim) out->type = 1, out->order = 0, out->porder = 0, out->bits = (long)verbatim;
  else out->type = 2, out->bits = (long)best;
}

// the same over the larger set: rice[c * 9 + p], c = o for the fixed orders and 4 + m for the LPC orders of tab.  Strict
// comparisons in this order of visits are the tie rule: fixed before LPC, the lower order, the lower p.
FLAC_HD void flac_enc_pick_lpc(const uint64_t* rice, int bs, int b, int P, int max_order, const FlacEncLpcTab* tab,
                               FlacEncSub* out) {
  const int maxo = bs < 4 ? bs : 4, pmax = flac_enc_pmax(bs), top = max_order < bs ? max_order : bs;
  uint64_t best = 0;
  int have = 0, lpc = 0;
  for (int c = 0; c <= 4 + top; ++c) {
    const int o = c <= 4 ? c : c - 4;
    if (c <= 4 ? c > maxo : tab->shift[o - 1] < 0) continue;
    const uint64_t head = c <= 4 ? 8 + (uint64_t)o * b + 6 : 8 + (uint64_t)o * b + 4 + 5 + (uint64_t)o * P + 6;
    for (int p = 0; p <= pmax; ++p) {
      if ((bs >> p) < o) continue;
      const uint64_t cost = head + rice[c * 9 + p];
      if (!have || cost < best) best = cost, out->order = o, out->porder = p, lpc = c > 4, have = 1;
    }
  }
  const uint64_t verbatim = 8 + (uint64_t)bs * b;
  if (best >= verbatim) {
    out->type = 1, out->order = 0, out->porder = 0, out->bits = (long)verbatim;
    return;
  }
  out->type = lpc ? 3 : 2, out->bits = (long)best;
  if (lpc) {
    out->shift = tab->shift[out->order - 1], out->precision = P;
    for (int j = 0; j < out->order; ++j) out->qlp[j] = tab->qlp[out->order - 1][j];
  }
}

FLAC_HD void flac_enc_constant(int b, FlacEncSub* out) { out->type = 0, out->order = 0, out->porder = 0, out->bits = 8 + b; }

// bits of the four candidates L, R, M, S -> the assignment; *bits = the two subframes' length
FLAC_HD int flac_enc_pick_assign(const long* c, long* bits) {
  const long a[4] = {c[0] + c[1], c[0] + c[3], c[3] + c[1], c[2] + c[3]};
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (a[i] < a[best]) best = i;
  *bits = a[best];
  return best;
}
// which candidate (0 L, 1 R, 2 M, 3 S) the coded channel c of an assignment is
FLAC_HD int flac_enc_cand(int assign, int c) {
  if (c == 0) return assign == 2 ? 3 : assign == 3 ? 2 : 0;
  return assign == 0 || assign == 2 ? 1 : 3;
}
FLAC_HD int32_t flac_enc_cand_sample(int cand, int32_t l, int32_t r) {
  return cand == 0 ? l : cand == 1 ? r : cand == 2 ? (l + r) >> 1 : l - r;
}

// ------------------------------------------------------------------------------------------------------ LPC analysis
FLAC_HD int flac_enc_lpc_precision(int bps) { return bps <= 16 ? 12 : 15; }
// the Welch window in Q15: 0 < N^2 - d^2 <= N^2, so the quotient is a floor and at most 2^15
FLAC_HD int32_t flac_enc_window(int i, int bs) {
  const int64_t N = (int64_t)bs + 1, d = 2 * (int64_t)i - ((int64_t)bs - 1);
  return (int32_t)((((int64_t)1 << 15) * (N * N - d * d)) / (N * N));
}
FLAC_HD int32_t flac_enc_windowed(int32_t s, int i, int bs) { return (int32_t)(((int64_t)s * flac_enc_window(i, bs)) >> 15); }

// r[0 .. FLAC_ENC_MAX_LPC] of the windowed block x; |x| <= 2^24 and bs <= 4608 keep every sum under 2^61
FLAC_HD void flac_enc_autocorr(const int32_t* x, int bs, int64_t* r) {
  for (int l = 0; l < FLAC_ENC_LAGS; ++l) {
    int64_t acc = 0;
    for (int i = 0; i + l < bs; ++i) acc += (int64_t)x[i] * (int64_t)x[i + l];
    r[l] = acc;
  }
}

FLAC_HD bool flac_enc_finite(double v) { return v - v == 0.0; }     // false for NaN and the infinities
FLAC_HD double flac_enc_round_half_up(double v) { return __builtin_floor(v + 0.5); }

// Levinson-Durbin and the quantiser (steps 3 and 4 of the rule): r -> tab, for orders 1..min(max_order, bs).  ws: two rows of
// FLAC_ENC_MAX_LPC doubles.  A few hundred operations, serial.
FLAC_HD void flac_enc_lpc_table(const int64_t* r, int bs, int max_order, int P, FlacEncLpcTab* tab, double* ws) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int m = 0; m < FLAC_ENC_MAX_LPC; ++m) tab->shift[m] = -1;
  if (r[0] == 0) return;
  const int top = max_order < bs ? max_order : bs;
  const double lim = (double)((1 << (P - 1)) - 1), low = -(double)(1 << (P - 1));
  double* a = ws;
  double* t = ws + FLAC_ENC_MAX_LPC;
  double err = (double)r[0];
  for (int m = 1; m <= top; ++m) {
    double acc = (double)r[m];
    for (int j = 0; j < m - 1; ++j) {
      const double prod = a[j] * (double)r[m - 1 - j];
      acc = acc - prod;
    }
    const double k = acc / err;
    if (!flac_enc_finite(k) || !((k < 0 ? -k : k) < 1.0)) return;
    for (int j = 0; j < m - 1; ++j) {
      const double prod = k * a[m - 2 - j];
      t[j] = a[j] - prod;
    }
    t[m - 1] = k;
    const double kk = k * k;
    const double one = 1.0 - kk;
    err = err * one;
    if (!flac_enc_finite(err) || !(err > 0.0)) return;
    double cmax = 0.0;
    for (int j = 0; j < m; ++j) {
      a[j] = t[j];
      const double c = a[j] < 0 ? -a[j] : a[j];
      if (c > cmax) cmax = c;
    }
    int shift = -1;
    for (int s = 15; s >= 0 && shift < 0; --s)
      if (flac_enc_round_half_up(cmax * (double)(1 << s)) <= lim) shift = s;
    if (shift < 0) continue;                                        // too large for the precision: this order only
    tab->shift[m - 1] = shift;
    for (int j = 0; j < m; ++j) {
      double q = flac_enc_round_half_up(a[j] * (double)(1 << shift));
      q = q < low ? low : q > lim ? lim : q;
      tab->qlp[m - 1][j] = (int)q;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- headers
FLAC_HD int flac_enc_bs_code(int bs) {
  if (bs == 192) return 1;
  for (int c = 2; c < 6; ++c)
    if (bs == (576 << (c - 2))) return c;
  for (int c = 8; c < 16; ++c)
    if (bs == (256 << (c - 8))) return c;
  return bs <= 256 ? 6 : 7;
}
FLAC_HD int flac_enc_rate_code(int rate) {
  const int t[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  for (int c = 1; c < 12; ++c)
    if (t[c] == rate) return c;
  return 0;
}
FLAC_HD int flac_enc_size_code(int bps) { return bps == 8 ? 1 : bps == 12 ? 2 : bps == 16 ? 4 : bps == 20 ? 5 : 6; }

// the frame header with its CRC-8 into h (at most 14 bytes); returns its length
FLAC_HD int flac_enc_frame_header(uint8_t* h, int bs, int rate, int channels, int assign, int bps, uint64_t number) {
  const int bsc = flac_enc_bs_code(bs);
  h[0] = 0xff, h[1] = 0xf8;
  h[2] = (uint8_t)((bsc << 4) | flac_enc_rate_code(rate));
  h[3] = (uint8_t)(((assign ? 7 + assign : channels - 1) << 4) | (flac_enc_size_code(bps) << 1));
  int i = 4;
  if (number < 0x80) {
    h[i++] = (uint8_t)number;
  } else {
    int n = 2;
    while (n < 7 && number >= ((uint64_t)1 << (5 * n + 1))) ++n;
    h[i++] = (uint8_t)((0xff00u >> n) | (unsigned)(n < 7 ? number >> (6 * (n - 1)) : 0));
    for (int j = n - 2; j >= 0; --j) h[i++] = (uint8_t)(0x80 | ((number >> (6 * j)) & 0x3f));
  }
  if (bsc == 6) h[i++] = (uint8_t)(bs - 1);
  if (bsc == 7) h[i++] = (uint8_t)((bs - 1) >> 8), h[i++] = (uint8_t)(bs - 1);
  h[i] = (uint8_t)flac_crc8(h, i);
  return i + 1;
}

FLAC_HD void flac_enc_stream_header(uint8_t* h, int block_size, long min_frame, long max_frame, int rate, int channels, int bps,
                                    long total, const uint8_t* md5) {
  h[0] = 'f', h[1] = 'L', h[2] = 'a', h[3] = 'C';
  h[4] = 0x80, h[5] = 0, h[6] = 0, h[7] = 34;
  uint8_t* s = h + 8;
  s[0] = s[2] = (uint8_t)(block_size >> 8), s[1] = s[3] = (uint8_t)block_size;
  s[4] = (uint8_t)(min_frame >> 16), s[5] = (uint8_t)(min_frame >> 8), s[6] = (uint8_t)min_frame;
  s[7] = (uint8_t)(max_frame >> 16), s[8] = (uint8_t)(max_frame >> 8), s[9] = (uint8_t)max_frame;
  s[10] = (uint8_t)(rate >> 12), s[11] = (uint8_t)(rate >> 4);
  s[12] = (uint8_t)(((rate & 15) << 4) | ((channels - 1) << 1) | ((bps - 1) >> 4));
  s[13] = (uint8_t)((((bps - 1) & 15) << 4) | ((total >> 32) & 15));
  s[14] = (uint8_t)(total >> 24), s[15] = (uint8_t)(total >> 16), s[16] = (uint8_t)(total >> 8), s[17] = (uint8_t)total;
  for (int i = 0; i < 16; ++i) s[18 + i] = md5[i];
}

// the verbatim bound of one frame and of a stream
FLAC_HD long flac_enc_frame_bound(int bs, int channels, int bps) {
  const long side = channels == 2 ? 1 : 0;
  return 14 + ((long)channels * 8 + (long)bs * ((long)channels * bps + side) + 7) / 8 + 2;
}
FLAC_HD long flac_enc_frames(long n, int block_size) { return (n + block_size - 1) / block_size; }
FLAC_HD long flac_enc_bound(long n, int channels, int bps, int block_size) {
  const long full = n / block_size, rest = n - full * block_size;
  return FLAC_ENC_STREAM_HEAD + full * flac_enc_frame_bound(block_size, channels, bps) +
         (rest ? flac_enc_frame_bound((int)rest, channels, bps) : 0);
}

// ---------------------------------------------------------------------------------------------------------------- CRC-16
FLAC_HD unsigned flac_enc_crc16_step(unsigned c, unsigned byte) {       // flac_crc16's step
  const unsigned x = (c >> 8) ^ byte;
  unsigned par = x ^ (x >> 4);
  par ^= par >> 2;
  par ^= par >> 1;
  return ((c << 8) ^ (x << 1) ^ (x << 2) ^ ((par & 1u) ? 0x8003u : 0u)) & 0xffffu;
}
FLAC_HD unsigned flac_enc_gf_mul(unsigned a, unsigned b) {              // a b mod x^16 + x^15 + x^2 + 1
  unsigned r = 0;
  for (int i = 15; i >= 0; --i) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x18005u;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// the CRC (init 0) of A || B from crc(A), crc(B) and B's length: crc(A) x^(8 |B|) + crc(B)
FLAC_HD unsigned flac_enc_crc16_shift(unsigned crc, long nbytes) {
  unsigned base = 0x100u, r = 1u;
  for (long m = nbytes; m > 0; m >>= 1) {
    if (m & 1) r = flac_enc_gf_mul(r, base);
    base = flac_enc_gf_mul(base, base);
  }
  return flac_enc_gf_mul(crc, r);
}

// ------------------------------------------------------------------------------------------------------- serial encoder
struct FlacBitWriter {           // big-endian, ORs into a zero-filled buffer
  uint8_t* p;
  long bit;
  FLAC_HD void put(uint32_t v, int n) {                                 // 0 <= n <= 32, v < 2^n
    if (n <= 0) return;
    const long byte = bit >> 3;
    uint64_t x = (uint64_t)v << (64 - n - (int)(bit & 7));
    for (int i = 0; x; ++i, x <<= 8) p[byte + i] |= (uint8_t)(x >> 56);
    bit += n;
  }
  FLAC_HD void put_signed(int32_t v, int n) { put((uint32_t)v & (n >= 32 ? 0xffffffffu : ((1u << n) - 1u)), n); }
};

struct FlacEncScratch {
  int32_t* cand;                 // [4][FLAC_ENC_MAX_BS]: L, R, M, S of the frame
  uint64_t* sums;                // [31][FLAC_ENC_PARTS]
  int32_t* win;                  // [FLAC_ENC_MAX_BS]: the windowed block; the LPC predictor only
};

// sums[k][part] over the residuals of order o at partition order p (cleared here); q: the LPC coefficients, or null for the
// fixed predictor.  False when an LPC residual leaves [-2^28, 2^28).
FLAC_HD bool flac_enc_part_sums(const int32_t* s, int bs, int o, int p, int kmax, uint64_t* sums, const int* q = nullptr,
                                int shift = 0) {
  const int np = 1 << p, ps = bs >> p;
  for (int k = 0; k <= kmax; ++k)
    for (int part = 0; part < np; ++part) sums[k * FLAC_ENC_PARTS + part] = 0;
  for (int i = o; i < bs; ++i) {
    int32_t e;
    if (q) {
      const int64_t e64 = flac_enc_lpc_residual(s + i, o, q, shift);
      if (!flac_enc_residual_ok(e64)) return false;
      e = (int32_t)e64;
    } else {
      e = flac_enc_residual(s + i, o);
    }
    const uint32_t u = flac_enc_zigzag(e);
    const int part = i / ps;
    for (int k = 0; k <= kmax; ++k) sums[k * FLAC_ENC_PARTS + part] += u >> k;
  }
  return true;
}

// max_order 0: the fixed predictors alone; 1..12: the LPC candidates too (win: scratch of bs samples)
FLAC_HD void flac_enc_plan_sub(const int32_t* s, int bs, int b, int method, uint64_t* sums, FlacEncSub* out, int max_order = 0,
                               int P = 0, int32_t* win = nullptr) {
  bool same = true;
  for (int i = 1; i < bs && same; ++i) same = s[i] == s[0];
  if (same) {
    flac_enc_constant(b, out);
    return;
  }
  const int kmax = flac_enc_kmax(method), pbits = flac_enc_pbits(method);
  const int maxo = bs < 4 ? bs : 4, pmax = flac_enc_pmax(bs), top = max_order < bs ? max_order : bs;
  uint64_t rice[FLAC_ENC_CANDS * 9] = {};
  FlacEncLpcTab tab;
  if (max_order) {
    int64_t r[FLAC_ENC_LAGS];
    double ws[2 * FLAC_ENC_MAX_LPC];
    for (int i = 0; i < bs; ++i) win[i] = flac_enc_windowed(s[i], i, bs);
    flac_enc_autocorr(win, bs, r);
    flac_enc_lpc_table(r, bs, max_order, P, &tab, ws);
  }
  for (int c = 0; c <= (max_order ? 4 + top : maxo); ++c) {
    const int o = c <= 4 ? c : c - 4;
    if (c <= 4 ? c > maxo : tab.shift[o - 1] < 0) continue;
    if (!flac_enc_part_sums(s, bs, o, pmax, kmax, sums, c <= 4 ? nullptr : tab.qlp[o - 1], c <= 4 ? 0 : tab.shift[o - 1])) {
      tab.shift[o - 1] = -1;
      continue;
    }
    for (int p = pmax; p >= 0; --p) {
      const int np = 1 << p, ps = bs >> p;
      if (ps >= o) {
        uint64_t tot = 0;
        for (int q = 0; q < np; ++q) {
          int k;
          tot += pbits + flac_enc_best_k(sums + q, FLAC_ENC_PARTS, q == 0 ? ps - o : ps, kmax, &k);
        }
        rice[c * 9 + p] = tot;
      }
      if (p > 0)
        for (int q = 0; q < np / 2; ++q)                          // ascending q: q <= 2 q, nothing read after it is written
          for (int k = 0; k <= kmax; ++k)
            sums[k * FLAC_ENC_PARTS + q] = sums[k * FLAC_ENC_PARTS + 2 * q] + sums[k * FLAC_ENC_PARTS + 2 * q + 1];
    }
  }
  if (max_order) flac_enc_pick_lpc(rice, bs, b, P, max_order, &tab, out);
  else flac_enc_pick(rice, bs, b, out);
}

// the LPC subframe's head: type 31 + m, the warm-up samples, P - 1 in 4 bits, the shift in 5 (signed, never negative here),
// m coefficients of P bits
FLAC_HD long flac_enc_lpc_head_bits(int m, int b, int P) { return 8 + (long)m * b + 4 + 5 + (long)m * P; }

FLAC_HD void flac_enc_write_sub(FlacBitWriter& w, const int32_t* s, int bs, int b, int method, const FlacEncSub& sub,
                                uint64_t* sums) {
  w.put(sub.type == 0 ? 0u : sub.type == 1 ? 2u : (unsigned)((sub.type == 3 ? 31 : 8) + sub.order) << 1, 8);
  if (sub.type == 0) {
    w.put_signed(s[0], b);
    return;
  }
  if (sub.type == 1) {
    for (int i = 0; i < bs; ++i) w.put_signed(s[i], b);
    return;
  }
  const int o = sub.order, p = sub.porder, kmax = flac_enc_kmax(method), pbits = flac_enc_pbits(method);
  const int* q = sub.type == 3 ? sub.qlp : nullptr;
  for (int i = 0; i < o; ++i) w.put_signed(s[i], b);
  if (q) {
    w.put((unsigned)(sub.precision - 1), 4);
    w.put((unsigned)sub.shift, 5);
    for (int j = 0; j < o; ++j) w.put_signed(q[j], sub.precision);
  }
  w.put((unsigned)method, 2);
  w.put((unsigned)p, 4);
  flac_enc_part_sums(s, bs, o, p, kmax, sums, q, sub.shift);
  const int np = 1 << p, ps = bs >> p;
  int i = o;
  for (int part = 0; part < np; ++part) {
    const int cnt = part == 0 ? ps - o : ps;
    int k;
    flac_enc_best_k(sums + part, FLAC_ENC_PARTS, cnt, kmax, &k);
    w.put((unsigned)k, pbits);
    for (int e = i + cnt; i < e; ++i) {
      const int32_t res = q ? (int32_t)flac_enc_lpc_residual(s + i, o, q, sub.shift) : flac_enc_residual(s + i, o);
      const uint32_t u = flac_enc_zigzag(res);
      w.bit += u >> k;                                            // the unary zeros are the cleared buffer
      w.put((1u << k) | (u & ((1u << k) - 1u)), k + 1);
    }
  }
}

// One frame of pcm [C][n] (channel c at pcm + c n) at sample pos, into the zero-filled out; returns its length in bytes
// (at most flac_enc_frame_bound).  Channels 3..8 are coded independently.
FLAC_HD long flac_enc_frame(const int32_t* pcm, long n, int C, int bps, int rate, long number, long pos, int bs,
                            const FlacEncScratch& sc, uint8_t* out, int max_order = 0) {
  const int method = bps <= 16 ? 0 : 1, P = flac_enc_lpc_precision(bps);
  FlacEncSub sub[8];
  int assign = 0;
  const int32_t* ch[8];
  int width[8];
  if (C == 2) {
    for (int c = 0; c < 4; ++c)
      for (int i = 0; i < bs; ++i) sc.cand[c * FLAC_ENC_MAX_BS + i] = flac_enc_cand_sample(c, pcm[pos + i], pcm[n + pos + i]);
    FlacEncSub cs[4];
    long cb[4], bits;
    for (int c = 0; c < 4; ++c) {
      flac_enc_plan_sub(sc.cand + c * FLAC_ENC_MAX_BS, bs, bps + (c == 3), method, sc.sums, &cs[c], max_order, P, sc.win);
      cb[c] = cs[c].bits;
    }
    assign = flac_enc_pick_assign(cb, &bits);
    for (int c = 0; c < 2; ++c) {
      const int k = flac_enc_cand(assign, c);
      sub[c] = cs[k], ch[c] = sc.cand + k * FLAC_ENC_MAX_BS, width[c] = bps + (k == 3);
    }
  } else {
    for (int c = 0; c < C; ++c) {
      ch[c] = pcm + (long)c * n + pos, width[c] = bps;
      flac_enc_plan_sub(ch[c], bs, bps, method, sc.sums, &sub[c], max_order, P, sc.win);
    }
  }
  FlacBitWriter w{out, 0};
  w.bit = 8L * flac_enc_frame_header(out, bs, rate, C, assign, bps, (uint64_t)number);
  for (int c = 0; c < C; ++c) flac_enc_write_sub(w, ch[c], bs, width[c], method, sub[c], sc.sums);
  const long body = (w.bit + 7) >> 3;
  const unsigned crc = flac_crc16(out, body);
  out[body] = (uint8_t)(crc >> 8), out[body + 1] = (uint8_t)crc;
  return body + 2;
}

// The serial encoder: pcm [C][n] -> out [cap] (cleared here), cap >= flac_enc_bound(n, C, bps, block_size).  Returns the
// stream's length.  Arguments are the caller's to check (1 <= C <= 8, a supported bps, 16 <= block_size <= 4608, n >= 1,
// 1 <= rate < 2^20, every sample inside bps bits).  max_order 0: predictor "fixed"; 1..12: predictor "lpc", which needs
// sc.win.
FLAC_HD long flac_encode_serial(const int32_t* pcm, long n, int C, int bps, int rate, int block_size, const FlacEncScratch& sc,
                                uint8_t* out, long cap, int max_order = 0) {
  for (long i = 0; i < cap; ++i) out[i] = 0;
  long off = FLAC_ENC_STREAM_HEAD, min_frame = 0, max_frame = 0, number = 0;
  for (long pos = 0; pos < n; pos += block_size, ++number) {
    const int bs = n - pos < block_size ? (int)(n - pos) : block_size;
    const long len = flac_enc_frame(pcm, n, C, bps, rate, number, pos, bs, sc, out + off, max_order);
    if (number == 0 || len < min_frame) min_frame = len;
    if (len > max_frame) max_frame = len;
    off += len;
  }
  uint8_t md5[16];
  md5_pcm(pcm, n, C, bps, md5);
  flac_enc_stream_header(out, block_size, min_frame, max_frame, rate, C, bps, n, md5);
  return off;
}
