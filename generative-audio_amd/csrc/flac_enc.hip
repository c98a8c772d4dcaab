// FLAC encoding for gfx950 (nppc_audio/flac.py).  Every decision is csrc/flac_enc_core.h, shared with
// the serial host encoder below and with tools/check/flac_enc_host_check.cc; specification tests/flac_enc_ref.py.
//   nppc_flac_enc_bound     host only: the verbatim bound of a stream and its frame count
//   nppc_flac_encode_host   host only: the serial encoder
//   nppc_pcm_quantize       fp32 waveforms -> int32 PCM, ragged
//   nppc_flac_enc_plan      one workgroup per (file, frame): the subframes' types, orders, partition orders, the channel
//                           assignment and the frame's exact byte length
//   nppc_flac_enc_scan      one workgroup: exclusive scan of the frame lengths over the batch (files lie back to back, each
//                           behind its 42-byte stream header) and every file's begin, end, min and max frame size
//   nppc_flac_enc_write     one workgroup per frame: the frame put together in a cleared LDS buffer, CRC-16, copy out; the
//                           first frame of a file also writes the stream header
//   nppc_flac_encode_host_lpc, nppc_flac_enc_plan_lpc, nppc_flac_enc_scan_stride, nppc_flac_enc_write_lpc: predictor "lpc"
//                           (specification tests/flac_lpc_ref.py): the same kernels instantiated with the
//                           LPC candidates, a plan record of NPPC_FLAC_ENC_PLAN_LPC ints that carries the coefficients, and the
//                           scan told the record's stride
// Sums of (u >> k) are integers: they are accumulated with integer LDS atomics, so no result depends on the order of
// arrival; so is the LPC autocorrelation.  No kernel waits for another workgroup, there is no float anywhere but in the
// quantiser and in the serial fp64 Levinson-Durbin of one thread (contraction off): two runs give identical bytes, and a
// file's bytes do not depend on its neighbours.
#include <vector>

#include "common.h"
#include "flac_enc_core.h"
#include "nppc_hip.h"

namespace {

constexpr int META = NPPC_FLAC_META;
constexpr int PLAN = NPPC_FLAC_ENC_PLAN;
constexpr int PLAN_LPC = NPPC_FLAC_ENC_PLAN_LPC;
constexpr int T = 256;
typedef unsigned long long u64;

struct Frame {
  int f, C, bs;
  long n, pos, number;
  const int* l;                  // channel 0 at the frame's first sample
  const int* r;                  // channel 1 (or l)
};

// the (file, frame) of workgroup g, checked against the buffers; false: nothing to do
__device__ bool frame_of(long g, const long* meta, int nfiles, const int* ftab, const int* pcm, long pcm_elems, int block_size,
                         Frame* fr) {
  const int f = ftab[2 * g], number = ftab[2 * g + 1];
  if (f < 0 || f >= nfiles || number < 0) return false;
  const long* m = meta + (long)f * META;
  const long C = m[3], n = m[7], po = m[9];
  if (C < 1 || C > 2 || n < 1 || n >= (1L << 36) || po < 0 || po > pcm_elems - C * n) return false;
  const long pos = (long)number * block_size;
  if (pos >= n) return false;
  fr->f = f, fr->C = (int)C, fr->n = n, fr->pos = pos, fr->number = number;
  fr->bs = n - pos < block_size ? (int)(n - pos) : block_size;
  fr->l = pcm + po + pos;
  fr->r = C == 2 ? fr->l + n : fr->l;
  return true;
}

__device__ __forceinline__ void load_cand(int* smp, const Frame& fr, int cand) {
  for (int i = threadIdx.x; i < fr.bs; i += T) smp[i] = flac_enc_cand_sample(cand, fr.l[i], fr.r[i]);
}

// sums[k][q] over the residuals of order o at partition order p: 256 >> p threads share a partition
// LPC: qlp (in LDS) holds the coefficients of an LPC order, or is null for a fixed one; a residual outside [-2^28, 2^28)
// sets *bad, which every thread may read once this returns
template <int KMAX, bool LPC>
__device__ void part_sums(const int* smp, int bs, int o, int p, u64* sums, const int* qlp = nullptr, int shift = 0,
                          int* bad = nullptr) {
  const int ps = bs >> p, tpp = T >> p;
  for (int i = threadIdx.x; i < (KMAX + 1) * FLAC_ENC_PARTS; i += T) sums[i] = 0;
  if (LPC && threadIdx.x == 0) *bad = 0;
  __syncthreads();
  const int q = threadIdx.x / tpp, sub = threadIdx.x - q * tpp;
  u64 acc[KMAX + 1];
#pragma unroll
  for (int k = 0; k <= KMAX; ++k) acc[k] = 0;
  const int end = (q + 1) * ps;                                 // bs == np ps
  int outside = 0;
  for (int i = q * ps + sub; i < end; i += tpp) {
    if (i < o) continue;
    int32_t e;
    if (LPC && qlp) {
      const int64_t e64 = flac_enc_lpc_residual(smp + i, o, qlp, shift);
      outside |= !flac_enc_residual_ok(e64);
      e = (int32_t)e64;
    } else {
      e = flac_enc_residual(smp + i, o);
    }
    const uint32_t u = flac_enc_zigzag(e);
#pragma unroll
    for (int k = 0; k <= KMAX; ++k) acc[k] += u >> k;
  }
  if (LPC && outside) atomicOr(bad, 1);
#pragma unroll
  for (int k = 0; k <= KMAX; ++k)
    if (acc[k]) atomicAdd(&sums[k * FLAC_ENC_PARTS + q], acc[k]);
  __syncthreads();
}

// what the LPC analysis of a subframe keeps in LDS
struct LpcLds {
  FlacEncLpcTab tab;
  u64 r[FLAC_ENC_LAGS];          // the autocorrelation: int64 sums, accumulated as two's complement
  double ws[2 * FLAC_ENC_MAX_LPC];
  int bad;
};
constexpr int rice_elems(bool lpc) { return lpc ? FLAC_ENC_CANDS * 9 + 1 : 46; }       // even: what follows stays 16-byte aligned

// steps 1 to 4 of the LPC rule: window and autocorrelation by all threads (the window in the sums' LDS, which part_sums
// clears before it uses it), Levinson-Durbin and the quantiser of every order by thread 0
__device__ void lpc_analyse(const int* smp, int bs, int max_order, int P, int* x, LpcLds* lp) {
  const int t = threadIdx.x;
  for (int i = t; i < bs; i += T) x[i] = flac_enc_windowed(smp[i], i, bs);
  if (t < FLAC_ENC_LAGS) lp->r[t] = 0;
  __syncthreads();
  long long acc[FLAC_ENC_LAGS];
#pragma unroll
  for (int l = 0; l < FLAC_ENC_LAGS; ++l) acc[l] = 0;
  for (int i = t; i < bs; i += T) {
    const long long xi = x[i];
#pragma unroll
    for (int l = 0; l < FLAC_ENC_LAGS; ++l)
      if (i + l < bs) acc[l] += xi * (long long)x[i + l];
  }
#pragma unroll
  for (int l = 0; l < FLAC_ENC_LAGS; ++l)
    if (acc[l]) atomicAdd(&lp->r[l], (u64)acc[l]);
  __syncthreads();
  if (t == 0) flac_enc_lpc_table(reinterpret_cast<const int64_t*>(lp->r), bs, max_order, P, &lp->tab, lp->ws);
  __syncthreads();
}

template <int KMAX, bool LPC>
__device__ void plan_sub(const int* smp, int bs, int b, int max_order, u64* sums, u64* rice, int* flag, LpcLds* lp,
                         FlacEncSub* out) {
  constexpr int METHOD = KMAX == 30, PBITS = METHOD ? 5 : 4, P = METHOD ? 15 : 12;
  if (threadIdx.x == 0) *flag = 0;
  for (int i = threadIdx.x; i < rice_elems(LPC); i += T) rice[i] = 0;
  __syncthreads();
  int diff = 0;
  for (int i = threadIdx.x; i < bs; i += T) diff |= smp[i] != smp[0];
  if (diff) atomicOr(flag, 1);
  __syncthreads();
  if (!*flag) {
    if (threadIdx.x == 0) flac_enc_constant(b, out);
    __syncthreads();
    return;
  }
  const int maxo = bs < 4 ? bs : 4, pmax = flac_enc_pmax(bs);
  int ncand = maxo + 1;
  if (LPC) {
    lpc_analyse(smp, bs, max_order, P, reinterpret_cast<int*>(sums), lp);
    ncand = 5 + (max_order < bs ? max_order : bs);
  }
  for (int c = 0; c < ncand; ++c) {                                // fixed 0..4, then LPC 1..: every test below is uniform
    const int o = c <= 4 ? c : c - 4;
    const int* qlp = nullptr;
    int shift = 0;
    if (c <= 4) {
      if (c > maxo) continue;
    } else {
      shift = lp->tab.shift[o - 1];
      if (shift < 0) continue;
      qlp = lp->tab.qlp[o - 1];
    }
    part_sums<KMAX, LPC>(smp, bs, o, pmax, sums, qlp, shift, LPC ? &lp->bad : nullptr);
    if (LPC && lp->bad) {                                          // a residual out of range: the order is no candidate
      __syncthreads();                                             // every thread has read the flag
      if (threadIdx.x == 0) lp->tab.shift[o - 1] = -1;             // read again by thread 0 alone, in the pick
      continue;
    }
    for (int p = pmax; p >= 0; --p) {
      const int np = 1 << p, ps = bs >> p, q = threadIdx.x;
      if (ps >= o && q < np) {
        int k;
        const u64 bits = PBITS + flac_enc_best_k((const uint64_t*)sums + q, FLAC_ENC_PARTS, q == 0 ? ps - o : ps, KMAX, &k);
        atomicAdd(&rice[c * 9 + p], bits);
      }
      if (p > 0) {
        u64 m[KMAX + 1];
        const bool mine = q < np / 2;
        if (mine) {
#pragma unroll
          for (int k = 0; k <= KMAX; ++k) m[k] = sums[k * FLAC_ENC_PARTS + 2 * q] + sums[k * FLAC_ENC_PARTS + 2 * q + 1];
        }
        __syncthreads();
        if (mine) {
#pragma unroll
          for (int k = 0; k <= KMAX; ++k) sums[k * FLAC_ENC_PARTS + q] = m[k];
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    if (LPC) flac_enc_pick_lpc((const uint64_t*)rice, bs, b, P, max_order, &lp->tab, out);
    else flac_enc_pick((const uint64_t*)rice, bs, b, out);
  }
  __syncthreads();
}

// LDS of both kernels: sums, then what the kernel adds, then the samples
__host__ __device__ constexpr long sums_bytes(int kmax) { return (long)(kmax + 1) * FLAC_ENC_PARTS * 8; }

// the plan record of a coded channel: (type, order, partition order), and with LPC the shift and 12 coefficients
constexpr int plan_stride(bool lpc) { return lpc ? PLAN_LPC : PLAN; }
constexpr int plan_rec(bool lpc) { return lpc ? 4 + FLAC_ENC_MAX_LPC : 3; }

template <int KMAX, bool LPC>
__global__ __launch_bounds__(T) void flac_enc_plan_kernel(const int* __restrict__ pcm, long pcm_elems, const long* __restrict__ meta,
                                                          int nfiles, const int* __restrict__ ftab, int bps, int block_size,
                                                          int max_order, int* __restrict__ plan) {
  constexpr int STRIDE = plan_stride(LPC), REC = plan_rec(LPC);
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_lds[];
  u64* sums = reinterpret_cast<u64*>(enc_lds);
  u64* rice = sums + (KMAX + 1) * FLAC_ENC_PARTS;                 // [5 or 17][9]
  int* smp = reinterpret_cast<int*>(rice + rice_elems(LPC));      // [block_size]
  __shared__ FlacEncSub sub[4];
  __shared__ int flag;
  __shared__ LpcLds lpc_lds;                                      // unused by the fixed predictor
  LpcLds* lp = LPC ? &lpc_lds : nullptr;
  const long g = blockIdx.x;
  int* out = plan + g * STRIDE;
  Frame fr;
  if (!frame_of(g, meta, nfiles, ftab, pcm, pcm_elems, block_size, &fr)) {
    if (threadIdx.x < STRIDE) out[threadIdx.x] = 0;
    return;
  }
  const int ncand = fr.C == 2 ? 4 : 1;
  for (int c = 0; c < ncand; ++c) {
    __syncthreads();
    load_cand(smp, fr, c);
    __syncthreads();
    plan_sub<KMAX, LPC>(smp, fr.bs, bps + (c == 3), max_order, sums, rice, &flag, lp, &sub[c]);
  }
  if (threadIdx.x == 0) {
    int assign = 0;
    long bits = sub[0].bits;
    if (fr.C == 2) {
      const long cb[4] = {sub[0].bits, sub[1].bits, sub[2].bits, sub[3].bits};
      assign = flac_enc_pick_assign(cb, &bits);
    }
    uint8_t h[16];
    const int hl = flac_enc_frame_header(h, fr.bs, 16000, fr.C, assign, bps, (uint64_t)fr.number);   // the length needs no rate
    out[0] = (int)(hl + ((bits + 7) >> 3) + 2);
    out[1] = assign;
    for (int c = 0; c < 2; ++c) {
      const FlacEncSub& s = sub[fr.C == 2 ? flac_enc_cand(assign, c) : 0];
      int* rec = out + 2 + REC * c;
      rec[0] = s.type, rec[1] = s.order, rec[2] = s.porder;
      if (LPC) {
        rec[3] = s.type == 3 ? s.shift : 0;
        for (int j = 0; j < FLAC_ENC_MAX_LPC; ++j) rec[4 + j] = s.type == 3 && j < s.order ? s.qlp[j] : 0;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- scan
constexpr int ST = 1024;

__global__ __launch_bounds__(ST) void flac_enc_scan_kernel(const int* __restrict__ plan, int stride, const int* __restrict__ ftab,
                                                           long nframes, int nfiles, long* __restrict__ goff,
                                                           long* __restrict__ stats) {
  __shared__ long part[ST];
  const int t = threadIdx.x;
  for (int f = t; f < nfiles; f += ST) {
    long* s = stats + 4L * f;
    s[0] = 0, s[1] = 0, s[2] = 0x7fffffffffffffffL, s[3] = 0;
  }
  const long chunk = (nframes + ST - 1) / ST, g0 = t * chunk, g1 = g0 + chunk < nframes ? g0 + chunk : nframes;
  long sum = 0;
  for (long g = g0; g < g1; ++g) sum += plan[g * stride] + (ftab[2 * g + 1] == 0 ? FLAC_ENC_STREAM_HEAD : 0);
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long run = 0;
    for (int i = 0; i < ST; ++i) {
      const long v = part[i];
      part[i] = run;
      run += v;
    }
    stats[4L * nfiles] = run;                                     // the batch's byte count
  }
  __syncthreads();
  long run = part[t];
  for (long g = g0; g < g1; ++g) {
    const int f = ftab[2 * g], len = plan[g * stride];
    const bool first = ftab[2 * g + 1] == 0;
    if (first) run += FLAC_ENC_STREAM_HEAD;
    goff[g] = run;
    if (f >= 0 && f < nfiles && len > 0) {
      u64* s = reinterpret_cast<u64*>(stats + 4L * f);
      if (first) stats[4L * f] = run - FLAC_ENC_STREAM_HEAD;     // one frame of a file is its first
      atomicMax(&s[1], (u64)(run + len));                         // the file's end
      atomicMin(&s[2], (u64)len);
      atomicMax(&s[3], (u64)len);
    }
    run += len;
  }
}

// --------------------------------------------------------------------------------------------------------------- write
__device__ __forceinline__ void lds_put(unsigned* buf, long bit, uint32_t v, int n) {    // 1 <= n <= 32, v < 2^n
  const int w = (int)(bit >> 5), r = (int)(bit & 31);
  const u64 x = (u64)v << (64 - n - r);
  const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
  if (hi) atomicOr(&buf[w], hi);
  if (lo) atomicOr(&buf[w + 1], lo);
}
__device__ __forceinline__ unsigned lds_byte(const unsigned* buf, long j) { return (buf[j >> 2] >> (24 - 8 * (int)(j & 3))) & 0xffu; }

template <int KMAX, bool LPC>
__global__ __launch_bounds__(T) void flac_enc_write_kernel(const int* __restrict__ pcm, long pcm_elems, const long* __restrict__ meta,
                                                           int nfiles, const int* __restrict__ ftab, int bps, int rate,
                                                           int block_size, const int* __restrict__ plan,
                                                           const long* __restrict__ goff, const long* __restrict__ stats,
                                                           const unsigned char* __restrict__ digest,
                                                           unsigned char* __restrict__ out, long out_cap, int buf_words) {
  constexpr int METHOD = KMAX == 30, PBITS = METHOD ? 5 : 4, P = METHOD ? 15 : 12;
  constexpr int STRIDE = plan_stride(LPC), REC = plan_rec(LPC);
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_lds[];
  u64* sums = reinterpret_cast<u64*>(enc_lds);
  unsigned* buf = reinterpret_cast<unsigned*>(sums + (KMAX + 1) * FLAC_ENC_PARTS);     // [buf_words]
  int* smp = reinterpret_cast<int*>(buf + buf_words);                                  // [block_size]
  __shared__ int kpart[FLAC_ENC_PARTS];
  __shared__ unsigned scan[T];
  __shared__ unsigned crc_acc;
  __shared__ int qlp[FLAC_ENC_MAX_LPC];                          // the coefficients of an LPC subframe
  __shared__ int bad;
  __shared__ uint8_t head[FLAC_ENC_STREAM_HEAD + 16];
  const long g = blockIdx.x;
  const int t = threadIdx.x;
  Frame fr;
  if (!frame_of(g, meta, nfiles, ftab, pcm, pcm_elems, block_size, &fr)) return;
  const int* pl = plan + g * STRIDE;
  const long nb = pl[0], off = goff[g];
  const int assign = pl[1];
  // everything the frame's bits depend on is checked: a plan that is not this frame's writes nothing
  if (nb < 8 || nb > flac_enc_frame_bound(fr.bs, fr.C, bps) || (nb + 3) / 4 + 2 > buf_words || assign < 0 || assign > 3 ||
      (assign && fr.C != 2) || off < FLAC_ENC_STREAM_HEAD || off > out_cap - nb)
    return;
  for (int i = t; i < buf_words; i += T) buf[i] = 0;
  if (t == 0) crc_acc = 0;
  __syncthreads();
  const int bs = fr.bs;
  int hl = 0;
  if (t == 0) {
    hl = flac_enc_frame_header(head + FLAC_ENC_STREAM_HEAD, bs, rate, fr.C, assign, bps, (uint64_t)fr.number);
    for (int i = 0; i < hl; ++i) lds_put(buf, 8L * i, head[FLAC_ENC_STREAM_HEAD + i], 8);
    scan[0] = (unsigned)hl;
  }
  __syncthreads();
  long pos = 8L * scan[0];
  __syncthreads();
  for (int c = 0; c < fr.C; ++c) {
    const int cand = fr.C == 2 ? flac_enc_cand(assign, c) : 0, b = bps + (cand == 3);
    const int* rec = pl + 2 + REC * c;
    const int type = rec[0], o = rec[1], p = rec[2];
    const unsigned mask = (1u << b) - 1u;
    const bool lpc = LPC && type == 3;
    int shift = 0;
    if (type < 0 || type > (LPC ? 3 : 2) || o < 0 || o > (lpc ? FLAC_ENC_MAX_LPC : 4) || o > bs || p < 0 ||
        p > flac_enc_pmax(bs) || (bs >> p) < o)
      return;                                                                                                          // uniform
    if (lpc) {                                                                          // uniform: the record is the frame's
      shift = rec[3];
      if (o < 1 || shift < 0 || shift > 15) return;
      for (int j = 0; j < o; ++j)
        if (rec[4 + j] < -(1 << (P - 1)) || rec[4 + j] >= (1 << (P - 1))) return;
    }
    const long hbits = lpc ? flac_enc_lpc_head_bits(o, b, P) + 6 : 8 + (long)o * b + 6; // of a fixed or LPC subframe
    if (pos + (type == 0 ? 8 + b : type == 1 ? 8 + (long)bs * b : hbits) > 8 * (nb - 2)) return;                      // uniform
    load_cand(smp, fr, cand);
    if (lpc && t < o) qlp[t] = rec[4 + t];
    __syncthreads();
    if (t == 0 && type) lds_put(buf, pos, type == 1 ? 2u : (unsigned)((lpc ? 31 : 8) + o) << 1, 8);
    if (type == 0) {
      if (t == 0) lds_put(buf, pos + 8, (uint32_t)smp[0] & mask, b);
      pos += 8 + b;
    } else if (type == 1) {
      for (int i = t; i < bs; i += T) lds_put(buf, pos + 8 + (long)i * b, (uint32_t)smp[i] & mask, b);
      pos += 8 + (long)bs * b;
    } else {
      if (t < o) lds_put(buf, pos + 8 + (long)t * b, (uint32_t)smp[t] & mask, b);
      const long rbase = pos + hbits;
      if (lpc) {
        const long at = pos + 8 + (long)o * b;
        if (t == 0) lds_put(buf, at, (unsigned)((P - 1) << 5) | (unsigned)shift, 9);
        if (t < o) lds_put(buf, at + 9 + (long)t * P, (uint32_t)qlp[t] & ((1u << P) - 1u), P);
      }
      if (t == 0) lds_put(buf, rbase - 6, (unsigned)(METHOD << 4) | (unsigned)p, 6);
      part_sums<KMAX, LPC>(smp, bs, o, p, sums, lpc ? qlp : nullptr, shift, LPC ? &bad : nullptr);
      if (LPC && bad) return;                                                           // uniform: a plan of other samples
      const auto zz = [&](int i) {
        return flac_enc_zigzag(lpc ? (int32_t)flac_enc_lpc_residual(smp + i, o, qlp, shift) : flac_enc_residual(smp + i, o));
      };
      const int np = 1 << p, ps = bs >> p;
      if (t < np) {
        int k;
        flac_enc_best_k((const uint64_t*)sums + t, FLAC_ENC_PARTS, t == 0 ? ps - o : ps, KMAX, &k);
        kpart[t] = k;
      }
      __syncthreads();
      // the code lengths of this thread's run of samples, then the block's exclusive scan of the runs
      const int chunk = (bs + T - 1) / T, i0 = t * chunk, i1 = i0 + chunk < bs ? i0 + chunk : bs;
      u64 mine = 0;
      for (int i = i0 > o ? i0 : o; i < i1; ++i) {
        const int k = kpart[i / ps];
        mine += (u64)(zz(i) >> k) + 1 + k;
      }
      // a subframe the plan chose is shorter than verbatim; a run that is not is a plan of another frame
      scan[t] = mine > 0x7fffffu ? 0x7fffffu : (unsigned)mine;
      __syncthreads();
      for (int d = 1; d < T; d <<= 1) {
        const unsigned v = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
      }
      const long total = scan[T - 1] + (long)np * PBITS;
      if (rbase + total > 8 * (nb - 2)) return;                                         // uniform: scan is shared
      long at = rbase + (t ? (long)scan[t - 1] : 0L);
      for (int i = i0 > o ? i0 : o; i < i1; ++i) {
        const int q = i / ps, k = kpart[q];
        const long here = at + (long)PBITS * (q + 1);
        if ((i == q * ps || i == o) && k) lds_put(buf, here - PBITS, (unsigned)k, PBITS);
        const uint32_t u = zz(i);
        lds_put(buf, here + (u >> k), (1u << k) | (u & ((1u << k) - 1u)), k + 1);
        at += (u >> k) + 1 + k;
      }
      pos = rbase + total;
      __syncthreads();
    }
    __syncthreads();
  }
  if (((pos + 7) >> 3) + 2 != nb) return;                                               // uniform
  __syncthreads();
  // CRC-16 of bytes [0, nb - 2): every thread its run of bytes from zero, moved to the end by the polynomial's linearity
  {
    const long len = nb - 2, cb = (len + T - 1) / T, j0 = t * cb, j1 = j0 + cb < len ? j0 + cb : len;
    if (j0 < j1) {
      unsigned c = 0;
      for (long j = j0; j < j1; ++j) c = flac_enc_crc16_step(c, lds_byte(buf, j));
      c = flac_enc_crc16_shift(c, len - j1);
      if (c) atomicXor(&crc_acc, c);
    }
  }
  __syncthreads();
  if (t == 0 && crc_acc) lds_put(buf, 8 * (nb - 2), crc_acc, 16);
  __syncthreads();
  // out: bytes up to the first 4-byte boundary, whole words, the bytes left
  unsigned char* dst = out + off;
  const long lead = (4 - (long)((uintptr_t)dst & 3)) & 3, headb = lead < nb ? lead : nb, words = (nb - headb) >> 2;
  for (long j = t; j < headb; j += T) dst[j] = (unsigned char)lds_byte(buf, j);
  for (long w = t; w < words; w += T) {
    const long j = headb + 4 * w;
    const int sh = 8 * (int)(j & 3);
    const unsigned a = buf[j >> 2], bnext = buf[(j >> 2) + 1];
    const unsigned be = sh ? (a << sh) | (bnext >> (32 - sh)) : a;
    *reinterpret_cast<unsigned*>(dst + j) = __builtin_bswap32(be);
  }
  for (long j = headb + 4 * words + t; j < nb; j += T) dst[j] = (unsigned char)lds_byte(buf, j);
  if (fr.number == 0) {                                                                 // the stream header
    const long* s = stats + 4L * fr.f;
    if (t == 0)
      flac_enc_stream_header(head, block_size, s[2], s[3], rate, fr.C, bps, fr.n, digest + 16L * fr.f);
    __syncthreads();
    if (t < FLAC_ENC_STREAM_HEAD) dst[t - FLAC_ENC_STREAM_HEAD] = head[t];
  }
}

__global__ __launch_bounds__(256) void pcm_quantize_kernel(const float* __restrict__ x, long ldx, const long* __restrict__ lengths,
                                                           int bits, int* __restrict__ pcm, const long* __restrict__ pcm_off,
                                                           long pcm_elems) {
  const int v = blockIdx.y;
  long len = lengths ? lengths[v] : ldx;
  len = len < 0 ? 0 : len > ldx ? ldx : len;
  const long po = pcm_off[v];
  if (po < 0 || po > pcm_elems - len) return;
  const float scale = (float)(1 << (bits - 1)), lo = -scale, hi = scale - 1.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) {
    const float y = rintf(x[v * ldx + i] * scale);                // v_rndne_f32: halves to even
    pcm[po + i] = y != y ? 0 : (int)fminf(fmaxf(y, lo), hi);
  }
}

bool enc_args_ok(int bps, int block_size) {
  return flac_enc_bps_ok(bps) && block_size >= FLAC_ENC_MIN_BS && block_size <= FLAC_ENC_MAX_BS;
}
// the serial encoder behind both host entry points; max_order 0: the fixed predictors alone
int encode_host(const int* pcm, long n, int channels, int bps, int rate, int block_size, int max_order, unsigned char* out,
                long cap, long* nbytes) {
  if (!pcm || !out || !nbytes || n < 1 || n >= (1L << 36) || channels < 1 || channels > 8 || rate < 1 || rate >= (1 << 20))
    return NPPC_EBADARG;
  if (!enc_args_ok(bps, block_size)) return NPPC_EUNSUPPORTED;
  if (cap < flac_enc_bound(n, channels, bps, block_size)) return NPPC_EBADARG;
  const int lo = -(1 << (bps - 1)), hi = (1 << (bps - 1)) - 1;
  for (long i = 0; i < n * channels; ++i)
    if (pcm[i] < lo || pcm[i] > hi) return NPPC_EBADARG;
  std::vector<int32_t> cand(4 * FLAC_ENC_MAX_BS), win(max_order ? FLAC_ENC_MAX_BS : 0);
  std::vector<uint64_t> sums(31 * FLAC_ENC_PARTS);
  const FlacEncScratch sc{cand.data(), sums.data(), win.data()};
  *nbytes = flac_encode_serial(pcm, n, channels, bps, rate, block_size, sc, out, cap, max_order);
  return NPPC_OK;
}
int write_buf_words(int block_size, int bps) { return (int)((flac_enc_frame_bound(block_size, 2, bps) + 3) / 4 + 2); }

template <class K> int raise_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return NPPC_ELAUNCH;
  return NPPC_OK;
}

template <bool LPC>
int launch_plan(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                int block_size, int max_order, int* plan, void* stream) {
  if (!pcm || !meta || !ftab || !plan || pcm_elems < 1 || nfiles < 1 || nframes < 1 || nframes >= (1L << 31)) return NPPC_EBADARG;
  if (!enc_args_ok(bps, block_size)) return NPPC_EUNSUPPORTED;
  const int kmax = bps <= 16 ? 14 : 30;
  const size_t lds = sums_bytes(kmax) + rice_elems(LPC) * 8 + (size_t)block_size * 4;
  if (kmax == 14) {
    if (raise_lds(flac_enc_plan_kernel<14, LPC>, lds)) return NPPC_ELAUNCH;
    hipLaunchKernelGGL((flac_enc_plan_kernel<14, LPC>), dim3((unsigned)nframes), dim3(T), lds, (hipStream_t)stream, pcm, pcm_elems,
                       meta, nfiles, ftab, bps, block_size, max_order, plan);
  } else {
    if (raise_lds(flac_enc_plan_kernel<30, LPC>, lds)) return NPPC_ELAUNCH;
    hipLaunchKernelGGL((flac_enc_plan_kernel<30, LPC>), dim3((unsigned)nframes), dim3(T), lds, (hipStream_t)stream, pcm, pcm_elems,
                       meta, nfiles, ftab, bps, block_size, max_order, plan);
  }
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

template <bool LPC>
int launch_write(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps, int rate,
                 int block_size, const int* plan, const long* goff, const long* stats, const unsigned char* digest,
                 unsigned char* out, long out_cap, void* stream) {
  if (!pcm || !meta || !ftab || !plan || !goff || !stats || !digest || !out || pcm_elems < 1 || nfiles < 1 || nframes < 1 ||
      nframes >= (1L << 31) || out_cap < 1 || rate < 1 || rate >= (1 << 20))
    return NPPC_EBADARG;
  if (!enc_args_ok(bps, block_size)) return NPPC_EUNSUPPORTED;
  const int kmax = bps <= 16 ? 14 : 30, words = write_buf_words(block_size, bps);
  const size_t lds = sums_bytes(kmax) + (size_t)words * 4 + (size_t)block_size * 4;
  if (kmax == 14) {
    if (raise_lds(flac_enc_write_kernel<14, LPC>, lds)) return NPPC_ELAUNCH;
    hipLaunchKernelGGL((flac_enc_write_kernel<14, LPC>), dim3((unsigned)nframes), dim3(T), lds, (hipStream_t)stream, pcm, pcm_elems,
                       meta, nfiles, ftab, bps, rate, block_size, plan, goff, stats, digest, out, out_cap, words);
  } else {
    if (raise_lds(flac_enc_write_kernel<30, LPC>, lds)) return NPPC_ELAUNCH;
    hipLaunchKernelGGL((flac_enc_write_kernel<30, LPC>), dim3((unsigned)nframes), dim3(T), lds, (hipStream_t)stream, pcm, pcm_elems,
                       meta, nfiles, ftab, bps, rate, block_size, plan, goff, stats, digest, out, out_cap, words);
  }
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // namespace

extern "C" {

int nppc_flac_enc_bound(long n, int channels, int bps, int block_size, long* bytes, long* frames) {
  if (n < 1 || n >= (1L << 36) || channels < 1 || channels > 8 || (!bytes && !frames)) return NPPC_EBADARG;
  if (!enc_args_ok(bps, block_size)) return NPPC_EUNSUPPORTED;
  if (bytes) *bytes = flac_enc_bound(n, channels, bps, block_size);
  if (frames) *frames = flac_enc_frames(n, block_size);
  return NPPC_OK;
}

int nppc_flac_encode_host(const int* pcm, long n, int channels, int bps, int rate, int block_size, unsigned char* out, long cap,
                          long* nbytes) {
  return encode_host(pcm, n, channels, bps, rate, block_size, 0, out, cap, nbytes);
}

int nppc_flac_encode_host_lpc(const int* pcm, long n, int channels, int bps, int rate, int block_size, int max_order,
                              unsigned char* out, long cap, long* nbytes) {
  if (max_order < 1 || max_order > FLAC_ENC_MAX_LPC) return NPPC_EBADARG;
  return encode_host(pcm, n, channels, bps, rate, block_size, max_order, out, cap, nbytes);
}

int nppc_pcm_quantize(const float* x, long ldx, const long* lengths, int V, int bits, int* pcm, const long* pcm_off, long pcm_elems,
                      void* stream) {
  if (!x || !pcm || !pcm_off || ldx < 1 || V < 1 || V > 65535 || pcm_elems < 0) return NPPC_EBADARG;
  if (!flac_enc_bps_ok(bits)) return NPPC_EUNSUPPORTED;
  const long bx = (ldx + 255) / 256;
  hipLaunchKernelGGL(pcm_quantize_kernel, dim3((unsigned)(bx < 4096 ? bx : 4096), V), dim3(256), 0, (hipStream_t)stream, x, ldx,
                     lengths, bits, pcm, pcm_off, pcm_elems);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_flac_enc_plan(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                       int block_size, int* plan, void* stream) {
  return launch_plan<false>(pcm, pcm_elems, meta, nfiles, ftab, nframes, bps, block_size, 0, plan, stream);
}

int nppc_flac_enc_plan_lpc(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                           int block_size, int max_order, int* plan, void* stream) {
  if (max_order < 1 || max_order > FLAC_ENC_MAX_LPC) return NPPC_EBADARG;
  return launch_plan<true>(pcm, pcm_elems, meta, nfiles, ftab, nframes, bps, block_size, max_order, plan, stream);
}

int nppc_flac_enc_scan(const int* plan, const int* ftab, long nframes, int nfiles, long* goff, long* stats, void* stream) {
  return nppc_flac_enc_scan_stride(plan, PLAN, ftab, nframes, nfiles, goff, stats, stream);
}

int nppc_flac_enc_scan_stride(const int* plan, int stride, const int* ftab, long nframes, int nfiles, long* goff, long* stats,
                              void* stream) {
  if (!plan || !ftab || !goff || !stats || nfiles < 1 || nframes < 1 || nframes >= (1L << 31) || stride < 1 || stride > 1024)
    return NPPC_EBADARG;
  hipLaunchKernelGGL(flac_enc_scan_kernel, dim3(1), dim3(ST), 0, (hipStream_t)stream, plan, stride, ftab, nframes, nfiles, goff,
                     stats);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_flac_enc_write(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                        int rate, int block_size, const int* plan, const long* goff, const long* stats,
                        const unsigned char* digest, unsigned char* out, long out_cap, void* stream) {
  return launch_write<false>(pcm, pcm_elems, meta, nfiles, ftab, nframes, bps, rate, block_size, plan, goff, stats, digest, out,
                             out_cap, stream);
}

int nppc_flac_enc_write_lpc(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                            int rate, int block_size, const int* plan, const long* goff, const long* stats,
                            const unsigned char* digest, unsigned char* out, long out_cap, void* stream) {
  return launch_write<true>(pcm, pcm_elems, meta, nfiles, ftab, nframes, bps, rate, block_size, plan, goff, stats, digest, out,
                            out_cap, stream);
}

}  // extern "C"
