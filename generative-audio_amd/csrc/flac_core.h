// FLAC decoder core (specification tests/flac_ref.py): plain C++ that compiles as __host__ __device__
// under hipcc and as ordinary inline functions under any host compiler, so the serial host decoder, the device kernels
// (csrc/flac.hip) and the sanitizer program (tools/check/flac_host_check.cc) run the same text.
//
// Safety rules every function here keeps, whatever the bytes are:
//   * FlacBits never touches a byte outside [p, p + nbytes): past the end it yields zeros and sets `overrun`;
//   * every loop is bounded by the blocksize (<= 65536), the channel count (<= 8), the predictor order (<= 32) or the bit
//     length of the file (the unary run);
//   * a frame stores only to pcm[c * total + pos + i], 0 <= i < blocksize, after pos >= 0 and pos + blocksize <= total were
//     checked, and to mono[pos + i];
//   * arithmetic on stream-controlled values is unsigned or int64 and cannot overflow: coefficients have at most 15 bits,
//     samples are int32, orders at most 32, so |sum| < 2^(14 + 31 + 5) = 2^50.
// Predictions accumulate in int64 on every path; there is no narrower path.
#pragma once
#include <stdint.h>

#include "nppc_hip.h"

#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

struct FlacInfo {       // STREAMINFO plus where the frames begin
  int rate, channels, bps, min_bs, max_bs;
  long total;           // samples per channel
  long first_frame;     // byte offset of the first frame
};

struct FlacFrame {      // a parsed frame header
  int bs, channels, assign, bps;   // assign: 0 independent, 1 left/side, 2 side/right, 3 mid/side
  long pos;                        // index of the frame's first sample
  long hdr_end;                    // byte offset just past the CRC-8
};

// ---------------------------------------------------------------------------------------------------------------- CRCs
FLAC_HD unsigned flac_crc8(const uint8_t* p, int n) {            // x^8 + x^2 + x + 1, init 0
  unsigned c = 0;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
  }
  return c;
}

// x^16 + x^15 + x^2 + 1, init 0, one byte per step without a table: for this polynomial the remainder of x * 2^16 is
// (x << 1) ^ (x << 2) ^ (0x8003 when x has odd parity) (tests/flac_ref.py computes the same CRC bit by bit)
FLAC_HD unsigned flac_crc16(const uint8_t* p, long n) {
  unsigned c = 0;
  for (long i = 0; i < n; ++i) {
    const unsigned x = (c >> 8) ^ p[i];
    unsigned par = x ^ (x >> 4);
    par ^= par >> 2;
    par ^= par >> 1;
    c = ((c << 8) ^ (x << 1) ^ (x << 2) ^ ((par & 1u) ? 0x8003u : 0u)) & 0xffffu;
  }
  return c;
}

// ----------------------------------------------------------------------------------------------------------- bit reader
struct FlacBits {       // big-endian bit reader over [p, p + nbytes)
  const uint8_t* p;
  long nbytes;
  long byte;            // next byte to load into acc
  uint64_t acc;         // unread bits, left-aligned; bits below the top `nacc` are zero
  int nacc;
  int overrun;

  FLAC_HD void seek_bits(long bit) {
    byte = bit >> 3;
    acc = 0;
    nacc = 0;
    const int r = (int)(bit & 7);
    if (r) {
      refill();
      acc <<= r;
      nacc -= r;
    }
  }
  FLAC_HD void init(const uint8_t* p_, long nbytes_, long byte_off) {
    p = p_;
    nbytes = nbytes_;
    overrun = 0;
    seek_bits(byte_off * 8);
  }
  FLAC_HD long bitpos() const { return byte * 8 - nacc; }
  FLAC_HD void refill() {
    while (nacc <= 56) {
      const uint64_t b = (byte >= 0 && byte < nbytes) ? p[byte] : 0;
      acc |= b << (56 - nacc);
      nacc += 8;
      ++byte;
    }
  }
  FLAC_HD void check() {
    if (bitpos() > nbytes * 8) overrun = 1;
  }
  FLAC_HD uint32_t read(int n) {                                  // 0 <= n <= 32
    if (n <= 0) return 0;
    refill();
    const uint32_t v = (uint32_t)(acc >> (64 - n));
    acc <<= n;
    nacc -= n;
    check();
    return v;
  }
  FLAC_HD int32_t read_signed(int n) {                            // 1 <= n <= 32, two's complement
    const uint32_t v = read(n);
    return (int32_t)(v << (32 - n)) >> (32 - n);
  }
  FLAC_HD uint32_t read_unary() {                                 // zeros before the next one; bounded by the file's end
    uint32_t q = 0;
    for (;;) {
      refill();
      if (acc == 0) {
        q += (uint32_t)nacc;
        nacc = 0;
        if (bitpos() >= nbytes * 8) {
          overrun = 1;
          return q;
        }
        continue;
      }
      const int z = __builtin_clzll(acc);                         // < nacc: the bits below nacc are zero and acc != 0
      q += (uint32_t)z;
      acc <<= z;
      acc <<= 1;
      nacc -= z + 1;
      check();
      return q;
    }
  }
  FLAC_HD void skip(long n) {                                     // n >= 0
    const long to = bitpos() + n;
    if (to > nbytes * 8) {
      overrun = 1;
      return;
    }
    seek_bits(to);
  }
};

// --------------------------------------------------------------------------------------------------------- frame header
// The header at byte `off` of the file, checked against the file's STREAMINFO (channels, sample size and, where the header
// states one, the rate must agree; the blocksize may not exceed the maximum).  The serial decoder and the parallel scan
// both call this, so they accept the same headers.
FLAC_HD int flac_parse_header(const uint8_t* p, long nbytes, long off, const FlacInfo& si, FlacFrame* fr) {
  if (off < 0 || off >= nbytes) return NPPC_FLAC_TRUNCATED;
  const int avail = nbytes - off < 16 ? (int)(nbytes - off) : 16;
  uint8_t h[16];
  for (int i = 0; i < 16; ++i) h[i] = i < avail ? p[off + i] : 0;
  if (avail < 2) return NPPC_FLAC_TRUNCATED;
  if (h[0] != 0xff || (h[1] & 0xfe) != 0xf8) return NPPC_FLAC_BAD_HEADER;     // 14-bit sync, reserved 0
  if (avail < 6) return NPPC_FLAC_TRUNCATED;
  const int variable = h[1] & 1;
  const int bsc = h[2] >> 4, src = h[2] & 15, chc = h[3] >> 4, szc = (h[3] >> 1) & 7;
  if (h[3] & 1) return NPPC_FLAC_BAD_HEADER;
  if (bsc == 0 || src == 15 || chc > 10 || szc == 3 || szc == 7) return NPPC_FLAC_BAD_HEADER;
  // the "UTF-8" coded number: 1 to 7 bytes, up to 36 bits
  int n;
  uint64_t val;
  const unsigned b0 = h[4];
  if (b0 < 0x80) n = 1, val = b0;
  else if ((b0 & 0xe0) == 0xc0) n = 2, val = b0 & 0x1f;
  else if ((b0 & 0xf0) == 0xe0) n = 3, val = b0 & 0x0f;
  else if ((b0 & 0xf8) == 0xf0) n = 4, val = b0 & 0x07;
  else if ((b0 & 0xfc) == 0xf8) n = 5, val = b0 & 0x03;
  else if ((b0 & 0xfe) == 0xfc) n = 6, val = b0 & 0x01;
  else if (b0 == 0xfe) n = 7, val = 0;
  else return NPPC_FLAC_BAD_HEADER;
  for (int i = 1; i < n; ++i) {
    if ((h[4 + i] & 0xc0) != 0x80) return NPPC_FLAC_BAD_HEADER;
    val = (val << 6) | (h[4 + i] & 0x3f);
  }
  int i = 4 + n;                                                  // <= 11; at most 2 + 2 + 1 more bytes follow
  int bs;
  if (bsc == 1) bs = 192;
  else if (bsc <= 5) bs = 576 << (bsc - 2);
  else if (bsc == 6) bs = h[i] + 1, i += 1;
  else if (bsc == 7) bs = ((h[i] << 8) | h[i + 1]) + 1, i += 2;
  else bs = 256 << (bsc - 8);
  int rate;
  switch (src) {
    case 0: rate = si.rate; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = h[i] * 1000, i += 1; break;
    case 13: rate = (h[i] << 8) | h[i + 1], i += 2; break;
    default: rate = ((h[i] << 8) | h[i + 1]) * 10, i += 2; break;
  }
  if (i + 1 > avail) return NPPC_FLAC_TRUNCATED;
  if (flac_crc8(h, i) != h[i]) return NPPC_FLAC_BAD_HEADER;
  int bps;
  switch (szc) {
    case 0: bps = si.bps; break;
    case 1: bps = 8; break;
    case 2: bps = 12; break;
    case 4: bps = 16; break;
    case 5: bps = 20; break;
    default: bps = 24; break;
  }
  const int channels = chc < 8 ? chc + 1 : 2;
  if (channels != si.channels || bps != si.bps || rate != si.rate || bs > si.max_bs) return NPPC_FLAC_BAD_HEADER;
  fr->bs = bs;
  fr->channels = channels;
  fr->assign = chc < 8 ? 0 : chc - 7;
  fr->bps = bps;
  fr->pos = variable ? (long)val : (long)val * (long)si.min_bs;   // val < 2^36, min_bs < 2^16
  fr->hdr_end = off + i + 1;
  return NPPC_FLAC_OK;
}

// ------------------------------------------------------------------------------------------------------------ subframes
struct FlacPredictor {
  int order, lpc, shift;
  int32_t qlp[32];
};

FLAC_HD int64_t flac_predict(const FlacPredictor& pr, const int32_t* s) {     // s points AT sample i; reads s[-1 .. -order]
  if (pr.lpc) {
    int64_t sum = 0;
    for (int j = 0; j < pr.order; ++j) sum += (int64_t)pr.qlp[j] * (int64_t)s[-1 - j];
    return sum >> pr.shift;
  }
  switch (pr.order) {
    case 0: return 0;
    case 1: return (int64_t)s[-1];
    case 2: return 2 * (int64_t)s[-1] - (int64_t)s[-2];
    case 3: return 3 * (int64_t)s[-1] - 3 * (int64_t)s[-2] + (int64_t)s[-3];
    default: return 4 * (int64_t)s[-1] - 6 * (int64_t)s[-2] + 4 * (int64_t)s[-3] - (int64_t)s[-4];
  }
}

// the residual of one subframe; STORE: out[i] = residual + prediction for i in [order, bs)
template <bool STORE>
FLAC_HD int flac_residual(FlacBits& br, int32_t* out, int bs, const FlacPredictor& pr) {
  const int method = (int)br.read(2);
  if (method > 1) return br.overrun ? NPPC_FLAC_TRUNCATED : NPPC_FLAC_RESERVED;
  const int pbits = method ? 5 : 4, esc = (1 << pbits) - 1;
  const int po = (int)br.read(4);
  if (br.overrun) return NPPC_FLAC_TRUNCATED;
  const int psize = bs >> po;
  if ((po > 0 && (bs & ((1 << po) - 1))) || psize < pr.order) return NPPC_FLAC_RESERVED;
  int i = pr.order;
  for (int part = 0; part < (1 << po); ++part) {
    const int cnt = part == 0 ? psize - pr.order : psize;
    const int k = (int)br.read(pbits);
    if (k == esc) {
      const int n = (int)br.read(5);
      if (!STORE) {
        br.skip((long)n * cnt);
        i += cnt;
      } else {
        for (int e = i + cnt; i < e; ++i) {
          const int32_t r = n ? br.read_signed(n) : 0;
          out[i] = (int32_t)(uint32_t)((int64_t)r + flac_predict(pr, out + i));
        }
      }
    } else {
      for (int e = i + cnt; i < e; ++i) {
        const uint32_t q = br.read_unary();
        const uint32_t u = (q << k) | br.read(k);
        if (STORE) {
          const int32_t r = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
          out[i] = (int32_t)(uint32_t)((int64_t)r + flac_predict(pr, out + i));
        }
        if (br.overrun) return NPPC_FLAC_TRUNCATED;              // ends the partition early: every later read is past the end
      }
    }
    if (br.overrun) return NPPC_FLAC_TRUNCATED;
  }
  return NPPC_FLAC_OK;
}

template <bool STORE>
FLAC_HD int flac_subframe(FlacBits& br, int32_t* out, int bs, int bps) {       // 1 <= bps <= 25
  const unsigned head = br.read(8);
  if (br.overrun) return NPPC_FLAC_TRUNCATED;
  if (head & 0x80) return NPPC_FLAC_RESERVED;
  const int type = (head >> 1) & 0x3f;
  int wasted = 0;
  if (head & 1) {
    const uint32_t w = br.read_unary();
    if (br.overrun) return NPPC_FLAC_TRUNCATED;
    if (w >= (uint32_t)(bps - 1)) return NPPC_FLAC_RESERVED;     // at least one bit per sample must remain
    wasted = (int)w + 1;
  }
  const int b = bps - wasted;
  FlacPredictor pr;
  pr.order = 0, pr.lpc = 0, pr.shift = 0;
  if (type == 0) {
    const int32_t v = br.read_signed(b);
    if (STORE)
      for (int i = 0; i < bs; ++i) out[i] = v;
  } else if (type == 1) {
    if (STORE)
      for (int i = 0; i < bs && !br.overrun; ++i) out[i] = br.read_signed(b);
    else br.skip((long)bs * b);
  } else if ((type >= 8 && type <= 12) || type >= 32) {
    pr.lpc = type >= 32;
    pr.order = pr.lpc ? type - 31 : type - 8;
    if (pr.order > bs) return NPPC_FLAC_RESERVED;
    if (STORE)
      for (int i = 0; i < pr.order; ++i) out[i] = br.read_signed(b);
    else br.skip((long)pr.order * b);
    if (pr.lpc) {
      const int prec = (int)br.read(4) + 1;
      const int32_t shift = br.read_signed(5);
      if (br.overrun) return NPPC_FLAC_TRUNCATED;
      if (prec == 16 || shift < 0) return NPPC_FLAC_RESERVED;
      pr.shift = shift;
      for (int j = 0; j < pr.order; ++j) pr.qlp[j] = br.read_signed(prec);
    }
    if (br.overrun) return NPPC_FLAC_TRUNCATED;
    const int st = flac_residual<STORE>(br, out, bs, pr);
    if (st) return st;
  } else {
    return NPPC_FLAC_RESERVED;
  }
  if (br.overrun) return NPPC_FLAC_TRUNCATED;
  if (STORE && wasted)
    for (int i = 0; i < bs; ++i) out[i] = (int32_t)((uint32_t)out[i] << wasted);
  return NPPC_FLAC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- frame
// One frame whose header `fr` came from flac_parse_header at byte `off`.  STORE = false parses only (no sample is formed or
// stored; pcm and mono are ignored): *end_off and the CRC-16 verdict are what the chain needs.  STORE = true also writes
// pcm[c * si.total + fr.pos + i] and, when mono is not null, mono[fr.pos + i] = (sum_c (float)pcm[c] / 2^(bps-1)) / C,
// summed left to right in fp32.
template <bool STORE>
FLAC_HD int flac_decode_frame(const uint8_t* p, long nbytes, long off, const FlacInfo& si, const FlacFrame& fr, int check_crc,
                              int32_t* pcm, float* mono, long* end_off) {
  const int bs = fr.bs, C = fr.channels;
  if (C < 1 || C > 8 || bs < 1 || bs > 65536) return NPPC_FLAC_BAD_HEADER;
  if (STORE && (fr.pos < 0 || fr.pos > si.total - bs)) return NPPC_FLAC_COUNT_MISMATCH;
  FlacBits br;
  br.init(p, nbytes, fr.hdr_end);
  for (int c = 0; c < C; ++c) {
    const int side = (fr.assign == 1 && c == 1) || (fr.assign == 2 && c == 0) || (fr.assign == 3 && c == 1);
    const int st = flac_subframe<STORE>(br, STORE ? pcm + (long)c * si.total + fr.pos : nullptr, bs, fr.bps + side);
    if (st) return st;
  }
  const long bit = br.bitpos();
  br.skip((8 - (bit & 7)) & 7);
  const unsigned want = br.read(16);
  if (br.overrun) return NPPC_FLAC_TRUNCATED;
  const long end = br.bitpos() >> 3;
  *end_off = end;
  if (check_crc && flac_crc16(p + off, end - 2 - off) != want) return NPPC_FLAC_CRC16;
  if (STORE) {
    int32_t* a = pcm + fr.pos;
    int32_t* b = pcm + si.total + fr.pos;
    if (fr.assign == 1) {
      for (int i = 0; i < bs; ++i) b[i] = (int32_t)(uint32_t)((int64_t)a[i] - (int64_t)b[i]);
    } else if (fr.assign == 2) {
      for (int i = 0; i < bs; ++i) a[i] = (int32_t)(uint32_t)((int64_t)a[i] + (int64_t)b[i]);
    } else if (fr.assign == 3) {
      for (int i = 0; i < bs; ++i) {
        const int64_t side = b[i];
        const int64_t m = (int64_t)((uint64_t)(int64_t)a[i] << 1) | (side & 1);
        a[i] = (int32_t)(uint32_t)((m + side) >> 1);
        b[i] = (int32_t)(uint32_t)((m - side) >> 1);
      }
    }
    if (mono) {
      const float scale = 1.0f / (float)(1 << (fr.bps - 1));
      const float fc = (float)C;
      for (int i = 0; i < bs; ++i) {
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s += (float)pcm[(long)c * si.total + fr.pos + i] * scale;
        mono[fr.pos + i] = s / fc;
      }
    }
  }
  return NPPC_FLAC_OK;
}

// ----------------------------------------------------------------------------------------------------- stream and serial
// fLaC marker and metadata blocks -> *si.  Returns a status.
FLAC_HD int flac_probe(const uint8_t* p, long nbytes, FlacInfo* si) {
  if (nbytes >= 3 && p[0] == 'I' && p[1] == 'D' && p[2] == '3') return NPPC_FLAC_UNSUPPORTED;
  if (nbytes >= 4 && p[0] == 'O' && p[1] == 'g' && p[2] == 'g' && p[3] == 'S') return NPPC_FLAC_UNSUPPORTED;
  if (nbytes < 4) {
    const char* m = "fLaC";
    for (long i = 0; i < nbytes; ++i)
      if (p[i] != (uint8_t)m[i]) return NPPC_FLAC_BAD_MARKER;
    return NPPC_FLAC_TRUNCATED;
  }
  if (p[0] != 'f' || p[1] != 'L' || p[2] != 'a' || p[3] != 'C') return NPPC_FLAC_BAD_MARKER;
  long off = 4;
  for (int first = 1;; first = 0) {
    if (off + 4 > nbytes) return NPPC_FLAC_TRUNCATED;
    const int last = p[off] >> 7, type = p[off] & 0x7f;
    const long len = ((long)p[off + 1] << 16) | ((long)p[off + 2] << 8) | (long)p[off + 3];
    off += 4;
    if (type == 127 || (first && (type != 0 || len != 34)) || (!first && type == 0)) return NPPC_FLAC_BAD_STREAMINFO;
    if (off + len > nbytes) return NPPC_FLAC_TRUNCATED;
    if (first) {
      const uint8_t* s = p + off;
      si->min_bs = (s[0] << 8) | s[1];
      si->max_bs = (s[2] << 8) | s[3];
      si->rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
      si->channels = ((s[12] >> 1) & 7) + 1;
      si->bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      si->total = ((long)(s[13] & 15) << 32) | ((long)s[14] << 24) | ((long)s[15] << 16) | ((long)s[16] << 8) | (long)s[17];
    }
    off += len;                                                   // off grows by at least 4 per block: the walk ends
    if (last) break;
  }
  si->first_frame = off;
  if (si->min_bs < 1 || si->max_bs < si->min_bs || si->rate == 0) return NPPC_FLAC_BAD_STREAMINFO;
  if (si->total == 0 || (si->bps != 8 && si->bps != 12 && si->bps != 16 && si->bps != 20 && si->bps != 24))
    return NPPC_FLAC_UNSUPPORTED;
  return NPPC_FLAC_OK;
}

// the serial decoder: frame after frame from the first until si.total samples are written
FLAC_HD int flac_decode_serial(const uint8_t* p, long nbytes, const FlacInfo& si, int32_t* pcm, float* mono) {
  long off = si.first_frame, count = 0;
  while (count < si.total) {
    FlacFrame fr;
    int st = flac_parse_header(p, nbytes, off, si, &fr);
    if (st) return st;
    if (fr.pos != count || fr.bs > si.total - count) return NPPC_FLAC_COUNT_MISMATCH;
    long end = 0;
    st = flac_decode_frame<true>(p, nbytes, off, si, fr, 1, pcm, mono, &end);
    if (st) return st;
    count += fr.bs;
    off = end;                                                    // end > off: a frame has at least 8 bytes
  }
  return NPPC_FLAC_OK;
}
