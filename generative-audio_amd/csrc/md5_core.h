// MD5 (RFC 1321) and FLAC's message over planar PCM: plain C++ that compiles as __host__ __device__
// under hipcc and as ordinary inline functions under any host compiler, so nppc_flac_md5_host, flac_md5_kernel
// (csrc/flac_md5.hip) and the sanitizer program (tools/check/md5_host_check.cc) run the same text.
//
// STREAMINFO's MD5 is taken over the unencoded samples as libFLAC feeds them: interleaved by channel, sample-major
// (sample 0 of channel 0, sample 0 of channel 1, ..., sample 1 of channel 0, ...), each a signed little-endian integer of
// (bps + 7) / 8 bytes -- the low bytes of the sign-extended int32, so a 12- or 20-bit sample fills 2 or 3 bytes.  The
// message is n * C * bytes_per_sample bytes long and is never materialised: the 16 words of a block are put together from
// the samples in registers.
//
// Safety rules every function here keeps:
//   * a sample pcm[c * n + i] is read only for 0 <= c < C and 0 <= i < n; the vector loads of the 16-bit paths cover whole
//     blocks only, which lie inside the message;
//   * lengths and byte positions are int64 / uint64_t: a message of 2^31 bytes or more hashes like any other;
//   * nothing is written but the caller's 16 digest bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MD5_HD __host__ __device__ inline
#else
#define MD5_HD inline
#endif

struct Md5 {
  uint32_t a, b, c, d;
};

MD5_HD void md5_init(Md5* s) { s->a = 0x67452301u, s->b = 0xefcdab89u, s->c = 0x98badcfeu, s->d = 0x10325476u; }

MD5_HD uint32_t md5_rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }       // 0 < s < 32: one v_alignbit_b32

// the selects as single bit-field inserts where there is one: F = d ^ (b & (c ^ d)), G = c ^ (d & (b ^ c))
#define MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, x, k, s) a = b + md5_rotl(a + f(b, c, d) + ((x) + (k)), s)

// one 64-byte block, w = its 16 little-endian words; the 64 steps written out so every constant is an immediate
MD5_HD void md5_block(Md5* st, const uint32_t w[16]) {
  uint32_t a = st->a, b = st->b, c = st->c, d = st->d;
  MD5_STEP(MD5_F, a, b, c, d, w[0], 0xd76aa478u, 7);
  MD5_STEP(MD5_F, d, a, b, c, w[1], 0xe8c7b756u, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[2], 0x242070dbu, 17);
  MD5_STEP(MD5_F, b, c, d, a, w[3], 0xc1bdceeeu, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[4], 0xf57c0fafu, 7);
  MD5_STEP(MD5_F, d, a, b, c, w[5], 0x4787c62au, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[6], 0xa8304613u, 17);
  MD5_STEP(MD5_F, b, c, d, a, w[7], 0xfd469501u, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[8], 0x698098d8u, 7);
  MD5_STEP(MD5_F, d, a, b, c, w[9], 0x8b44f7afu, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[10], 0xffff5bb1u, 17);
  MD5_STEP(MD5_F, b, c, d, a, w[11], 0x895cd7beu, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[12], 0x6b901122u, 7);
  MD5_STEP(MD5_F, d, a, b, c, w[13], 0xfd987193u, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[14], 0xa679438eu, 17);
  MD5_STEP(MD5_F, b, c, d, a, w[15], 0x49b40821u, 22);
  MD5_STEP(MD5_G, a, b, c, d, w[1], 0xf61e2562u, 5);
  MD5_STEP(MD5_G, d, a, b, c, w[6], 0xc040b340u, 9);
  MD5_STEP(MD5_G, c, d, a, b, w[11], 0x265e5a51u, 14);
  MD5_STEP(MD5_G, b, c, d, a, w[0], 0xe9b6c7aau, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[5], 0xd62f105du, 5);
  MD5_STEP(MD5_G, d, a, b, c, w[10], 0x02441453u, 9);
  MD5_STEP(MD5_G, c, d, a, b, w[15], 0xd8a1e681u, 14);
  MD5_STEP(MD5_G, b, c, d, a, w[4], 0xe7d3fbc8u, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[9], 0x21e1cde6u, 5);
  MD5_STEP(MD5_G, d, a, b, c, w[14], 0xc33707d6u, 9);
  MD5_STEP(MD5_G, c, d, a, b, w[3], 0xf4d50d87u, 14);
  MD5_STEP(MD5_G, b, c, d, a, w[8], 0x455a14edu, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[13], 0xa9e3e905u, 5);
  MD5_STEP(MD5_G, d, a, b, c, w[2], 0xfcefa3f8u, 9);
  MD5_STEP(MD5_G, c, d, a, b, w[7], 0x676f02d9u, 14);
  MD5_STEP(MD5_G, b, c, d, a, w[12], 0x8d2a4c8au, 20);
  MD5_STEP(MD5_H, a, b, c, d, w[5], 0xfffa3942u, 4);
  MD5_STEP(MD5_H, d, a, b, c, w[8], 0x8771f681u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[11], 0x6d9d6122u, 16);
  MD5_STEP(MD5_H, b, c, d, a, w[14], 0xfde5380cu, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[1], 0xa4beea44u, 4);
  MD5_STEP(MD5_H, d, a, b, c, w[4], 0x4bdecfa9u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[7], 0xf6bb4b60u, 16);
  MD5_STEP(MD5_H, b, c, d, a, w[10], 0xbebfbc70u, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[13], 0x289b7ec6u, 4);
  MD5_STEP(MD5_H, d, a, b, c, w[0], 0xeaa127fau, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[3], 0xd4ef3085u, 16);
  MD5_STEP(MD5_H, b, c, d, a, w[6], 0x04881d05u, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[9], 0xd9d4d039u, 4);
  MD5_STEP(MD5_H, d, a, b, c, w[12], 0xe6db99e5u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[15], 0x1fa27cf8u, 16);
  MD5_STEP(MD5_H, b, c, d, a, w[2], 0xc4ac5665u, 23);
  MD5_STEP(MD5_I, a, b, c, d, w[0], 0xf4292244u, 6);
  MD5_STEP(MD5_I, d, a, b, c, w[7], 0x432aff97u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[14], 0xab9423a7u, 15);
  MD5_STEP(MD5_I, b, c, d, a, w[5], 0xfc93a039u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[12], 0x655b59c3u, 6);
  MD5_STEP(MD5_I, d, a, b, c, w[3], 0x8f0ccc92u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[10], 0xffeff47du, 15);
  MD5_STEP(MD5_I, b, c, d, a, w[1], 0x85845dd1u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[8], 0x6fa87e4fu, 6);
  MD5_STEP(MD5_I, d, a, b, c, w[15], 0xfe2ce6e0u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[6], 0xa3014314u, 15);
  MD5_STEP(MD5_I, b, c, d, a, w[13], 0x4e0811a1u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[4], 0xf7537e82u, 6);
  MD5_STEP(MD5_I, d, a, b, c, w[11], 0xbd3af235u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[2], 0x2ad7d2bbu, 15);
  MD5_STEP(MD5_I, b, c, d, a, w[9], 0xeb86d391u, 21);
  st->a += a, st->b += b, st->c += c, st->d += d;
}

#undef MD5_STEP
#undef MD5_F
#undef MD5_G
#undef MD5_H
#undef MD5_I

MD5_HD void md5_store(const Md5& s, uint8_t out[16]) {
  const uint32_t v[4] = {s.a, s.b, s.c, s.d};
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
}

// The last len % 64 bytes of a message of len bytes, the padding byte 0x80, zeros, and the 64-bit little-endian bit
// length: one block, or two when fewer than 8 bytes of the first stay free.  src.seek(m) / src.next() yield the message
// bytes from position m on; next() is called for positions below len only.
template <class Src>
MD5_HD void md5_finish(Md5* st, Src& src, uint64_t len) {
  const uint64_t base = len & ~(uint64_t)63;
  const int rem = (int)(len - base);
  if (rem) src.seek(base);
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    uint32_t x = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 4 * j + t;
      const uint32_t byte = k < rem ? (uint32_t)src.next() : k == rem ? 0x80u : 0u;
      x |= byte << (8 * t);
    }
    w[j] = x;
  }
  if (rem >= 56) {
    md5_block(st, w);
#pragma unroll
    for (int j = 0; j < 14; ++j) w[j] = 0;
  }
  w[14] = (uint32_t)(len << 3);
  w[15] = (uint32_t)(len >> 29);
  md5_block(st, w);
}

// ---------------------------------------------------------------------------------------------------------- plain bytes
struct Md5ByteSrc {
  const uint8_t* p;
  uint64_t at;
  MD5_HD void seek(uint64_t m) { at = m; }
  MD5_HD uint8_t next() { return p[at++]; }
};

MD5_HD void md5_bytes(const uint8_t* msg, uint64_t len, uint8_t out[16]) {
  Md5 st;
  md5_init(&st);
  Md5ByteSrc src{msg, 0};
  for (uint64_t b = 0; b < (len >> 6); ++b) {
    uint32_t w[16];
    for (int j = 0; j < 16; ++j) {
      uint32_t x = 0;
      for (int t = 0; t < 4; ++t) x |= (uint32_t)src.next() << (8 * t);
      w[j] = x;
    }
    md5_block(&st, w);
  }
  md5_finish(&st, src, len);
  md5_store(st, out);
}

// ------------------------------------------------------------------------------------------------- FLAC's message of PCM
// the general former: a cursor (sample i, channel c, byte k of the sample) that walks the message byte by byte with no
// division after seek()
struct Md5PcmSrc {
  const int32_t* pcm;       // [C][n]
  long n;
  int C, B;                 // channels, bytes per sample
  long i;
  int c, k;
  uint32_t v;               // the sample under the cursor, when k > 0
  MD5_HD void seek(uint64_t m) {
    const uint64_t q = m / (uint64_t)B, s = q / (uint64_t)C;
    k = (int)(m - q * (uint64_t)B);
    c = (int)(q - s * (uint64_t)C);
    i = (long)s;
    if (k) v = (uint32_t)pcm[(long)c * n + i];
  }
  MD5_HD uint8_t next() {
    if (k == 0) v = (uint32_t)pcm[(long)c * n + i];
    const uint8_t byte = (uint8_t)(v >> (8 * k));
    if (++k == B) {
      k = 0;
      if (++c == C) c = 0, ++i;
    }
    return byte;
  }
};

// four consecutive samples; one 16-byte load where the address allows it (device), four 4-byte loads otherwise
MD5_HD void md5_load4(const int32_t* p, bool aligned16, int32_t* v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (aligned16) {
    const int4 q = *reinterpret_cast<const int4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    return;
  }
#endif
  (void)aligned16;
  v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
}

MD5_HD bool md5_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The 2-byte paths (bps 9..16): two samples per message word.  STEREO = 0: block b is samples [32 b, 32 b + 32) of the one
// channel; STEREO = 1: samples [16 b, 16 b + 16) of both.  The 32 samples of the next block are loaded before the 64 steps
// of the current one run: a lane's chain is dependent ALU work, and these loads are the only latency there is to hide.
template <int STEREO>
MD5_HD void md5_pcm16_blocks(Md5* st, const int32_t* pcm, long n, uint64_t blocks) {
  const int32_t* p0 = pcm;
  const int32_t* p1 = STEREO ? pcm + n : pcm + 16;
  const long step = STEREO ? 16 : 32;
  const bool al0 = md5_aligned16(p0), al1 = md5_aligned16(p1);
  int32_t raw[32];
  if (blocks) {
#pragma unroll
    for (int q = 0; q < 4; ++q) md5_load4(p0 + 4 * q, al0, raw + 4 * q), md5_load4(p1 + 4 * q, al1, raw + 16 + 4 * q);
  }
  for (uint64_t b = 0; b < blocks; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t lo = (uint32_t)(STEREO ? raw[j] : raw[2 * j]), hi = (uint32_t)(STEREO ? raw[16 + j] : raw[2 * j + 1]);
      w[j] = (lo & 0xffffu) | (hi << 16);
    }
    if (b + 1 < blocks) {                                         // in flight during the 64 steps below
      p0 += step, p1 += step;
#pragma unroll
      for (int q = 0; q < 4; ++q) md5_load4(p0 + 4 * q, al0, raw + 4 * q), md5_load4(p1 + 4 * q, al1, raw + 16 + 4 * q);
    }
    md5_block(st, w);
  }
}

// the general path: every other (C, bps), a byte at a time
MD5_HD void md5_pcm_general_blocks(Md5* st, Md5PcmSrc& src, uint64_t blocks) {
  src.seek(0);
  for (uint64_t b = 0; b < blocks; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint32_t x = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) x |= (uint32_t)src.next() << (8 * t);
      w[j] = x;
    }
    md5_block(st, w);
  }
}

// MD5 of FLAC's message of pcm [C][n] (int32, channel c at pcm + c n), 1 <= C <= 8, 4 <= bps <= 32, n >= 0
MD5_HD void md5_pcm(const int32_t* pcm, long n, int C, int bps, uint8_t out[16]) {
  const int B = (bps + 7) >> 3;
  const uint64_t len = (uint64_t)n * (uint64_t)(C * B);
  const uint64_t blocks = len >> 6;
  Md5 st;
  md5_init(&st);
  Md5PcmSrc src{pcm, n, C, B, 0, 0, 0, 0};
  if (B == 2 && C == 1) md5_pcm16_blocks<0>(&st, pcm, n, blocks);
  else if (B == 2 && C == 2) md5_pcm16_blocks<1>(&st, pcm, n, blocks);
  else md5_pcm_general_blocks(&st, src, blocks);
  md5_finish(&st, src, len);
  md5_store(st, out);
}
