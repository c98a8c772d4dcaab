// PNG writer core (specification tests/png_ref.py): plain C++ that compiles as __host__ __device__
// under hipcc and as ordinary inline functions under any host compiler, so the serial host encoder, the device kernels
// (csrc/spec_png.hip) and the sanitizer program (tools/check/png_host_check.cc) take every decision with the same text.
//
// The file: signature, IHDR (8 bits, colour type 3, no interlace), PLTE (256 entries), one IDAT, IEND.  Every scanline has
// filter type 2 (Up; the row above row 0 is zeros): the filtered stream s has n = H (W + 1) bytes.  zlib: 78 01, ONE
// deflate block (BFINAL = 1, BTYPE = 01, the fixed Huffman codes of RFC 1951 section 3.2.6), end code, pad, Adler-32 of s.
// The token rule, a function of s alone:
//   s is split into maximal runs of equal bytes (rows do not matter: the filter byte is a byte of s like any other);
//   a run of length L emits its first byte as a literal; rem = L - 1; while rem >= 3 a match (distance 1, length
//   m = min(258, rem)), rem -= m; the last rem < 3 bytes are literals.  Nothing else is ever matched.
// png_emit states the rule per POSITION of a run, so any split of s into tiles gives the same tokens.
//
// Safety rules: the bit writer ORs into a zero-filled buffer and touches only bytes that receive a one bit, all of which lie
// inside png_bound(W, H); every loop is bounded by the stream or by 32 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

#define PNG_MAX_DIM 16384            // W and H
#define PNG_MAX_PIXELS (1L << 26)    // W * H
#define PNG_TILE 4096                // bytes of s per workgroup of the device encoder
#define PNG_PLTE 780                 // the PLTE chunk: length, type, 256 x 3, CRC
#define PNG_HEAD (8 + 25 + PNG_PLTE + 8 + 2)   // everything in front of the deflate block: ... IDAT's length and type, 78 01
#define PNG_TAIL (4 + 4 + 12)        // Adler-32, IDAT's CRC, IEND
#define PNG_ADLER 65521u

PNG_HD bool png_dims_ok(long W, long H) {
  return W >= 1 && H >= 1 && W <= PNG_MAX_DIM && H <= PNG_MAX_DIM && W * H <= PNG_MAX_PIXELS;
}
PNG_HD long png_stream_len(long W, long H) { return H * (W + 1); }
// bytes of the deflate block whose tokens take `bits` bits: 3 header bits, the tokens, the 7-bit end code, padded
PNG_HD long png_deflate_bytes(long bits) { return (3 + bits + 7 + 7) / 8; }
PNG_HD long png_file_bytes(long bits) { return PNG_HEAD + png_deflate_bytes(bits) + PNG_TAIL; }
PNG_HD long png_bound(long W, long H) { return png_file_bytes(9 * png_stream_len(W, H)); }

// byte i of the filtered stream of the index image idx [H][W]
PNG_HD unsigned png_filt(const unsigned char* idx, long W, long i) {
  const long y = i / (W + 1), x = i - y * (W + 1);
  if (x == 0) return 2u;
  const unsigned cur = idx[y * W + x - 1], up = y ? idx[(y - 1) * W + x - 1] : 0u;
  return (cur - up) & 0xffu;
}

PNG_HD unsigned png_rev(unsigned v, int n) {                      // the n low bits of v, reversed
  unsigned r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// literal / length symbol 0..287 -> its fixed Huffman code as it enters the LSB-first stream, and its length
PNG_HD unsigned png_sym_code(int sym, int* n) {
  if (sym < 144) return *n = 8, png_rev(0x30u + sym, 8);
  if (sym < 256) return *n = 9, png_rev(0x190u + (sym - 144), 9);
  if (sym < 280) return *n = 7, png_rev((unsigned)(sym - 256), 7);
  return *n = 8, png_rev(0xC0u + (sym - 280), 8);
}

// RFC 1951 section 3.2.5: length codes 257..285
struct PngLenTab {
  unsigned short base[29];
  unsigned char extra[29];
};
PNG_HD PngLenTab png_len_tab() {
  return PngLenTab{{3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258},
                   {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0}};
}
PNG_HD int png_len_index(int m) {                                 // 3 <= m <= 258 -> 0..28
  if (m == 258) return 28;
  int c = 0;
  const PngLenTab t = png_len_tab();
  while (c < 27 && m >= t.base[c + 1]) ++c;
  return c;
}

PNG_HD unsigned png_literal(unsigned v, int* n) { return png_sym_code((int)v, n); }
// a match of distance 1 and length m: length code, its extra bits, the 5-bit distance code 0
PNG_HD unsigned png_match(int m, int* n) {
  const PngLenTab t = png_len_tab();
  const int c = png_len_index(m);
  int ns;
  unsigned code = png_sym_code(257 + c, &ns);
  code |= (unsigned)(m - t.base[c]) << ns;
  *n = ns + t.extra[c] + 5;
  return code;
}

// what position p (0-based) of a run of L equal bytes v puts into the stream: the code and its length, 0 for nothing
PNG_HD unsigned png_emit(unsigned v, long p, long L, int* n) {
  if (p == 0) return png_literal(v, n);
  const long q = p - 1, j = q / 258, r = q - j * 258, rem = L - 1 - 258 * j;
  if (rem < 3) return png_literal(v, n);
  if (r) return *n = 0, 0u;
  return png_match(rem < 258 ? (int)rem : 258, n);
}

// ---- CRC-32 (PNG annex D; the polynomial reflected) ------------------------------------------------------------------------
#define PNG_CRC_POLY 0xEDB88320u
PNG_HD unsigned png_crc_entry(unsigned b) {
  unsigned c = b;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PNG_CRC_POLY : c >> 1;
  return c;
}
// the register (not the finished CRC) after one more byte
PNG_HD unsigned png_crc_step(unsigned c, unsigned byte) { return png_crc_entry((c ^ byte) & 0xffu) ^ (c >> 8); }
PNG_HD unsigned png_crc(const unsigned char* p, long n) {
  unsigned c = 0xffffffffu;
  for (long i = 0; i < n; ++i) c = png_crc_step(c, p[i]);
  return c ^ 0xffffffffu;
}
// a(x) b(x) mod P in the reflected representation (bit 31 is x^0)
PNG_HD unsigned png_gf_mul(unsigned a, unsigned b) {
  unsigned p = 0;
  for (unsigned m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
  }
  return p;
}
// the finished CRC of A moved in front of nbytes more bytes: crc(A B) = png_crc_shift(crc(A), |B|) ^ crc(B)
PNG_HD unsigned png_crc_shift(unsigned crc, long nbytes) {
  unsigned p = 0x80000000u, base = 0x40000000u;                   // x^0, x^1
  for (unsigned long e = 8ul * (unsigned long)nbytes; e; e >>= 1) {
    if (e & 1ul) p = png_gf_mul(base, p);
    base = png_gf_mul(base, base);
  }
  return png_gf_mul(p, crc);
}

// ---- Adler-32: (a, b) of a piece of len bytes is a = sum s_j, b = sum (len - j) s_j, both mod 65521 ---------------------------
PNG_HD void png_adler_append(unsigned* A, unsigned* B, unsigned a, unsigned b, long len) {
  *B = (unsigned)(((unsigned long)*B + (unsigned long)(len % PNG_ADLER) * *A + b) % PNG_ADLER);
  *A = (*A + a) % PNG_ADLER;
}

// ---- bytes ----------------------------------------------------------------------------------------------------------------------
PNG_HD void png_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24), p[1] = (unsigned char)(v >> 16), p[2] = (unsigned char)(v >> 8), p[3] = (unsigned char)v;
}
// the PLTE chunk of a 256 x 3 palette
PNG_HD void png_plte(unsigned char* c, const unsigned char* palette) {
  png_be32(c, 768);
  c[4] = 'P', c[5] = 'L', c[6] = 'T', c[7] = 'E';
  for (int i = 0; i < 768; ++i) c[8 + i] = palette[i];
  png_be32(c + 776, png_crc(c + 4, 772));
}
// bytes [0, 33): the signature and IHDR
PNG_HD void png_ihdr(unsigned char* h, long W, long H) {
  const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  for (int i = 0; i < 8; ++i) h[i] = sig[i];
  png_be32(h + 8, 13);
  h[12] = 'I', h[13] = 'H', h[14] = 'D', h[15] = 'R';
  png_be32(h + 16, (unsigned)W), png_be32(h + 20, (unsigned)H);
  h[24] = 8, h[25] = 3, h[26] = 0, h[27] = 0, h[28] = 0;
  png_be32(h + 29, png_crc(h + 12, 17));
}
// bytes [33 + PNG_PLTE, PNG_HEAD): IDAT's length and type, the zlib header
PNG_HD void png_idat_head(unsigned char* h, long deflate_bytes) {
  png_be32(h, (unsigned)(2 + deflate_bytes + 4));
  h[4] = 'I', h[5] = 'D', h[6] = 'A', h[7] = 'T', h[8] = 0x78, h[9] = 0x01;
}
// the PNG_TAIL bytes behind the deflate block
PNG_HD void png_tail(unsigned char* p, unsigned adler, unsigned idat_crc) {
  png_be32(p, adler), png_be32(p + 4, idat_crc), png_be32(p + 8, 0);
  p[12] = 'I', p[13] = 'E', p[14] = 'N', p[15] = 'D';
  png_be32(p + 16, 0xAE426082u);
}

PNG_HD void png_put(unsigned char* buf, long bit, unsigned v, int n) {       // LSB first; buf is zero where it is written
  for (int i = 0; i < n; ++i, ++bit)
    if ((v >> i) & 1u) buf[bit >> 3] |= (unsigned char)(1u << (bit & 7));
}

// The serial encoder: idx [H][W], palette [256][3] -> out (zeroed here; cap >= png_bound(W, H)); returns the file's length.
PNG_HD long png_encode_serial(const unsigned char* idx, long W, long H, const unsigned char* palette, unsigned char* out, long cap) {
  const long n = png_stream_len(W, H);
  for (long i = 0; i < cap; ++i) out[i] = 0;
  unsigned char* d = out + PNG_HEAD;
  long bit = 0, start = 0;
  unsigned A = 1, B = 0;
  png_put(d, bit, 3u, 3), bit += 3;                               // BFINAL = 1, BTYPE = 01
  while (start < n) {
    const unsigned v = png_filt(idx, W, start);
    long end = start + 1;
    while (end < n && png_filt(idx, W, end) == v) ++end;
    const long L = end - start;
    for (long p = 0; p < L; ++p) {
      int nb;
      const unsigned code = png_emit(v, p, L, &nb);
      png_put(d, bit, code, nb), bit += nb;
      png_adler_append(&A, &B, v, v, 1);
    }
    start = end;
  }
  const long db = png_deflate_bytes(bit - 3);                     // the end code is seven zero bits
  png_ihdr(out, W, H);
  png_plte(out + 33, palette);
  png_idat_head(out + 33 + PNG_PLTE, db);
  const unsigned adler = (B << 16) | A;
  png_be32(d + db, adler);
  png_tail(d + db, adler, png_crc(out + PNG_HEAD - 6, 6 + db + 4));
  return PNG_HEAD + db + PNG_TAIL;
}
