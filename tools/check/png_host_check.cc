// Sanitizer program of the PNG writer core (csrc/png_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/png_host_check.cc -o png_host_check && ./png_host_check
//
// Every index image lives in a heap block of exactly W * H bytes and every file in a block of exactly the bound the caller
// is told to provide (png_bound), so a read or a write one byte outside either is an AddressSanitizer report.  The shapes are
// those of tests/test_png_cpu.py: 1 x 1, 1 x 5, 2 x 1, 3 x 1, constant rows of 259, 260, 261, 262 and 517 pixels, constant
// images of index 2, 0 and 200, ramps, a permutation of 0..255, uniform noise 64 x 33, a replicated pattern, 300 x 70
// images (noise with equal rows and a blank block; constant 2; a stream that is one run of 21070 twos).  Each file is walked
// chunk by chunk (lengths, types, CRC-32 by a bitwise loop of its own), its IDAT inflated by a small fixed-Huffman decoder
// that knows literals, distance-1 matches and the end code, the Up filter undone and compared with the input, and the
// Adler-32 recomputed.  The token rule is also evaluated one position at a time (png_emit, as the device kernels call it) and
// must give the serial encoder's bits; the CRC-32 of IDAT is put together from pieces by png_crc_shift, as the device does, and the Adler-32 from the sums of 4096-byte tiles.
// Exit status 0 and a line of counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_core.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Image {
  long W, H;
  unsigned char* px;                                              // exactly W * H bytes
};

Image make(long W, long H) { return Image{W, H, (unsigned char*)malloc((size_t)(W * H))}; }

[[noreturn]] void fail(const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "png_host_check: %s (%ld, %ld)\n", what, a, b);
  exit(1);
}

unsigned crc_bitwise(const unsigned char* p, long n) {
  unsigned c = 0xffffffffu;
  for (long i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}
unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

struct BitReader {
  const unsigned char* p;
  long n, bit;
  unsigned get(int k) {                                           // LSB first
    unsigned v = 0;
    for (int i = 0; i < k; ++i, ++bit) {
      if ((bit >> 3) >= n) fail("inflate: the stream ends inside a code", bit, n);
      v |= ((unsigned)(p[bit >> 3] >> (bit & 7)) & 1u) << i;
    }
    return v;
  }
  unsigned huff(int k) {                                          // MSB first
    unsigned v = 0;
    for (int i = 0; i < k; ++i) v = (v << 1) | get(1);
    return v;
  }
};

// fixed-Huffman inflate of one final block with distance-1 matches only
std::vector<unsigned char> inflate(const unsigned char* z, long n, long* tokens, long* matches) {
  BitReader r{z, n, 0};
  if (r.get(1) != 1 || r.get(2) != 1) fail("inflate: not one final fixed-Huffman block");
  static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  std::vector<unsigned char> out;
  for (;;) {
    unsigned c = r.huff(7);
    int sym;
    if (c <= 0x17) sym = 256 + (int)c;                            // 0000000 .. 0010111
    else {
      c = (c << 1) | r.get(1);
      if (c >= 0x30 && c <= 0xBF) sym = (int)c - 0x30;            // 00110000 .. 10111111
      else if (c >= 0xC0 && c <= 0xC7) sym = 280 + (int)c - 0xC0;
      else {
        c = (c << 1) | r.get(1);
        if (c < 0x190 || c > 0x1FF) fail("inflate: no such code", c);
        sym = 144 + (int)c - 0x190;
      }
    }
    if (sym == 256) break;
    ++*tokens;
    if (sym < 256) {
      out.push_back((unsigned char)sym);
      continue;
    }
    if (sym > 285) fail("inflate: a reserved length code", sym);
    const int len = base[sym - 257] + (int)r.get(extra[sym - 257]);
    if (r.huff(5) != 0) fail("inflate: a distance other than 1");
    if (out.empty()) fail("inflate: a match before any byte");
    ++*matches;
    for (int i = 0; i < len; ++i) out.push_back(out.back());
  }
  if ((r.bit + 7) / 8 != n) fail("inflate: bytes behind the end code", (r.bit + 7) / 8, n);
  return out;
}

struct Counts {
  long files = 0, bytes = 0, pixels = 0, tokens = 0, matches = 0, tilings = 0;
};

void check(const Image& im, const unsigned char* palette, Counts* cn) {
  const long cap = png_bound(im.W, im.H);
  unsigned char* out = (unsigned char*)malloc((size_t)cap);       // exactly the bound
  const long len = png_encode_serial(im.px, im.W, im.H, palette, out, cap);
  if (len > cap || len < PNG_HEAD + PNG_TAIL) fail("length outside the bound", len, cap);
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (memcmp(out, sig, 8)) fail("signature");
  long at = 8;
  const char* want[4] = {"IHDR", "PLTE", "IDAT", "IEND"};
  const unsigned char* z = nullptr;
  long zn = 0;
  for (int k = 0; k < 4; ++k) {
    if (at + 12 > len) fail("a chunk runs past the file", k);
    const long n = be32(out + at);
    if (at + 12 + n > len || memcmp(out + at + 4, want[k], 4)) fail("chunk order or length", k, n);
    if (crc_bitwise(out + at + 4, 4 + n) != be32(out + at + 8 + n)) fail("chunk CRC", k);
    if (k == 0 && (n != 13 || be32(out + at + 8) != (unsigned)im.W || be32(out + at + 12) != (unsigned)im.H || out[at + 16] != 8 ||
                   out[at + 17] != 3 || out[at + 18] || out[at + 19] || out[at + 20]))
      fail("IHDR");
    if (k == 1 && (n != 768 || memcmp(out + at + 8, palette, 768))) fail("PLTE");
    if (k == 2) z = out + at + 8, zn = n;
    at += 12 + n;
  }
  if (at != len) fail("bytes behind IEND", at, len);
  if (zn < 6 || z[0] != 0x78 || z[1] != 0x01) fail("zlib header");
  long tokens = 0, matches = 0;
  const std::vector<unsigned char> s = inflate(z + 2, zn - 6, &tokens, &matches);
  const long n = png_stream_len(im.W, im.H);
  if ((long)s.size() != n) fail("stream length", (long)s.size(), n);
  unsigned A = 1, B = 0;
  for (long i = 0; i < n; ++i) A = (A + s[i]) % 65521u, B = (B + A) % 65521u;
  if (be32(z + zn - 4) != ((B << 16) | A)) fail("Adler-32");
  for (long y = 0; y < im.H; ++y) {                               // undo the Up filter
    if (s[y * (im.W + 1)] != 2) fail("filter type", y);
    for (long x = 0; x < im.W; ++x) {
      const unsigned up = y ? im.px[(y - 1) * im.W + x] : 0u;
      if (((s[y * (im.W + 1) + 1 + x] + up) & 0xffu) != im.px[y * im.W + x]) fail("pixel", x, y);
    }
  }
  // the rule position by position (png_emit of every byte on its own, as the device kernels call it, whatever the tiling)
  {
    std::vector<unsigned char> bits((size_t)(zn - 6) + 8, 0);
    long bit = 0, a = 0, b = -1;
    png_put(bits.data(), bit, 3u, 3), bit += 3;
    for (long i = 0; i < n; ++i) {
      const unsigned v = png_filt(im.px, im.W, i);
      if (i > b) {
        a = b = i;
        while (b + 1 < n && png_filt(im.px, im.W, b + 1) == v) ++b;
      }
      int nb;
      const unsigned code = png_emit(v, i - a, b - a + 1, &nb);
      if ((bit + nb + 7) / 8 > zn - 6) fail("by position: more bits than the serial encoder wrote", i);
      png_put(bits.data(), bit, code, nb), bit += nb;
    }
    if (png_deflate_bytes(bit - 3) != zn - 6 || memcmp(bits.data(), z + 2, (size_t)(zn - 6))) fail("by position: other bits");
    ++cn->tilings;
    const long m = 4 + zn;                                          // IDAT's type and data, in pieces of 1, 2, 3, ... bytes
    unsigned acc = 0;
    for (long j = 0, step = 1; j < m; j += step, ++step) {
      const long e = j + step < m ? j + step : m;
      acc ^= png_crc_shift(png_crc(z - 4 + j, e - j), m - e);
    }
    if (acc != be32(z + zn)) fail("CRC-32 from pieces");
    unsigned PA = 1, PB = 0;                                        // Adler-32 from the sums of tiles, as png_scan appends them
    for (long i0 = 0; i0 < n; i0 += PNG_TILE) {
      const long tl = n - i0 < PNG_TILE ? n - i0 : PNG_TILE;
      unsigned ta = 0, tb = 0;
      for (long j = 0; j < tl; ++j) ta += s[i0 + j], tb += (unsigned)(tl - j) * s[i0 + j];
      png_adler_append(&PA, &PB, ta % PNG_ADLER, tb % PNG_ADLER, tl);
    }
    if (((PB << 16) | PA) != be32(z + zn - 4)) fail("Adler-32 from pieces");
  }
  cn->files += 1, cn->bytes += len, cn->pixels += im.W * im.H, cn->tokens += tokens, cn->matches += matches;
  free(out);
}

}  // namespace

int main() {
  unsigned char* palette = (unsigned char*)malloc(768);
  for (int i = 0; i < 768; ++i) palette[i] = (unsigned char)rnd();
  std::vector<Image> ims;
  auto constant = [&](long W, long H, int v) {
    Image im = make(W, H);
    memset(im.px, v, (size_t)(W * H));
    ims.push_back(im);
  };
  constant(1, 1, 7);
  {
    Image im = make(1, 5);
    const unsigned char v[5] = {3, 3, 9, 9, 9};
    memcpy(im.px, v, 5);
    ims.push_back(im);
  }
  constant(2, 1, 5), constant(3, 1, 5);
  for (long w : {259L, 260L, 261L, 262L, 517L}) constant(w, 1, 17);
  constant(40, 7, 2), constant(40, 7, 0), constant(9, 5, 200);
  {
    Image a = make(256, 1), b = make(3, 256), c = make(256, 1);
    for (int i = 0; i < 256; ++i) a.px[i] = (unsigned char)i, b.px[3 * i] = b.px[3 * i + 1] = b.px[3 * i + 2] = (unsigned char)i;
    for (int i = 0; i < 256; ++i) c.px[i] = (unsigned char)i;
    for (int i = 255; i > 0; --i) {
      const int j = (int)(rnd() % (unsigned)(i + 1));
      const unsigned char t = c.px[i];
      c.px[i] = c.px[j], c.px[j] = t;
    }
    ims.push_back(a), ims.push_back(b), ims.push_back(c);
  }
  {
    Image im = make(64, 33);
    for (long i = 0; i < 64 * 33; ++i) im.px[i] = (unsigned char)rnd();
    ims.push_back(im);
  }
  {
    Image im = make(15, 8);                                       // sx = 3, sy = 2 of a 5 x 4 pattern
    unsigned char pat[20];
    for (int i = 0; i < 20; ++i) pat[i] = (unsigned char)(rnd() % 254u);
    for (int y = 0; y < 8; ++y)
      for (int x = 0; x < 15; ++x) im.px[y * 15 + x] = pat[(y / 2) * 5 + x / 3];
    ims.push_back(im);
  }
  {
    Image im = make(300, 70);
    for (long i = 0; i < 300 * 70; ++i) im.px[i] = (unsigned char)(rnd() % 254u);
    for (int y = 11; y < 30; ++y) memcpy(im.px + y * 300, im.px + 10 * 300, 300);
    for (int y = 40; y < 50; ++y) memset(im.px + y * 300 + 20, 255, 260);
    ims.push_back(im);
  }
  constant(300, 70, 2);
  {
    Image im = make(300, 70);                                     // every byte of the stream is 2: one run over every tile
    for (int y = 0; y < 70; ++y) memset(im.px + y * 300, (2 * (y + 1)) & 0xff, 300);
    ims.push_back(im);
  }
  Counts cn;
  for (const Image& im : ims) {
    check(im, palette, &cn);
    free(im.px);
  }
  free(palette);
  printf("png_host_check: %ld files, %ld pixels -> %ld bytes, %ld tokens (%ld matches), %ld streams equal by position, CRC and Adler pieces, all decoded ok\n",
         cn.files, cn.pixels, cn.bytes, cn.tokens, cn.matches, cn.tilings);
  return 0;
}
