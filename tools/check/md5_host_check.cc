// Sanitizer program of the MD5 core (csrc/md5_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/md5_host_check.cc -o md5_host_check && ./md5_host_check
//
// Every message and every block of samples lives in a heap block of exactly its size, so a read one byte outside either is
// an AddressSanitizer report.  It checks
//   (a) the known answers of RFC 1321, appendix A.5 (all seven);
//   (b) plain messages of every length 0..130 of seeded random bytes: md5_bytes against an MD5 written a second time here,
//       the plain way (a padded copy of the message, a table of constants, a loop over the 64 steps);
//   (c) FLAC's message of planar PCM: md5_pcm for every (channels, bits) of the tests -- (1, 8), (1, 16), (2, 16), (2, 24),
//       (3, 12), (8, 20), (1, 24) -- and (2, 12), (1, 32), (5, 4), at every sample count 0..130 and a few long ones, against
//       the second MD5 over a byte buffer built here sample by sample.  Samples are random over the whole range of their
//       width, with both extremes and -1 among them.
// Exit status 0 and a line of counts when all of that held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "md5_core.h"

namespace {

// ---- the second MD5: RFC 1321 as its text gives it --------------------------------------------------------------------
std::string plain_md5(const std::vector<uint8_t>& msg) {
  static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,
                            14, 20, 5, 9,  14, 20, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21,
                            6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
  uint32_t K[64];
  for (int i = 0; i < 64; ++i) K[i] = (uint32_t)(uint64_t)std::floor(std::fabs(std::sin((double)(i + 1))) * 4294967296.0);
  std::vector<uint8_t> m(msg);
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  const uint64_t bits = (uint64_t)msg.size() * 8;
  for (int i = 0; i < 8; ++i) m.push_back((uint8_t)(bits >> (8 * i)));
  uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
  for (size_t off = 0; off < m.size(); off += 64) {
    uint32_t w[16];
    for (int j = 0; j < 16; ++j)
      w[j] = (uint32_t)m[off + 4 * j] | ((uint32_t)m[off + 4 * j + 1] << 8) | ((uint32_t)m[off + 4 * j + 2] << 16) |
             ((uint32_t)m[off + 4 * j + 3] << 24);
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    for (int i = 0; i < 64; ++i) {
      uint32_t f;
      int g;
      if (i < 16) f = (b & c) | (~b & d), g = i;
      else if (i < 32) f = (d & b) | (~d & c), g = (5 * i + 1) % 16;
      else if (i < 48) f = b ^ c ^ d, g = (3 * i + 5) % 16;
      else f = c ^ (b | ~d), g = (7 * i) % 16;
      const uint32_t x = a + f + K[i] + w[g];
      a = d, d = c, c = b;
      b = b + ((x << S[i]) | (x >> (32 - S[i])));
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d;
  }
  std::string out(16, '\0');
  for (int i = 0; i < 16; ++i) out[i] = (char)(uint8_t)(h[i >> 2] >> (8 * (i & 3)));
  return out;
}

std::string hex(const std::string& d) {
  static const char* x = "0123456789abcdef";
  std::string s;
  for (unsigned char c : d) s += x[c >> 4], s += x[c & 15];
  return s;
}

// md5_bytes over a heap block of exactly the message
std::string core_md5(const std::vector<uint8_t>& msg) {
  uint8_t* p = (uint8_t*)std::malloc(msg.size() ? msg.size() : 1);
  if (!msg.empty()) std::memcpy(p, msg.data(), msg.size());
  uint8_t d[16];
  md5_bytes(p, (uint64_t)msg.size(), d);
  std::free(p);
  return std::string((const char*)d, 16);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

long n_known = 0, n_plain = 0, n_pcm = 0;

void fail(const char* what, long a, long b, long c) {
  std::fprintf(stderr, "md5_host_check: %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(2);
}

void check_pcm(int C, int bps, long n) {
  const int B = (bps + 7) / 8;
  const int64_t lo = -((int64_t)1 << (bps - 1)), hi = ((int64_t)1 << (bps - 1)) - 1;
  const size_t elems = (size_t)C * (size_t)n;
  int32_t* pcm = (int32_t*)std::malloc(elems ? elems * sizeof(int32_t) : 1);   // exactly C * n samples
  for (size_t i = 0; i < elems; ++i) {
    const uint32_t r = rnd(), pick = r & 15;                      // 3 in 16 are an extreme or -1
    const uint64_t wide = ((uint64_t)rnd() << 1) | (r >> 31);     // 33 random bits: enough for the 2^32 values of 32 bits
    const int64_t v = pick == 0 ? lo : pick == 1 ? hi : pick == 2 ? -1 : lo + (int64_t)(wide % (uint64_t)(hi - lo + 1));
    pcm[i] = (int32_t)v;
  }
  std::vector<uint8_t> msg;                                       // the message, sample by sample
  for (long i = 0; i < n; ++i)
    for (int c = 0; c < C; ++c) {
      const int64_t v = pcm[(size_t)c * (size_t)n + (size_t)i];
      for (int k = 0; k < B; ++k) msg.push_back((uint8_t)(((uint64_t)v >> (8 * k)) & 0xff));
    }
  if ((long)msg.size() != n * C * B) fail("message length", C, bps, n);
  uint8_t d[16];
  md5_pcm(pcm, n, C, bps, d);
  std::free(pcm);
  if (std::string((const char*)d, 16) != plain_md5(msg)) fail("md5_pcm differs from the MD5 of the message", C, bps, n);
  ++n_pcm;
}

}  // namespace

int main() {
  // (a) RFC 1321, A.5
  const char* known[][2] = {{"", "d41d8cd98f00b204e9800998ecf8427e"},
                            {"a", "0cc175b9c0f1b6a831c399e269772661"},
                            {"abc", "900150983cd24fb0d6963f7d28e17f72"},
                            {"message digest", "f96b697d7cb7938d525a2f31aaf161d0"},
                            {"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"},
                            {"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"},
                            {"12345678901234567890123456789012345678901234567890123456789012345678901234567890",
                             "57edf4a22be3c955ac49da2e2107b67a"}};
  for (auto& k : known) {
    const std::vector<uint8_t> msg(k[0], k[0] + std::strlen(k[0]));
    if (hex(core_md5(msg)) != k[1] || hex(plain_md5(msg)) != k[1]) {
      std::fprintf(stderr, "md5_host_check: \"%s\" gives %s and %s, not %s\n", k[0], hex(core_md5(msg)).c_str(),
                   hex(plain_md5(msg)).c_str(), k[1]);
      return 2;
    }
    ++n_known;
  }
  // (b) every message length 0..130
  for (long len = 0; len <= 130; ++len)
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<uint8_t> msg((size_t)len);
      for (auto& b : msg) b = (uint8_t)rnd();
      if (core_md5(msg) != plain_md5(msg)) fail("md5_bytes differs from the plain MD5 at length", len, rep, 0);
      ++n_plain;
    }
  // (c) the PCM message former
  const int formats[][2] = {{1, 8}, {1, 16}, {2, 16}, {2, 24}, {3, 12}, {8, 20}, {1, 24}, {2, 12}, {1, 32}, {5, 4}};
  for (auto& f : formats) {
    for (long n = 0; n <= 130; ++n) check_pcm(f[0], f[1], n);
    for (long n : {255L, 256L, 257L, 1000L, 4099L}) check_pcm(f[0], f[1], n);
  }
  std::printf("md5_host_check: %ld known answers, %ld plain messages of 0..130 bytes, %ld PCM messages: all equal\n", n_known,
              n_plain, n_pcm);
  return 0;
}
