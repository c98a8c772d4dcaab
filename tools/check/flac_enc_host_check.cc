// Sanitizer program of the FLAC encoder core (csrc/flac_enc_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/flac_enc_host_check.cc -o flac_enc_host_check && ./flac_enc_host_check
//
// Every input lives in a heap block of exactly C * n samples and every stream in a block of exactly the bound the caller is
// told to provide (flac_enc_bound), so a read or a write one byte outside either is an AddressSanitizer report.  The shapes
// are those of tests/test_flac_encode_cpu.py: every sample size (8, 12, 16, 20, 24), lengths 1, 15, 16, 4095, 4096, 4097 and
// 3 * 4096 + 1000, block sizes 16, 192, 4096 and 4608, 130 and 2050 frames of 16 samples, a frame of zeros, a frame of
// full-scale noise, 1001 zeros with one spike, a ramp, loud and quiet runs of 16 samples, bursts of two partials, stereo
// pairs (equal, independent, one or both noisy) and three to eight channels.  Each stream is decoded with the decoder core
// (csrc/flac_core.h): the samples must come back exactly, STREAMINFO must state the MD5 md5_pcm gives, the block size, and
// the smallest and largest frame, and the stream may not be longer than the bound.  Exit status 0 and a line of counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_enc_core.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
double unit() { return (double)rnd() / 4294967296.0 * 2.0 - 1.0; }

enum Kind { SPEECH, ZERO, NOISE, SPIKE, RAMP, RUNS };

void fill(std::vector<int32_t>& x, size_t at, long n, int bps, Kind kind, int seed) {
  const double full = (double)(1 << (bps - 1));
  for (long i = 0; i < n; ++i) {
    double v = 0;
    switch (kind) {
      case SPEECH: {
        const double env = 0.02 + 0.98 * std::pow(std::sin(2 * M_PI * i / 2900.0 + seed), 8);
        v = env * (0.25 * std::sin(2 * M_PI * 0.011 * i + seed) + 0.12 * std::sin(2 * M_PI * 0.037 * i) + 0.016 * unit()) * full;
        break;
      }
      case ZERO: v = 0; break;
      case NOISE: v = unit() * full; break;
      case SPIKE: v = i == n / 2 ? (30000 < full - 1 ? 30000 : full - 1) : 0; break;
      case RAMP: v = (double)(i % (long)full) - full / 2; break;
      case RUNS: v = unit() * (((i / 16) & 1) ? full / 8 : 2); break;
    }
    double r = std::nearbyint(v);
    r = r < -full ? -full : r > full - 1 ? full - 1 : r;
    x[at + (size_t)i] = (int32_t)r;
  }
}

long n_streams = 0, n_frames = 0, n_bytes = 0, n_raw = 0;

void die(const char* what, int C, long n, int bps, int bs) {
  std::fprintf(stderr, "C %d n %ld bps %d block %d: %s\n", C, n, bps, bs, what);
  std::exit(2);
}

void check(const std::vector<int32_t>& samples, int C, long n, int bps, int rate, int block_size) {
  int32_t* pcm = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)(C * n));    // exactly the samples
  std::memcpy(pcm, samples.data(), sizeof(int32_t) * (size_t)(C * n));
  const long cap = flac_enc_bound(n, C, bps, block_size);
  uint8_t* out = (uint8_t*)std::malloc((size_t)cap);                            // exactly the bound
  std::memset(out, 0xA5, (size_t)cap);
  int32_t* cand = (int32_t*)std::malloc(sizeof(int32_t) * 4 * FLAC_ENC_MAX_BS);
  uint64_t* sums = (uint64_t*)std::malloc(sizeof(uint64_t) * 31 * FLAC_ENC_PARTS);
  const FlacEncScratch sc{cand, sums};
  const long len = flac_encode_serial(pcm, n, C, bps, rate, block_size, sc, out, cap);
  if (len < FLAC_ENC_STREAM_HEAD + 8 || len > cap) die("the stream's length leaves the bound", C, n, bps, block_size);
  uint8_t* file = (uint8_t*)std::malloc((size_t)len);                           // exactly the stream
  std::memcpy(file, out, (size_t)len);
  FlacInfo si = {};
  if (flac_probe(file, len, &si) != NPPC_FLAC_OK) die("the probe rejects the stream", C, n, bps, block_size);
  if (si.rate != rate || si.channels != C || si.bps != bps || si.total != n || si.min_bs != block_size || si.max_bs != block_size)
    die("STREAMINFO is not the input's", C, n, bps, block_size);
  int32_t* back = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)(C * n));
  std::memset(back, 0x5a, sizeof(int32_t) * (size_t)(C * n));
  if (flac_decode_serial(file, len, si, back, nullptr) != NPPC_FLAC_OK) die("the decoder rejects the stream", C, n, bps, block_size);
  if (std::memcmp(back, pcm, sizeof(int32_t) * (size_t)(C * n)) != 0) die("other samples come back", C, n, bps, block_size);
  uint8_t md5[16];
  md5_pcm(pcm, n, C, bps, md5);
  if (std::memcmp(md5, file + 26, 16) != 0) die("STREAMINFO's MD5 is not the samples'", C, n, bps, block_size);
  long off = si.first_frame, count = 0, lo = 0, hi = 0;
  while (count < n) {                                                           // the frames' sizes
    FlacFrame fr;
    long end = 0;
    if (flac_parse_header(file, len, off, si, &fr) != NPPC_FLAC_OK ||
        flac_decode_frame<false>(file, len, off, si, fr, 1, nullptr, nullptr, &end) != NPPC_FLAC_OK)
      die("a frame does not parse", C, n, bps, block_size);
    if (end - off > flac_enc_frame_bound(fr.bs, C, bps)) die("a frame is longer than its bound", C, n, bps, block_size);
    lo = count == 0 || end - off < lo ? end - off : lo;
    hi = end - off > hi ? end - off : hi;
    count += fr.bs, off = end, ++n_frames;
  }
  const long smin = (file[12] << 16) | (file[13] << 8) | file[14], smax = (file[15] << 16) | (file[16] << 8) | file[17];
  if (off != len || smin != lo || smax != hi) die("STREAMINFO's frame sizes are not the frames'", C, n, bps, block_size);
  ++n_streams, n_bytes += len, n_raw += C * n * ((bps + 7) / 8);
  std::free(back), std::free(file), std::free(sums), std::free(cand), std::free(out), std::free(pcm);
}

void mono(long n, int bps, int block_size, Kind kind, int rate = 16000) {
  std::vector<int32_t> x((size_t)n);
  fill(x, 0, n, bps, kind, (int)(n % 7));
  check(x, 1, n, bps, rate, block_size);
}

}  // namespace

int main() {
  const int sizes[5] = {8, 12, 16, 20, 24};
  for (int bps : sizes) {
    {                                                             // speech, zeros, noise, a short speech frame
      std::vector<int32_t> x(3 * 4096 + 1000);
      fill(x, 0, 4096, bps, SPEECH, 1), fill(x, 4096, 4096, bps, ZERO, 0), fill(x, 8192, 4096, bps, NOISE, 0);
      fill(x, 12288, 1000, bps, SPEECH, 3);
      check(x, 1, (long)x.size(), bps, 16000, 4096);
    }
    {                                                             // the spike: one partition, a long unary run
      std::vector<int32_t> x(4096 + 1001);
      fill(x, 0, 4096, bps, SPEECH, 4), fill(x, 4096, 1001, bps, SPIKE, 0);
      check(x, 1, (long)x.size(), bps, 16000, 4096);
    }
    {                                                             // stereo: equal, independent, left noisy, both noisy, a tail
      const long n = 4 * 4096 + 333;
      std::vector<int32_t> x((size_t)(2 * n));
      fill(x, 0, n, bps, SPEECH, 5);
      for (long i = 0; i < n; ++i) x[(size_t)i] /= 2, x[(size_t)(n + i)] = x[(size_t)i];
      fill(x, 4096, 4096, bps, NOISE, 0), fill(x, (size_t)n + 4096, 4096, bps, NOISE, 0);
      const int a = (1 << (bps - 1)) >> 9 > 2 ? (1 << (bps - 1)) >> 9 : 2;
      for (long i = 8192; i < 16384; ++i) x[(size_t)i] += (int32_t)(rnd() % (2 * a + 1)) - a;
      for (long i = 12288; i < 16384; ++i) x[(size_t)(n + i)] += (int32_t)(rnd() % (2 * a + 1)) - a;
      check(x, 2, n, bps, 12345, 4096);
    }
    for (long n : {1L, 15L, 16L, 4095L, 4096L, 4097L}) mono(n, bps, 4096, SPEECH);
    mono(16 * 3 + 5, bps, 16, SPEECH), mono(192 * 2 + 50, bps, 192, SPEECH), mono(4608 + 300, bps, 4608, SPEECH, 44100);
    mono(4096, bps, 4096, RAMP), mono(2 * 4096, bps, 4096, RUNS);
    for (int C = 3; C <= 8; C += bps == 16 ? 1 : 5) {
      std::vector<int32_t> x((size_t)(C * 3000));
      for (int c = 0; c < C; ++c) fill(x, (size_t)c * 3000, 3000, bps, c == 4 ? ZERO : SPEECH, c);
      check(x, C, 3000, bps, 48000, 1024);
    }
  }
  mono(16 * 130, 16, 16, SPEECH), mono(16 * 2050, 16, 16, SPEECH);    // the frame number's 1 -> 2 and 2 -> 3 byte codes
  {
    std::vector<int32_t> x(2 * 4608 * 2);                             // the bound itself: full-scale stereo noise, 24 bits
    fill(x, 0, (long)x.size(), 24, NOISE, 0);
    check(x, 2, 2 * 4608, 24, 96000, 4608);
  }
  std::printf("flac_enc_host_check: %ld streams, %ld frames, %ld bytes for %ld raw (%.3f), all decoded exactly\n", n_streams,
              n_frames, n_bytes, n_raw, (double)n_bytes / (double)n_raw);
  return 0;
}
