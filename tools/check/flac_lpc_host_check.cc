// Sanitizer program of the FLAC encoder's predictor "lpc" (csrc/flac_enc_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/flac_lpc_host_check.cc -o flac_lpc_host_check && ./flac_lpc_host_check
//
// Every input lives in a heap block of exactly C * n samples, every stream in a block of exactly the bound (flac_enc_bound)
// and the windowed block in exactly FLAC_ENC_MAX_BS samples, so a read or a write outside any of them is an AddressSanitizer
// report; the int64 autocorrelation, the window and the residual are under UndefinedBehaviorSanitizer's overflow checks.  The
// shapes are those of tests/flac_lpc_cases.py at 16 and 24 bits (and the voiced one at 8, 12 and 20): a pulse train through
// three formant resonators with order limits 1, 8 and 12; speech, zeros, noise and a tail; a ramp; a spike; a stereo file
// (equal, independent, one or both noisy); all zeros but the first sample (r_0 = 0); +A, -A, ...; lengths 1, 2, 13, 16 and
// 17; block sizes 16, 192 and 4608; full-scale square and sine waves at 24 bits, mono and as L = -R (the side channel at
// 2^24, block 4608).  Each stream is decoded with the decoder core (csrc/flac_core.h): the samples must come back exactly,
// STREAMINFO must state the MD5 md5_pcm gives, and no frame may be longer than the fixed predictors' frame of the same
// samples.  Exit status 0 and a line of counts.
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

int32_t clip(double v, int bps) {
  const double full = (double)(1 << (bps - 1));
  double r = std::nearbyint(v);
  r = r < -full ? -full : r > full - 1 ? full - 1 : r;
  return (int32_t)r;
}

// a pulse train plus a little noise through resonators at 600, 1400 and 2600 Hz, peak at half of full scale
std::vector<int32_t> voiced(long n, int bps, int period) {
  std::vector<double> y((size_t)n);
  for (long i = 0; i < n; ++i) y[(size_t)i] = (i % period == 0 ? 1.0 : 0.0) + 0.01 * unit();
  const double f[3] = {600, 1400, 2600}, bw[3] = {80, 100, 150};
  for (int s = 0; s < 3; ++s) {
    const double r = std::exp(-M_PI * bw[s] / 16000.0), a1 = 2 * r * std::cos(2 * M_PI * f[s] / 16000.0), a2 = -r * r;
    double z1 = 0, z2 = 0;
    for (long i = 0; i < n; ++i) {
      const double z = y[(size_t)i] + a1 * z1 + a2 * z2;
      z2 = z1, z1 = z, y[(size_t)i] = z;
    }
  }
  double peak = 1e-30;
  for (double v : y) peak = std::fabs(v) > peak ? std::fabs(v) : peak;
  std::vector<int32_t> x((size_t)n);
  for (long i = 0; i < n; ++i) x[(size_t)i] = clip(y[(size_t)i] / peak * 0.5 * (double)(1 << (bps - 1)), bps);
  return x;
}

std::vector<int32_t> speech(long n, int bps, int seed) {
  std::vector<int32_t> x((size_t)n);
  for (long i = 0; i < n; ++i) {
    const double env = 0.02 + 0.98 * std::pow(std::sin(2 * M_PI * i / 2900.0 + seed), 8);
    x[(size_t)i] = clip(env * (0.25 * std::sin(2 * M_PI * 0.011 * i + seed) + 0.12 * std::sin(2 * M_PI * 0.037 * i) + 0.016 * unit()) *
                            (double)(1 << (bps - 1)), bps);
  }
  return x;
}

long n_streams = 0, n_frames = 0, n_lpc_bytes = 0, n_fixed_bytes = 0, n_raw = 0;

void die(const char* what, int C, long n, int bps, int bs, int m) {
  std::fprintf(stderr, "C %d n %ld bps %d block %d order %d: %s\n", C, n, bps, bs, m, what);
  std::exit(2);
}

// the frames' lengths of a stream the decoder accepts
std::vector<long> frame_lengths(const uint8_t* file, long len, const FlacInfo& si, int C, long n, int bps, int bs, int m) {
  std::vector<long> out;
  long off = si.first_frame, count = 0;
  while (count < n) {
    FlacFrame fr;
    long end = 0;
    if (flac_parse_header(file, len, off, si, &fr) != NPPC_FLAC_OK ||
        flac_decode_frame<false>(file, len, off, si, fr, 1, nullptr, nullptr, &end) != NPPC_FLAC_OK)
      die("a frame does not parse", C, n, bps, bs, m);
    if (end - off > flac_enc_frame_bound(fr.bs, C, bps)) die("a frame is longer than its bound", C, n, bps, bs, m);
    out.push_back(end - off), count += fr.bs, off = end;
  }
  if (off != len) die("bytes behind the last frame", C, n, bps, bs, m);
  return out;
}

void check(const std::vector<int32_t>& samples, int C, long n, int bps, int block_size, int max_order, int rate = 16000) {
  int32_t* pcm = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)(C * n));    // exactly the samples
  std::memcpy(pcm, samples.data(), sizeof(int32_t) * (size_t)(C * n));
  const long cap = flac_enc_bound(n, C, bps, block_size);
  int32_t* cand = (int32_t*)std::malloc(sizeof(int32_t) * 4 * FLAC_ENC_MAX_BS);
  uint64_t* sums = (uint64_t*)std::malloc(sizeof(uint64_t) * 31 * FLAC_ENC_PARTS);
  int32_t* win = (int32_t*)std::malloc(sizeof(int32_t) * FLAC_ENC_MAX_BS);
  const FlacEncScratch sc{cand, sums, win};
  std::vector<long> frames[2];
  for (int pass = 0; pass < 2; ++pass) {                                        // 0: predictor "lpc", 1: "fixed"
    const int m = pass ? 0 : max_order;
    uint8_t* out = (uint8_t*)std::malloc((size_t)cap);                          // exactly the bound
    std::memset(out, 0xA5, (size_t)cap);
    const long len = flac_encode_serial(pcm, n, C, bps, rate, block_size, sc, out, cap, m);
    if (len < FLAC_ENC_STREAM_HEAD + 8 || len > cap) die("the stream's length leaves the bound", C, n, bps, block_size, m);
    uint8_t* file = (uint8_t*)std::malloc((size_t)len);                         // exactly the stream
    std::memcpy(file, out, (size_t)len);
    FlacInfo si = {};
    if (flac_probe(file, len, &si) != NPPC_FLAC_OK) die("the probe rejects the stream", C, n, bps, block_size, m);
    if (si.rate != rate || si.channels != C || si.bps != bps || si.total != n || si.min_bs != block_size || si.max_bs != block_size)
      die("STREAMINFO is not the input's", C, n, bps, block_size, m);
    int32_t* back = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)(C * n));
    std::memset(back, 0x5a, sizeof(int32_t) * (size_t)(C * n));
    if (flac_decode_serial(file, len, si, back, nullptr) != NPPC_FLAC_OK) die("the decoder rejects the stream", C, n, bps, block_size, m);
    if (std::memcmp(back, pcm, sizeof(int32_t) * (size_t)(C * n)) != 0) die("other samples come back", C, n, bps, block_size, m);
    uint8_t md5[16];
    md5_pcm(pcm, n, C, bps, md5);
    if (std::memcmp(md5, file + 26, 16) != 0) die("STREAMINFO's MD5 is not the samples'", C, n, bps, block_size, m);
    frames[pass] = frame_lengths(file, len, si, C, n, bps, block_size, m);
    (pass ? n_fixed_bytes : n_lpc_bytes) += len;
    std::free(back), std::free(file), std::free(out);
  }
  if (frames[0].size() != frames[1].size()) die("the two streams have other frame counts", C, n, bps, block_size, max_order);
  for (size_t i = 0; i < frames[0].size(); ++i)
    if (frames[0][i] > frames[1][i]) die("an LPC frame is longer than the fixed frame", C, n, bps, block_size, max_order);
  ++n_streams, n_frames += (long)frames[0].size(), n_raw += C * n * ((bps + 7) / 8);
  std::free(win), std::free(sums), std::free(cand), std::free(pcm);
}

void append(std::vector<int32_t>& x, const std::vector<int32_t>& y) { x.insert(x.end(), y.begin(), y.end()); }

}  // namespace

int main() {
  for (int bps : {8, 12, 20}) check(voiced(2 * 4096 + 500, bps, 130), 1, 2 * 4096 + 500, bps, 4096, 8);
  for (int bps : {16, 24}) {
    const int full = 1 << (bps - 1);
    for (int m : {1, 8, 12}) check(voiced(2 * 4096 + 500, bps, 130), 1, 2 * 4096 + 500, bps, 4096, m);
    {                                                             // speech, zeros, noise, a short speech frame
      std::vector<int32_t> x = speech(4096, bps, 1);
      x.resize(2 * 4096, 0);
      for (int i = 0; i < 4096; ++i) x.push_back(clip(unit() * full, bps));
      append(x, speech(1000, bps, 3));
      check(x, 1, (long)x.size(), bps, 4096, 8);
    }
    {                                                             // a ramp: fixed order 2 leaves zeros and must win
      std::vector<int32_t> x;
      const int n = 4096 < 2 * full ? 4096 : 2 * full;
      for (int i = 0; i < n; ++i) x.push_back(i - n / 2);
      check(x, 1, n, bps, 4096, 8);
    }
    {                                                             // the spike: one partition, a long unary run
      std::vector<int32_t> x = speech(4096, bps, 4);
      x.resize(4096 + 1001, 0);
      x[4096 + 500] = 30000 < full - 1 ? 30000 : full - 1;
      check(x, 1, (long)x.size(), bps, 4096, 8);
    }
    {                                                             // stereo: equal, independent, left noisy, both noisy, a tail
      const long n = 4 * 4096 + 333;
      std::vector<int32_t> l = voiced(n, bps, 117), x((size_t)(2 * n));
      const int a = full >> 9 > 2 ? full >> 9 : 2;
      for (long i = 0; i < n; ++i) {
        int32_t lv = l[(size_t)i] / 2, rv = lv;
        if (i >= 4096 && i < 8192) lv = clip(unit() * full, bps), rv = clip(unit() * full, bps);
        if (i >= 8192 && i < 16384) lv += (int32_t)(rnd() % (2 * a + 1)) - a;
        if (i >= 12288 && i < 16384) rv += (int32_t)(rnd() % (2 * a + 1)) - a;
        x[(size_t)i] = lv, x[(size_t)(n + i)] = rv;
      }
      check(x, 2, n, bps, 4096, 8, 12345);
    }
    {                                                             // all zeros but the first sample: the windowed block is zero
      std::vector<int32_t> x(4096 + 50, 0);
      x[0] = 1;
      check(x, 1, (long)x.size(), bps, 4096, 8);
    }
    {                                                             // +A, -A, ...: a reflection coefficient next to -1
      std::vector<int32_t> x;
      for (int i = 0; i < 4096 + 31; ++i) x.push_back(i % 2 ? -(full - 1) : full - 1);
      check(x, 1, (long)x.size(), bps, 4096, 8);
    }
    for (long n : {1L, 2L, 13L, 16L, 17L}) {                      // orders capped by the block
      std::vector<int32_t> x = voiced(n + 40, bps, 130);
      x.erase(x.begin(), x.begin() + 40);
      check(x, 1, n, bps, 4096, 12);
    }
    check(voiced(16 * 3 + 5, bps, 130), 1, 16 * 3 + 5, bps, 16, 12);
    check(voiced(192 * 2 + 50, bps, 130), 1, 192 * 2 + 50, bps, 192, 12);
    check(voiced(4608 + 300, bps, 130), 1, 4608 + 300, bps, 4608, 12, 44100);
  }
  {                                                               // full scale at 24 bits: the side channel reaches 2^24
    const long n = 4608 + 100;
    const int full = 1 << 23;
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<int32_t> x((size_t)(2 * n));
      for (long i = 0; i < n; ++i) {
        const int32_t v = kind ? clip((full - 1) * std::sin(2 * M_PI * i / 61.7), 24) : ((i / 37) % 2 ? -(full - 1) : full - 1);
        x[(size_t)i] = v, x[(size_t)(n + i)] = -v;
      }
      check(x, 1, n, 24, 4608, 8);
      check(x, 2, n, 24, 4608, 8);
      check(x, 2, n, 24, 4608, 12);
    }
  }
  std::printf("flac_lpc_host_check: %ld streams, %ld frames, lpc %ld and fixed %ld bytes for %ld raw (%.3f, %.3f), all decoded "
              "exactly, no LPC frame longer than the fixed one\n", n_streams, n_frames, n_lpc_bytes, n_fixed_bytes, n_raw,
              (double)n_lpc_bytes / (double)n_raw, (double)n_fixed_bytes / (double)n_raw);
  return 0;
}
