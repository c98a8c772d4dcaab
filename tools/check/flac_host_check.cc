// Sanitizer program of the FLAC decoder core (csrc/flac_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/flac_host_check.cc -o flac_host_check && ./flac_host_check tests/golden/flac_two_frame.flac
//
// Every input lives in a heap block of exactly its size and every output in a block of exactly C * n samples, so a read
// or a write one byte outside either is an AddressSanitizer report.  On the stream given (the two-frame stereo stream of
// the mutation tests) it runs: every truncation length, every single-bit flip of the first 600 bytes, and 4000 seeded
// random byte strings behind the stream's own metadata and first frame header.  Each input goes through
//   (a) the serial decoder, and
//   (b) what the device kernels do, on the host: every byte position tested for a header, every candidate parsed to its
//       end with stores off, the chain walked over the candidates, the accepted frames decoded with stores on;
// Further files on the command line are put through (a) and (b) once each, as they are (the corrupt files of the GPU tests).
// (a) and (b) must agree in status and, when the status is 0, in every sample; a status of 0 must mean the original
// samples (or, for the random strings, just agreement).  Exit status 0 and a line of counts when all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "flac_core.h"

namespace {

struct Result {
  int status;
  FlacInfo si;
  std::vector<int32_t> pcm;
  std::vector<float> mono;
};

const long MAX_OUT = 1L << 22;   // a mutated STREAMINFO may claim 2^36 samples: such a file is only parsed, not stored

Result serial(const uint8_t* p, long n) {
  Result r{};
  r.status = flac_probe(p, n, &r.si);
  if (r.status) return r;
  if (r.si.channels * r.si.total > MAX_OUT) {
    r.status = -1;
    return r;
  }
  // exact-size heap blocks: vector storage of exactly C * total and total elements
  r.pcm.assign((size_t)(r.si.channels * r.si.total), 0x5a5a5a5a);
  r.pcm.shrink_to_fit();
  r.mono.assign((size_t)r.si.total, -7.0f);
  r.mono.shrink_to_fit();
  r.status = flac_decode_serial(p, n, r.si, r.pcm.data(), r.mono.data());
  return r;
}

Result device_like(const uint8_t* p, long n) {
  Result r{};
  r.status = flac_probe(p, n, &r.si);
  if (r.status) return r;
  const FlacInfo& si = r.si;
  struct Cand {
    int status;
    long end;
  };
  std::map<long, Cand> cands;                                     // scan + parse
  for (long off = si.first_frame; off < n; ++off) {
    FlacFrame fr;
    if (flac_parse_header(p, n, off, si, &fr) != NPPC_FLAC_OK) continue;
    Cand c{0, 0};
    c.status = flac_decode_frame<false>(p, n, off, si, fr, 1, nullptr, nullptr, &c.end);
    cands[off] = c;
  }
  std::vector<long> accepted;                                     // chain
  long off = si.first_frame, count = 0;
  int st = NPPC_FLAC_OK;
  while (count < si.total) {
    FlacFrame fr;
    st = flac_parse_header(p, n, off, si, &fr);
    if (st) break;
    if (fr.pos != count || fr.bs > si.total - count) {
      st = NPPC_FLAC_COUNT_MISMATCH;
      break;
    }
    auto it = cands.find(off);
    if (it == cands.end()) {
      std::fprintf(stderr, "a header the chain accepts was not a candidate (offset %ld)\n", off);
      std::exit(2);
    }
    st = it->second.status;
    if (st) break;
    if (it->second.end <= off) {
      std::fprintf(stderr, "a frame that does not advance (offset %ld)\n", off);
      std::exit(2);
    }
    accepted.push_back(off);
    count += fr.bs;
    off = it->second.end;
  }
  r.status = st;
  if (si.channels * si.total > MAX_OUT) {
    r.status = -1;
    return r;
  }
  r.pcm.assign((size_t)(si.channels * si.total), 0x5a5a5a5a);     // decode
  r.pcm.shrink_to_fit();
  r.mono.assign((size_t)si.total, -7.0f);
  r.mono.shrink_to_fit();
  for (long a : accepted) {
    FlacFrame fr;
    long end = 0;
    if (flac_parse_header(p, n, a, si, &fr) != NPPC_FLAC_OK ||
        flac_decode_frame<true>(p, n, a, si, fr, 0, r.pcm.data(), r.mono.data(), &end) != NPPC_FLAC_OK || end != cands[a].end) {
      std::fprintf(stderr, "an accepted frame does not decode as it parsed (offset %ld)\n", a);
      std::exit(2);
    }
  }
  return r;
}

long n_inputs = 0, n_ok = 0, n_status[16] = {};

// returns the serial status; dies when the two paths disagree or a status of 0 hides other samples than `want`
int check(const std::vector<uint8_t>& in, const Result* want) {
  uint8_t* p = (uint8_t*)std::malloc(in.size() ? in.size() : 1);  // exactly the file: one byte further is a report
  if (!in.empty()) std::memcpy(p, in.data(), in.size());
  const long n = (long)in.size();
  const Result a = serial(p, n), b = device_like(p, n);
  std::free(p);
  ++n_inputs;
  if (a.status != b.status) {
    std::fprintf(stderr, "input %ld: serial status %d, parallel status %d\n", n_inputs, a.status, b.status);
    std::exit(2);
  }
  if (a.status == 0) {
    ++n_ok;
    if (a.pcm != b.pcm || std::memcmp(a.mono.data(), b.mono.data(), a.mono.size() * sizeof(float)) != 0) {
      std::fprintf(stderr, "input %ld: the two paths give other samples\n", n_inputs);
      std::exit(2);
    }
    if (want && (a.pcm != want->pcm || a.si.total != want->si.total || a.si.channels != want->si.channels)) {
      std::fprintf(stderr, "input %ld: status 0 with samples that are not the original's\n", n_inputs);
      std::exit(2);
    }
  } else if (a.status > 0 && a.status < 16) {
    ++n_status[a.status];
  }
  return a.status;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

}  // namespace

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "tests/golden/flac_two_frame.flac";
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  std::vector<uint8_t> base;
  for (int c; (c = std::fgetc(f)) != EOF;) base.push_back((uint8_t)c);
  std::fclose(f);

  uint8_t* p = (uint8_t*)std::malloc(base.size());
  std::memcpy(p, base.data(), base.size());
  const Result want = serial(p, (long)base.size());
  FlacFrame first;
  const int hs = want.status ? 1 : flac_parse_header(p, (long)base.size(), want.si.first_frame, want.si, &first);
  std::free(p);
  if (want.status || hs) {
    std::fprintf(stderr, "%s does not decode: status %d\n", path, want.status);
    return 1;
  }
  if (check(base, &want) != 0) return 1;

  for (size_t cut = 0; cut < base.size(); ++cut) {                // every truncation is an error
    std::vector<uint8_t> in(base.begin(), base.begin() + cut);
    if (check(in, &want) == 0) {
      std::fprintf(stderr, "the stream cut to %zu bytes still decodes\n", cut);
      return 1;
    }
  }
  const size_t flip_bytes = base.size() < 600 ? base.size() : 600;
  for (size_t bit = 0; bit < flip_bytes * 8; ++bit) {             // a flip is an error or the original samples
    std::vector<uint8_t> in(base);
    in[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
    check(in, &want);
  }
  for (int i = 0; i < 4000; ++i) {                                // random payloads behind a valid frame header
    std::vector<uint8_t> in(base.begin(), base.begin() + first.hdr_end);
    const int len = (int)(rnd() % 400);
    const int mode = i % 4;                                       // all random; mostly zeros; mostly ones; a valid tail
    for (int k = 0; k < len; ++k) {
      const uint32_t r = rnd();
      in.push_back(mode == 0 ? (uint8_t)r : mode == 1 ? ((r & 7) ? 0 : (uint8_t)(r >> 8)) : mode == 2 ? ((r & 7) ? 0xff : (uint8_t)(r >> 8))
                                                                                                       : (uint8_t)r);
    }
    if (mode == 3) in.insert(in.end(), base.begin() + first.hdr_end + (len < 100 ? len : 100), base.end());
    check(in, nullptr);
  }
  for (int a = 2; a < argc; ++a) {                                // further files: as they are, whatever their status
    std::FILE* g = std::fopen(argv[a], "rb");
    if (!g) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 1;
    }
    std::vector<uint8_t> in;
    for (int c; (c = std::fgetc(g)) != EOF;) in.push_back((uint8_t)c);
    std::fclose(g);
    check(in, nullptr);
  }
  std::printf("flac_host_check: %ld inputs, %ld decoded (all exact), statuses", n_inputs, n_ok);
  for (int s = 1; s <= 8; ++s) std::printf(" %d:%ld", s, n_status[s]);
  std::printf("\n");
  return 0;
}
