// Sanitizer program of the whole-recording enhancement core (csrc/enhance_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/enhance_host_check.cc -o enhance_host_check && ./enhance_host_check
//
// The chunk waveforms, the tables and every output live in heap blocks of exactly their size (the last chunk holds only its
// last_length samples: the block ends there), so a read or a write one element outside any of them is an AddressSanitizer
// report.  Plans: K in {1, 2, 5, 16}, C in {2, 16, 18, 64}, n in {1, 2, 3, 6}, last chunks of H + 1 samples, of C samples
// and in between, one chunk shorter than C, A in {0, 1, 3}, both match modes, strided directions, and directions that are
// all zeros in an overlap.  The serial core (enh_chain_serial, enh_splice_serial: the functions the kernels walk) is
// compared with an implementation of the rule in this file that works chunk by chunk: it sorts the cosines of a boundary to
// match them, and it lays every chunk down whole and then cross-fades the overlaps in place.  Exit status 0 and a line of
// counts.  The posterior sampler's workgroups (csrc/enhance_post.hip) own blocks of output samples that divide H
// (enh_block_ok): walk_blocks visits every block of every such plan the way a workgroup does, from enh_locate of its first
// sample alone, reads the (at most two) chunks it names from heap blocks of exactly their lengths, writes a recording of
// exactly L samples and holds every sample against enh_locate of that sample.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "enhance_core.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
float unit() { return (float)((int)(rnd() % 20001u) - 10000) / 10000.f; }

[[noreturn]] void fail(const char* what, long a = 0, long b = 0, long c = 0) {
  fprintf(stderr, "enhance_host_check: %s (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}

template <class T>
T* exact(const std::vector<T>& v) {                               // a heap block of exactly v.size() elements (at least one byte)
  T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
  if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

float mulf(float a, float b) { volatile float r = a * b; return r; }
float addf(float a, float b) { volatile float r = a + b; return r; }

struct Plan {
  int n, K, C, last, A, match;
  bool strided, zero;
};

long run(const Plan& pl) {
  const int n = pl.n, K = pl.K, C = pl.C, H = C / 2, A = pl.A;
  const long L = (long)(n - 1) * H + pl.last;
  // directions: [n][K][pad] with pad = C (or C + 3 when strided); the block ends with the last chunk's last sample
  const long p_ks = pl.strided ? C + 3 : C, p_cs = p_ks * K, e_cs = C;
  std::vector<float> enh((size_t)(n - 1) * e_cs + pl.last), pcs((size_t)(n - 1) * p_cs + (K - 1) * p_ks + pl.last);
  for (auto& v : enh) v = unit();
  for (auto& v : pcs) v = unit();
  // shared content in the overlaps, under a random signed permutation, so that the chain has something to find
  for (int c = 1; c < n; ++c) {
    std::vector<int> perm(K);
    for (int k = 0; k < K; ++k) perm[k] = k;
    for (int k = K - 1; k > 0; --k) std::swap(perm[k], perm[rnd() % (uint32_t)(k + 1)]);
    for (int k = 0; k < K; ++k) {
      const float sg = (rnd() & 1) ? 1.f : -1.f;
      for (int i = 0; i < H; ++i)
        pcs[c * p_cs + k * p_ks + i] = sg * pcs[(c - 1) * p_cs + perm[k] * p_ks + H + i] + 0.05f * unit();
    }
  }
  if (pl.zero && n >= 2) {
    for (int i = 0; i < H; ++i) pcs[1 * p_cs + (K - 1) * p_ks + i] = 0.f;                 // a b row of boundary 1
    if (n >= 3) for (int i = 0; i < H; ++i) pcs[1 * p_cs + 0 * p_ks + H + i] = 0.f;       // an a row of boundary 2
  }
  std::vector<float> alphas(A), w(H);
  for (int a = 0; a < A; ++a) alphas[a] = 3.f * unit();
  for (int i = 0; i < H; ++i) w[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)C));
  float *d_enh = exact(enh), *d_pcs = exact(pcs), *d_al = exact(alphas), *d_w = exact(w);
  int* perm = (int*)malloc(sizeof(int) * n * K);
  int* sign = (int*)malloc(sizeof(int) * n * K);
  double* cont = (double*)malloc(n > 1 ? sizeof(double) * (n - 1) * K : 1);
  double* gram = (double*)malloc(n > 1 ? sizeof(double) * (n - 1) * ENH_E(K) : 1);
  enh_chain_serial(d_pcs, p_cs, p_ks, n, K, C, pl.match, perm, sign, cont, gram);

  // the chain again: per boundary, every (|cos|, j, k) sorted, slots served in order
  std::vector<int> rp(n * K), rs(n * K);
  for (int s = 0; s < K; ++s) rp[s] = s, rs[s] = 1;
  for (int c = 1; c < n; ++c) {
    const double* g = gram + (long)(c - 1) * ENH_E(K);
    std::vector<char> taken(K, 0);
    for (int s = 0; s < K; ++s) {
      const int j = rp[(c - 1) * K + s];
      int k = j;
      if (pl.match == ENH_MATCH_GREEDY) {
        std::vector<std::pair<double, int>> cand;
        for (int q = 0; q < K; ++q)
          if (!taken[q]) {
            const double d = g[K * K + j] * g[K * K + K + q];
            cand.push_back({d == 0.0 ? 0.0 : -fabs(g[j * K + q] / sqrt(d)), q});
          }
        k = std::min_element(cand.begin(), cand.end())->second;   // largest |cos|, then lowest k
      }
      taken[k] = 1;
      rp[c * K + s] = k;
      rs[c * K + s] = rs[(c - 1) * K + s] * (g[j * K + k] >= 0.0 ? 1 : -1);
      const double d = g[K * K + j] * g[K * K + K + k];
      const double want = d == 0.0 ? 0.0 : fabs(g[j * K + k] / sqrt(d));
      if (cont[(c - 1) * K + s] != want) fail("continuity", c, s);
      if (!(want >= 0.0 && want <= 1.0 + 1e-12)) fail("a cosine outside [0, 1]", c, s);
    }
  }
  for (int q = 0; q < n * K; ++q)
    if (perm[q] != rp[q] || sign[q] != rs[q]) fail("perm / sign", q, perm[q], rp[q]);
  if (pl.zero && n >= 2 && K > 1) {
    int zeros = 0;
    for (int s = 0; s < K; ++s) zeros += cont[s] == 0.0;
    if (zeros != 1) fail("a zero direction of boundary 1 is matched once, last", zeros);
  }

  // the splice again: every chunk laid down whole, later chunks cross-faded over the H samples they share
  const int V = 1 + K * A;
  float* out = (float*)malloc(sizeof(float) * V * L);
  EnhChunks q{d_enh, d_pcs, e_cs, p_cs, p_ks, n, A ? K : 0, C, L};
  enh_splice_serial(q, d_al, A, d_w, perm, sign, out, L);
  std::vector<float> ref((size_t)V * L);
  for (int v = 0; v < V; ++v) {
    const int s = v ? (v - 1) / A : 0, a = v ? (v - 1) % A : 0;
    for (int c = 0; c < n; ++c) {
      const int len = c == n - 1 ? pl.last : C;
      for (int i = 0; i < len; ++i) {
        float y = enh[c * e_cs + i];
        if (v) y = addf(y, mulf(mulf(alphas[a], (float)rs[c * K + s]), pcs[c * p_cs + rp[c * K + s] * p_ks + i]));
        float& o = ref[(size_t)v * L + (long)c * H + i];
        o = (c >= 1 && i < H) ? addf(mulf(o, addf(1.f, -w[i])), mulf(y, w[i])) : y;
      }
    }
  }
  for (long m = 0; m < (long)V * L; ++m)
    if (memcmp(&ref[m], &out[m], 4)) fail("splice", m / L, m % L);
  free(d_enh), free(d_pcs), free(d_al), free(d_w), free(perm), free(sign), free(cont), free(gram), free(out);
  return (long)V * L;
}

// blocks of `block` samples over the plan (n, C, last): -> samples visited
long walk_blocks(int n, int C, int last, int block) {
  const int H = C / 2;
  const long L = (long)(n - 1) * H + last;
  if (!enh_block_ok(C, block) || !enh_plan_ok(n, 0, C, L)) fail("walk_blocks: not a plan", n, C, block);
  std::vector<float*> chunk(n);
  for (int c = 0; c < n; ++c) {
    const int len = c == n - 1 ? last : C;
    chunk[c] = (float*)malloc(sizeof(float) * len);
    for (int i = 0; i < len; ++i) chunk[c][i] = (float)(c * C + i);
  }
  float* out = (float*)malloc(sizeof(float) * L);
  float* w = (float*)malloc(sizeof(float) * (H > 0 ? H : 1));
  for (int i = 0; i < H; ++i) w[i] = 0.25f;
  long seen = 0;
  for (long m0 = 0; m0 < L; m0 += block) {
    int cur, i0;
    const bool blend = enh_locate(m0, H, n, &cur, &i0);
    if (i0 % block) fail("a block off the chunk's block grid", m0, i0, block);
    for (int e = 0; e < block && m0 + e < L; ++e, ++seen) {
      int c1, i1;
      const bool b1 = enh_locate(m0 + e, H, n, &c1, &i1);
      if (c1 != cur || i1 != i0 + e || b1 != blend) fail("a block straddles a region", m0, e, c1);
      const float yc = chunk[cur][i0 + e];
      out[m0 + e] = blend ? enh_blend(chunk[cur - 1][i0 + e + H], yc, w[i0 + e]) : yc;
    }
  }
  for (int c = 0; c < n; ++c) free(chunk[c]);
  free(out), free(w);
  if (seen != L) fail("walk_blocks: samples missed", seen, L);
  return seen;
}

}  // namespace

int main() {
  long plans = 0, samples = 0;
  const int Ks[] = {1, 2, 5, 16}, Cs[] = {2, 16, 18, 64}, ns[] = {1, 2, 3, 6}, As[] = {0, 1, 3};
  for (int K : Ks)
    for (int C : Cs)
      for (int n : ns)
        for (int A : As)
          for (int match = 0; match < 2; ++match) {
            const int H = C / 2;
            std::vector<int> lasts = {C};
            if (n == 1) lasts.push_back(1), lasts.push_back(H);
            else if (H + 1 < C) lasts.push_back(H + 1), lasts.push_back(H + 1 + (C - H - 1) / 2);
            for (int last : lasts)
              for (int flags = 0; flags < 4; ++flags) {
                samples += run(Plan{n, K, C, last, A, match, (flags & 1) != 0, (flags & 2) != 0});
                ++plans;
              }
          }
  if (!enh_plan_ok(1, 0, 2, 1) || enh_plan_ok(0, 1, 16, 8) || enh_plan_ok(3, 1, 15, 20) || enh_plan_ok(3, 17, 16, 20) ||
      enh_plan_ok(3, 1, 16, 16) || enh_plan_ok(3, 1, 16, 33) || !enh_plan_ok(3, 1, 16, 32))
    fail("enh_plan_ok");
  long walked = 0, walks = 0;
  for (int C : {2, 16, 64, 1024})
    for (int n : ns)
      for (int block : {1, 2, 4, 8, 128, 512}) {
        const int H = C / 2;
        if (H % block) {
          if (enh_block_ok(C, block)) fail("enh_block_ok takes a block that does not divide H", C, block);
          continue;
        }
        std::vector<int> lasts = {C};
        if (n == 1) lasts.push_back(1), lasts.push_back(H);
        else if (H + 1 < C) lasts.push_back(H + 1), lasts.push_back(C - 1);
        for (int last : lasts) walked += walk_blocks(n, C, last, block), ++walks;
      }
  if (enh_block_ok(16, 0) || enh_block_ok(15, 1) || enh_block_ok(16, 3) || !enh_block_ok(1024, 128)) fail("enh_block_ok");
  printf("enhance_host_check: %ld plans, %ld output samples, all equal; %ld block walks, %ld samples\n", plans, samples, walks,
         walked);
  return 0;
}
