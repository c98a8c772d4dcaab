// Counter-based Philox4x32-10 and the nn.Dropout keep rule built on it, shared by the MC-dropout forward
// (mc_pca.hip: dropout_kernel) and the training backward that regenerates the same bits (unet.hip: the fused
// dropout + BatchNorm + LeakyReLU backward).  One definition, so the forward and backward bits agree by construction.
#pragma once
#include <hip/hip_runtime.h>

struct philox_u4 {
  unsigned x, y, z, w;
};

__device__ __forceinline__ philox_u4 philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return philox_u4{c0, c1, c2, c3};
}

// the four random words of channels [4 * c4, 4 * c4 + 4) of pixel row r: counter (r, c4, stream), key = 64-bit seed.
// Channel 4 * c4 + i is kept iff word i >= dropout_threshold(p).
__device__ __forceinline__ philox_u4 dropout_bits4(long r, int c4, unsigned stream_id, unsigned seed_lo, unsigned seed_hi) {
  return philox4x32((unsigned)r, (unsigned)((unsigned long long)r >> 32), (unsigned)c4, stream_id, seed_lo, seed_hi);
}

// p * 2^32 clamped to the u32 range (host side): the keep test is `bits >= threshold`
static inline unsigned dropout_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}
