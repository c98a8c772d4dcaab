// The MFMA tile core shared by the NT GEMMs (tcn.hip) and the implicit-GEMM convolutions (unet.hip): one copy each of the
// swizzled LDS image (stage load / store, fragment read), the two main loops and the per-element epilogues.  A kernel supplies
// where the operand rows of k-step `s` come from (a pair of source functors) and keeps what is its own: grid decoding,
// coalesced output staging, statistics reductions.  Every floating-point operation and its order are those of the kernels
// these pieces were taken from: the bit-for-bit tests rest on them.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ arguments
enum { EPI_PLAIN = 0, EPI_PRELU_STATS = 1, EPI_RESIDUAL = 2, EPI_RELU = 3, EPI_PLAIN_F32 = 4, EPI_MASK_POS = 5, EPI_RESIDUAL_GN = 6 };
// EPI_RESIDUAL_GN: the GroupNorm in front of the product is folded into it.  With a = (y - mean_b) * rstd_b * gamma + beta,
//   a W^T = rstd_b * (y Wg^T) - mean_b * rstd_b * v + u,   Wg[n][k] = gamma[k] W[n][k],  v[n] = sum_k Wg[n][k],  u[n] = sum_k beta[k] W[n][k] + bias[n]
// so the GEMM reads the un-normalised y (B operand = Wg, `bias` = u, `gnv` = v, `stats` = the per-sample (sum, sumsq) of y)
// and the normalised activation is never written (nppc_tcn_pack_sconv builds Wg, u, v).

struct GemmArgs {
  const void* A; long lda; long strideA;   // [R][lda]   (strides in elements, per batch z)
  const void* B; long ldb; long strideB;   // [N][ldb]
  void* C; long ldc; long strideC;         // [R][ldc]
  const float* bias; long strideBias;      // [N] or null
  const void* res; long ldres; long strideRes;  // residual [R][ldres] (EPI_RESIDUAL)
  const float* slope; long strideSlope;    // PReLU slope (1 value)
  double* stats; long strideStats;         // [R/Tp][2] (sum, sumsq) (EPI_PRELU_STATS)
  int R, N, K;                             // R % 128 == 0, N % 64 == 0, K % 32 == 0
  int Tp, Tv;                              // rows with (row % Tp) >= Tv are padding: forced to zero
  int Nv;                                  // columns >= Nv are padding: forced to zero
  int relu_in;                             // apply ReLU to A on load (TCN trailing nn.ReLU before the Linear)
  int ksplit;                              // >1: blockIdx.z = batch*ksplit + s; slice s covers K elements [s*K, (s+1)*K)
  const float* gnv; long strideGnv;        // EPI_RESIDUAL_GN: v[N]; `stats` then holds the GroupNorm (sum, sumsq) per sample
  double gcnt; float geps;                 // ... elements per sample, epsilon
  int staged;                              // LDS kernels, residual / mask epilogues: coalesced epilogue through LDS (ldc, ldres % 8 == 0)
  float* colpart; long strideColpart;      // optional (LDS kernels, EPI_RESIDUAL / EPI_MASK_POS): column sums of each 128-row tile of
                                           // the OUTPUT, [z][R/128][N] fp32 -- the bias gradient of the layer that consumes C as its
                                           // upstream gradient, without a pass of its own over C
};

struct ConvArgs {
  const void* A; long lda;            // haloed NHWC input, pointer at pixel row 0 (guard rows exist before it)
  const void* Wp;                     // packed weights [Np][ntap*Cin], K contiguous
  void* C; long ldc;                  // haloed NHWC output; interior rows, columns < Cout are written
  const float* bias;                  // [Cout] or null
  const float* scale;                 // optional folded BatchNorm (eval mode): v = leaky(v * scale[c] + shift[c])
  const float* shift;
  float slope;
  long P;                             // haloed pixel rows B*(H+2)*(W+2)
  int H, W, Cin, Cout, ntap;          // Cin % 32 == 0
  // optional (conv_tiled_kernel, conv_dma_kernel): per-tile column sums of the STORED output, [tile = row / 128][2: sum, sum of
  // squares][ldp] fp32 -- the batch statistics of the train-mode BatchNorm that follows, without a pass of its own over the tensor
  float* stat_part; int ldp;
};

// 32-bit arithmetic: the host entry points reject P >= 2^31 (64-bit integer division has no hardware support)
__device__ __forceinline__ bool interior(long p, long P, int H, int W) {
  if (p >= P) return false;
  const unsigned Wp = W + 2, Hp = H + 2, pu = (unsigned)p;
  const unsigned row = pu / Wp;
  const unsigned x = pu - row * Wp;
  const unsigned y = row % Hp;
  return x >= 1 && x <= (unsigned)W && y >= 1 && y <= (unsigned)H;
}

// row offset of tap t: (dy, dx) = (t/3 - 1, t%3 - 1) for a 3x3 kernel, 0 for 1x1 (arithmetic on a uniform value:
// a dynamically indexed array in the by-value argument struct would be copied to scratch / LDS)
__device__ __forceinline__ int tap_offset(const ConvArgs& g, int t) {
  return g.ntap == 9 ? (t / 3 - 1) * (g.W + 2) + (t % 3 - 1) : 0;
}

// XCD-aware tile order (grid.x is a multiple of 8) of a BM x BN output tile: workgroups are dealt round-robin to the 8 XCDs in
// linear id order; the gridDim.y channel tiles of one pixel tile run back to back on the SAME XCD, so the pixel rows are
// fetched from HBM once and re-read from that XCD's L2
template <int BM, int BN> __device__ __forceinline__ void xcd_tile(long& m0, int& n0) {
  const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
  const unsigned xcd = lin & 7, jj = lin >> 3;
  m0 = (long)((jj / gridDim.y) * 8 + xcd) * BM;
  n0 = (int)(jj % gridDim.y) * BN;
}

// ------------------------------------------------------------------------------------------------ operand fragments
template <typename T> __device__ __forceinline__ typename Frag<T>::type relu_frag(typename Frag<T>::type f);
template <> __device__ __forceinline__ bf16x8 relu_frag<bf16_t>(bf16x8 f) {
  u32x4 v = __builtin_bit_cast(u32x4, f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned x = v[i];
    if (x & 0x8000u) x &= 0xffff0000u;
    if (x & 0x80000000u) x &= 0x0000ffffu;
    v[i] = x;
  }
  return __builtin_bit_cast(bf16x8, v);
}
template <> __device__ __forceinline__ f32x8 relu_frag<float>(f32x8 f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = fmaxf(f[i], 0.f);
  return f;
}

// The LDS image of an operand tile: rows of 128 B = 8 chunks of 16 B (64 bf16 / 32 f32 of K), chunk c of row r stored at slot
// (c ^ (r & 7)): both the staging ds_write_b128 and the fragment ds_read_b128 are bank-conflict free.
// Fragment of 32-deep k-step `ks` of `row` for the lanes of quarter q = lane >> 4.
template <typename T>
__device__ __forceinline__ typename Frag<T>::type lds_frag(const unsigned char* base, int row, int ks, int q) {
  typedef typename Frag<T>::type frag;
  if constexpr (sizeof(T) == 2) {
    const int c = 4 * ks + q;
    return *reinterpret_cast<const frag*>(base + row * 128 + ((c ^ (row & 7)) << 4));
  } else {
    const int c0 = 2 * q, c1 = 2 * q + 1;   // KS == 1: the 32-float row is the whole k-step
    const float4 lo = *reinterpret_cast<const float4*>(base + row * 128 + ((c0 ^ (row & 7)) << 4));
    const float4 hi = *reinterpret_cast<const float4*>(base + row * 128 + ((c1 ^ (row & 7)) << 4));
    frag f;
    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    return f;
  }
}

// One thread's share of a 128 x (128 + BN) row stage on its way global -> registers -> LDS: chunk (tid & 7) of rows
// (tid >> 3) + 32 i of A (i = 0..3) and of B (i < BN / 32).  Named members: an indexed array would be demoted to scratch / LDS.
template <typename T, int BN> struct NtStage {
  u32x4 a0, a1, a2, a3, b0, b1, b2, b3;
  __device__ __forceinline__ void load(const T* pa, long lda, const T* pb, long ldb) {
    a0 = *reinterpret_cast<const u32x4*>(pa);
    a1 = *reinterpret_cast<const u32x4*>(pa + 32 * lda);
    a2 = *reinterpret_cast<const u32x4*>(pa + 64 * lda);
    a3 = *reinterpret_cast<const u32x4*>(pa + 96 * lda);
    b0 = *reinterpret_cast<const u32x4*>(pb);
    b1 = *reinterpret_cast<const u32x4*>(pb + 32 * ldb);
    if constexpr (BN == 128) {
      b2 = *reinterpret_cast<const u32x4*>(pb + 64 * ldb);
      b3 = *reinterpret_cast<const u32x4*>(pb + 96 * ldb);
    }
  }
  // p = the stage buffer + this thread's swizzled slot; image [A rows | B rows]
  __device__ __forceinline__ void store(unsigned char* p) const {
    *reinterpret_cast<u32x4*>(p) = a0;
    *reinterpret_cast<u32x4*>(p + 32 * 128) = a1;
    *reinterpret_cast<u32x4*>(p + 64 * 128) = a2;
    *reinterpret_cast<u32x4*>(p + 96 * 128) = a3;
    *reinterpret_cast<u32x4*>(p + 128 * 128) = b0;
    *reinterpret_cast<u32x4*>(p + 128 * 128 + 32 * 128) = b1;
    if constexpr (BN == 128) {
      *reinterpret_cast<u32x4*>(p + 128 * 128 + 64 * 128) = b2;
      *reinterpret_cast<u32x4*>(p + 128 * 128 + 96 * 128) = b3;
    }
  }
};

// ------------------------------------------------------------------------------------------------ main loops
// The MFMAs of one stage image `ta` ([A rows | B rows]) for wave (wm, wn): its 64 x BN/2 tile, k-steps in ascending order.
template <typename T, int BN>
__device__ __forceinline__ void nt_lds_stage_mma(f32x4 (&acc)[4][BN / 32], const unsigned char* ta, int wm, int wn, int n, int q,
                                                 int relu_in) {
  typedef typename Frag<T>::type frag;
  constexpr int KS = (128 / (int)sizeof(T)) / 32;   // 32-wide MFMA k-steps per stage
  constexpr int NJ = BN / 32;                       // 16-column MFMA tiles per wave
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    frag af[4], bf[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = lds_frag<T>(ta, wm * 64 + 16 * i + n, ks, q);
      if (relu_in) af[i] = relu_frag<T>(af[i]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = lds_frag<T>(ta + 128 * 128, wn * (BN / 2) + 16 * j + n, ks, q);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = mma16(af[i], bf[j], acc[i][j]);
  }
}

// LDS-staged NT main loop: 256 threads = 2 x 2 waves, block tile 128 x BN (wave tile 64 x BN/2), 128-byte K slices per stage,
// double-buffered LDS (lds: 2 * (128 + BN) * 128 bytes) with register staging (the next stage's global loads are issued before
// the MFMAs and written to LDS after them), one barrier per stage.  Operand tiles are read from HBM/L2 once per workgroup.
// a_of(s) / b_of(s): this thread's source of stage s = chunk (tid & 7) of row (tid >> 3) of the stage's A / B rows; they are
// called once per stage, in stage order, a_of before b_of, so a functor may walk its position incrementally.
// Ends with a barrier: the buffers are free for the caller's epilogue.
template <typename T, int BN, typename I, typename AOf, typename BOf>
__device__ __forceinline__ void nt_lds_mainloop(f32x4 (&acc)[4][BN / 32], unsigned char* lds, I nstage, long lda, long ldb,
                                                AOf a_of, BOf b_of, int relu_in) {
  constexpr int NJ = BN / 32;
  constexpr int STAGE = (128 + BN) * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = tid >> 3, sc = tid & 7;
  const int soff = srow * 128 + ((sc ^ (srow & 7)) << 4);   // (srow + 32*i) & 7 == srow & 7
  NtStage<T, BN> st;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const T* pa = a_of((I)0);
    st.load(pa, lda, b_of((I)0), ldb);
  }
  st.store(lds + soff);
  __syncthreads();
  for (I s = 0; s < nstage; ++s) {
    const int buf = (int)(s & 1);
    const unsigned char* ta = lds + buf * STAGE;
    if (s + 1 < nstage) {
      const T* pa = a_of(s + 1);
      st.load(pa, lda, b_of(s + 1), ldb);
    }
    nt_lds_stage_mma<T, BN>(acc, ta, wm, wn, n, q, relu_in);
    if (s + 1 < nstage) st.store(lds + (buf ^ 1) * STAGE + soff);
    __syncthreads();
  }
}

// nt_lds_mainloop with ONE stage image in LDS ((128 + BN) * 128 bytes): the next stage's global loads are issued before the
// MFMAs as there, the MFMAs read the image, then barrier, staging registers -> the same image, barrier.  The image, the
// fragment reads, the MFMA order and the functor contract are those of nt_lds_mainloop, so every accumulator is bit-identical
// to its; half the LDS buys a third or fourth workgroup per CU (more operand bytes in flight) for one more barrier per stage.
// Ends with a barrier as well.
template <typename T, int BN, typename I, typename AOf, typename BOf>
__device__ __forceinline__ void nt_lds_mainloop_1buf(f32x4 (&acc)[4][BN / 32], unsigned char* lds, I nstage, long lda, long ldb,
                                                     AOf a_of, BOf b_of, int relu_in) {
  constexpr int NJ = BN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = tid >> 3, sc = tid & 7;
  const int soff = srow * 128 + ((sc ^ (srow & 7)) << 4);
  NtStage<T, BN> st;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const T* pa = a_of((I)0);
    st.load(pa, lda, b_of((I)0), ldb);
  }
  st.store(lds + soff);
  __syncthreads();
  for (I s = 0; s < nstage; ++s) {
    const bool more = s + 1 < nstage;
    if (more) {
      const T* pa = a_of(s + 1);
      st.load(pa, lda, b_of(s + 1), ldb);
    }
    nt_lds_stage_mma<T, BN>(acc, lds, wm, wn, n, q, relu_in);
    __syncthreads();
    if (more) {
      st.store(lds + soff);
      __syncthreads();
    }
  }
}

// Register-pipelined NT main loop: 256 threads = 4 waves stacked over rows, wave tile 32 x 64 (block tile 128 x 64), fragments
// loaded straight from global memory two k-steps deep.  a_of(kk) / b_of(kk): this lane's fragment source of 32-deep k-step kk
// for A row (lane & 15) / B row (lane & 15) of the wave tile; called once per k-step, in order, a_of before b_of.
template <typename T, typename AOf, typename BOf>
__device__ __forceinline__ void nt_reg_mainloop(f32x4 (&acc)[2][4], int nk, long lda, long ldb, AOf a_of, BOf b_of, int relu_in) {
  typedef typename Frag<T>::type frag;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  frag a0[2], b0[4], a1[2], b1[4];
  auto ld = [&](frag(&a)[2], frag(&b)[4], int kk) {
    const T* pa = a_of(kk);
    const T* pb = b_of(kk);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) a[mi] = load_frag<T>(pa + (long)16 * mi * lda);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) b[ni] = load_frag<T>(pb + (long)16 * ni * ldb);
  };
  auto mm = [&](frag(&a)[2], frag(&b)[4]) {
    if (relu_in) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = relu_frag<T>(a[mi]);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mma16(a[mi], b[ni], acc[mi][ni]);
  };
  ld(a0, b0, 0);
  int kk = 0;
#pragma unroll 1
  for (; kk + 2 < nk; kk += 2) {
    ld(a1, b1, kk + 1);
    mm(a0, b0);
    ld(a0, b0, kk + 2);
    mm(a1, b1);
  }
  if (kk + 1 < nk) {
    ld(a1, b1, kk + 1);
    mm(a0, b0);
    mm(a1, b1);
  } else {
    mm(a0, b0);
  }
}

// ------------------------------------------------------------------------------------------------ NT epilogue
// The per-element epilogue of the NT GEMMs: bias, folded GroupNorm, PReLU / ReLU (act), then residual or mask, padding mask and
// the fp32-slab or rounded store (put).  The tile constants are derived once, in the constructor; m0 = first row of the
// workgroup's 128-row tile (EPI_RESIDUAL_GN: one sample per tile, Tp % 128 == 0).
template <typename T, int EPI> struct NtEpilogue {
  const GemmArgs& g;
  const float* bias;
  const float* gnv = nullptr;
  const T* res = nullptr;
  T* C;
  float* Cf;                                // EPI_PLAIN_F32: fp32 output (split-K slabs)
  float slope = 0.f, gn_rstd = 1.f, gn_mr = 0.f;
  __device__ __forceinline__ NtEpilogue(const GemmArgs& g_, int z, int m0) : g(g_) {
    C = reinterpret_cast<T*>(g.C) + (size_t)blockIdx.z * g.strideC;
    Cf = reinterpret_cast<float*>(g.C) + (size_t)blockIdx.z * g.strideC;
    bias = g.bias ? g.bias + (size_t)z * g.strideBias : nullptr;
    if (EPI == EPI_PRELU_STATS) slope = g.slope[(size_t)z * g.strideSlope];
    if (EPI == EPI_RESIDUAL_GN) {
      const double* st = g.stats + (size_t)z * g.strideStats + (size_t)(m0 / g.Tp) * 2;
      const double m = st[0] / g.gcnt, var = st[1] / g.gcnt - m * m;
      gn_rstd = (float)(1.0 / sqrt((var > 0 ? var : 0) + (double)g.geps));
      gn_mr = (float)m * gn_rstd;
      gnv = g.gnv + (size_t)z * g.strideGnv;
    }
    if (EPI == EPI_RESIDUAL || EPI == EPI_RESIDUAL_GN || EPI == EPI_MASK_POS) res = reinterpret_cast<const T*>(g.res) + (size_t)z * g.strideRes;
  }
  // the additive term of column `col` (0 in padding columns)
  __device__ __forceinline__ float col_bias(int col) const {
    const bool cvalid = col < g.Nv;
    const int cl = cvalid ? col : 0;        // padding columns: read column 0, select 0 (no divergent branch around the loads)
    float bv = bias ? bias[cl] : 0.f;
    if (EPI == EPI_RESIDUAL_GN) bv -= gn_mr * gnv[cl];
    if (!cvalid) bv = 0.f;
    return bv;
  }
  __device__ __forceinline__ float act(float a, float bv) const {
    float v = (EPI == EPI_RESIDUAL_GN ? gn_rstd * a : a) + bv;
    if (EPI == EPI_PRELU_STATS) v = v > 0.f ? v : slope * v;
    if (EPI == EPI_RELU) v = fmaxf(v, 0.f);
    return v;
  }
  // accumulator-layout store of element (row, col); returns the STORED (rounded) value
  __device__ __forceinline__ float put(float a, float bv, int row, int col) const { return put(a, bv, row, col, (row % g.Tp) < g.Tv); }
  // ... for a caller that knows whether `row` is a valid frame (rvalid) without dividing
  __device__ __forceinline__ float put(float a, float bv, int row, int col, bool rvalid) const {
    const bool valid = col < g.Nv && rvalid;
    float v = act(a, bv);
    if (EPI == EPI_RESIDUAL || EPI == EPI_RESIDUAL_GN) v += to_f32<T>(res[(size_t)row * g.ldres + col]);
    if (EPI == EPI_MASK_POS) {
      if (!(to_f32<T>(res[(size_t)row * g.ldres + col]) > 0.f)) v = 0.f;
    }
    if (!valid) v = 0.f;
    if (EPI == EPI_PLAIN_F32) {
      Cf[(size_t)row * g.ldc + col] = v;
      return v;
    }
    const T o = from_f32<T>(v);
    C[(size_t)row * g.ldc + col] = o;
    return to_f32<T>(o);
  }
};

// ------------------------------------------------------------------------------------------------ convolution epilogue
// a * b rounded on its own: never contracted into a fused multiply-add with a following addition
__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}


// Accumulator tile acc[MI][NJ] of a wave -> element (row0 + 16 i + r, col0 + 16 j): interior test, bias, folded BatchNorm +
// LeakyReLU, rounded store; st1 / st2 (zeroed by the caller) collect the sums and sums of squares of the STORED values per column slot j (the
// statistics of the stored (rounded) activations, as bn_stats_kernel read them).
template <typename T, int MI, int NJ>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& g, const f32x4 (&acc)[MI][NJ], long row0, int col0, float (&st1)[NJ],
                                              float (&st2)[NJ]) {
  T* C = reinterpret_cast<T*>(g.C);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = row0 + 16 * i + r;
      if (!interior(row, g.P, g.H, g.W)) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = col0 + 16 * j;
        if (col >= g.Cout) continue;
        float v = acc[i][j][r] + (g.bias ? g.bias[col] : 0.f);
        if (g.scale) {
          v = v * g.scale[col] + g.shift[col];
          v = v > 0.f ? v : g.slope * v;
        }
        const T o = from_f32<T>(v);
        C[row * g.ldc + col] = o;
        const float vo = to_f32<T>(o);
        st1[j] += vo;
        // fp32, 128-column tile (conv_tiled_kernel<float, 128>): the square is rounded before it is added.  That is what the
        // compiler made of this loop there (packed adds, no fused multiply-add) while it fuses everywhere else; written out so
        // that the fp32 batch statistics of the 128-wide layers stay bit for bit what they have been.
        if (sizeof(T) == 4 && NJ == 4) st2[j] += mul_unfused(vo, vo);
        else st2[j] += vo * vo;
      }
    }
}

// Column sums of TILES 128-row statistics tiles of a workgroup (waves wm = 2t, 2t + 1 cover tile t) -> g.stat_part: 16 rows per
// lane -> the four row groups of a wave (lanes n, n+16, n+32, n+48) -> the two waves along M through LDS (sp: 2 * TILES * 2 * BN
// floats of the operand buffers, free once every wave has left the main loop) -> one store per column.  Every wave of the
// workgroup calls it (one barrier); `compute` is false for waves that hold no accumulators.
template <int BN, int TILES>
__device__ __forceinline__ void conv_stat_part(const ConvArgs& g, float* sp, const float (&st1)[BN / 32], const float (&st2)[BN / 32],
                                               bool compute, int wm, int wn, long m0, int n0) {
  const int tid = threadIdx.x, n = tid & 15, q = (tid & 63) >> 4;
  if (compute) {
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) {
      float a = st1[j], b = st2[j];
      a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
      b += __shfl_xor(b, 16); b += __shfl_xor(b, 32);
      if (q == 0) {
        sp[(wm * 2 + 0) * BN + wn * (BN / 2) + 16 * j + n] = a;
        sp[(wm * 2 + 1) * BN + wn * (BN / 2) + 16 * j + n] = b;
      }
    }
  }
  __syncthreads();
  if (tid < TILES * BN) {
    const int t = tid / BN, c = tid % BN;
    if (m0 + 128 * t < g.P) {
      float* pt = g.stat_part + (size_t)(m0 / 128 + t) * 2 * g.ldp + n0 + c;
      pt[0] = sp[((2 * t) * 2 + 0) * BN + c] + sp[((2 * t + 1) * 2 + 0) * BN + c];
      pt[g.ldp] = sp[((2 * t) * 2 + 1) * BN + c] + sp[((2 * t + 1) * 2 + 1) * BN + c];
    }
  }
}
