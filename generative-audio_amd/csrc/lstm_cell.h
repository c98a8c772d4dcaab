// Per-cell code shared by the fused 2-layer LSTM kernels (lstm.hip, lstm_coop.hip).
#pragma once
#include "common.h"

// Backward of one LSTM cell.  Saved post-activation gates (i, g, f, o), this step's cell state ct, the previous one cp
// (0 at t = 0) and dh = d loss / d h_t (recurrent + external) -> the pre-activation gate gradients.  dc carries
// d loss / d c from step to step: it comes in as the gradient that flowed back from step t + 1 and leaves as the one
// for step t - 1.  It is updated HERE, not returned as a contribution for the caller to add: the expression shape
// (one fused multiply-add into dct) is what the bit-for-bit comparisons between the backward kernels rest on.
__device__ __forceinline__ void lstm_cell_bwd(float iv, float gv, float fv, float ov, float ct, float cp, float dh, float& dc,
                                              float& di, float& dg, float& df, float& dO) {
  const float tc = tanh_f(ct);
  const float dct = dh * ov * (1.f - tc * tc) + dc;
  dO = dh * tc * ov * (1.f - ov);
  di = dct * gv * iv * (1.f - iv);
  dg = dct * iv * (1.f - gv * gv);
  df = dct * cp * fv * (1.f - fv);
  dc = dct * fv;
}

// the four gate values of one (row, unit): one 16-byte (fp32) or 8-byte (bf16) store
template <typename T> __device__ __forceinline__ void store_gates(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store_gates<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void store_gates<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  uint2 v;
  v.x = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
  v.y = (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16);
  *reinterpret_cast<uint2*>(p) = v;
}
