// Windowed-sinc resampling of ragged batches for gfx950 (nppc_audio/resample.py; specification
// tests/resample_ref.py): torchaudio's default Resample -- a Hann-windowed sinc bank of `new` phases applied as a strided
// convolution -- with the bank compressed to its live taps.
//   nppc_resample_sinc_shape   host only: the LDS a (ratio, tile) needs and whether it fits the budget
//   nppc_resample_sinc         one launch, grid (output tiles, B)
// The table is [new][stride] 32-bit words: (k0, count, taps[maxcount]) per phase, every tap outside [k0, k0 + count) of the
// full bank being exactly 0.0f.  A workgroup copies the table and its tile's input span into LDS, then every output is ONE
// fp32 fma chain over its phase's live taps in ascending k: no atomics, no workspace, the bits of an output depend on its
// item's samples alone (not on the tile, the batch or the run).
#include "common.h"
#include "nppc_hip.h"

namespace {

constexpr int RS_THREADS = 256;

// input blocks (of `orig` samples) a tile of `tile` consecutive outputs can touch: outputs j0 .. j0 + tile - 1 have
// i = j / new in [j0 / new, (j0 + tile - 1) / new], at most (tile - 1) / new + 2 values whatever j0 is
static inline long rs_blocks(int new_, int tile) { return (long)(tile - 1) / new_ + 2; }

__global__ __launch_bounds__(RS_THREADS) void resample_sinc_kernel(const float* __restrict__ x, long ldx,
                                                                   const long* __restrict__ lengths,
                                                                   const int* __restrict__ table, int orig, int new_, int width,
                                                                   int maxcount, int stride, int tile, float* __restrict__ y,
                                                                   long ldy) {
  extern __shared__ int rs_lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  long len = lengths ? lengths[b] : ldx;
  len = len < 0 ? 0 : (len > ldx ? ldx : len);
  const long out_len = (len * new_ + orig - 1) / orig;
  const long j0 = (long)blockIdx.x * tile;
  float* yb = y + (size_t)b * ldy;
  const long jend = j0 + tile < ldy ? j0 + tile : ldy;           // this tile's columns of y: [j0, jend)
  if (j0 >= out_len) {                                           // the whole tile lies past the item: zeros, nothing is read
    for (long j = j0 + tid; j < jend; j += RS_THREADS) yb[j] = 0.f;
    return;
  }
  const int tab_words = new_ * stride;
  int* tab = rs_lds;
  float* xs = reinterpret_cast<float*>(rs_lds + tab_words);
  for (int w = tid; w < tab_words; w += RS_THREADS) tab[w] = table[w];
  const int klen = 2 * width + orig;
  const long jlast = (jend < out_len ? jend : out_len) - 1;      // the last output this tile computes (>= j0)
  const long i_lo = j0 / new_, i_hi = jlast / new_;
  const long g0 = i_lo * orig - width;                           // the recording's sample at xs[0] (negative at the start)
  const int span = (int)(i_hi - i_lo) * orig + klen;             // <= rs_blocks * orig + klen - orig, what shape() sized
  const float* xb = x + (size_t)b * ldx;
  for (int s = tid; s < span; s += RS_THREADS) {
    const long n = g0 + s;
    xs[s] = (n >= 0 && n < len) ? xb[n] : 0.f;                   // out of range and past the item: zeros, never read
  }
  __syncthreads();
  const int jl0 = (int)(j0 - i_lo * new_);                       // < new
  for (int r = tid; r < tile; r += RS_THREADS) {
    const long j = j0 + r;
    if (j >= jend) break;
    float acc = 0.f;
    if (j < out_len) {
      const int jl = jl0 + r;
      const int ir = jl / new_, p = jl - ir * new_;
      const int* row = tab + p * stride;
      int cnt = row[1];
      cnt = cnt < 0 ? 0 : (cnt > maxcount ? maxcount : cnt);
      int k0 = row[0];
      k0 = k0 < 0 ? 0 : (k0 > klen - cnt ? klen - cnt : k0);
      const float* h = reinterpret_cast<const float*>(row + 2);
      const float* xp = xs + ir * orig + k0;
      for (int k = 0; k < cnt; ++k) acc = __fmaf_rn(xp[k], h[k], acc);
    }
    yb[j] = acc;
  }
}

}  // namespace

extern "C" {

int nppc_resample_sinc_shape(int orig, int new_, int width, int maxcount, int tile, int* stride, long* table_bytes,
                             long* span_elems, long* lds_bytes, int* fits) {
  if (orig <= 0 || new_ <= 0 || width <= 0 || maxcount <= 0 || tile <= 0) return NPPC_EBADARG;
  const long klen = 2L * width + orig;
  if (maxcount > klen) return NPPC_EBADARG;
  const long st = (2L + maxcount) | 1;                           // odd: consecutive phases start in different banks
  const long tbytes = (long)new_ * st * 4;
  const long span = (rs_blocks(new_, tile) - 1) * orig + klen;
  const long lds = tbytes + span * 4;
  if (stride) *stride = st > 0x7fffffff ? 0 : (int)st;
  if (table_bytes) *table_bytes = tbytes;
  if (span_elems) *span_elems = span;
  if (lds_bytes) *lds_bytes = lds;
  if (fits) *fits = (tbytes <= NPPC_RESAMPLE_TABLE_BUDGET && lds <= NPPC_RESAMPLE_LDS_BUDGET) ? 1 : 0;
  return NPPC_OK;
}

int nppc_resample_sinc(const float* x, long ldx, const long* lengths, int B, const int* table, int orig, int new_, int width,
                       int maxcount, int tile, float* y, long ldy, void* stream) {
  if (!x || !table || !y || ldx <= 0 || B <= 0 || ldy <= 0) return NPPC_EBADARG;
  int stride = 0, fits = 0;
  long lds = 0;
  const int rc = nppc_resample_sinc_shape(orig, new_, width, maxcount, tile, &stride, nullptr, nullptr, &lds, &fits);
  if (rc != NPPC_OK) return rc;
  if (!fits || B > 65535) return NPPC_EUNSUPPORTED;
  const long tiles = (ldy + tile - 1) / tile;
  if (tiles > 0x7fffffffL) return NPPC_EUNSUPPORTED;
  hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(RS_THREADS), (size_t)lds,
                     (hipStream_t)stream, x, ldx, lengths, table, orig, new_, width, maxcount, stride, tile, y, ldy);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
