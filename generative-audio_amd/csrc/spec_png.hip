// Spectrogram sheets rendered and written as PNG on gfx950 (nppc_audio/png.py, nppc_audio/spectrogram_png.py, DESIGN.md
// section 8l).  Every decision of the PNG writer is csrc/png_core.h, shared with the serial host encoder below and with
// tools/check/png_host_check.cc; specification tests/png_ref.py.
//   nppc_png_bound / nppc_png_encode_host   host only
//   nppc_png_encode       a ragged batch of device index images -> PNG files back to back:
//     png_plan    one workgroup per tile of PNG_TILE bytes of the filtered stream: the tile's token bits and Adler sums
//     png_scan    one workgroup: every tile's bit offset inside its image, every file's Adler-32, begin and end
//     png_write   one workgroup per tile: the tokens OR-ed (LSB first) into a cleared LDS buffer at the tile's bit offset,
//                 32-bit stores; the first and last word of a tile are shared with its neighbours and go by integer atomicOr
//     png_finish  one workgroup per file: signature, IHDR, PLTE, IDAT's length, the CRC-32 of IDAT from per-thread pieces
//                 moved to the end by the polynomial's linearity, Adler-32, IEND
//   nppc_spec_windows     the context window and the gap markers of every item, from the mask
//   nppc_spec_render      layout (W, H of every image), autoscale (finite minimum and maximum of a cell), render (indices)
//   nppc_spec_render_png  nppc_spec_render then nppc_png_encode
// A run of equal bytes that crosses a tile boundary is followed to its true first and last byte (the whole workgroup looks
// back / ahead PNG_TILE bytes at a time), and png_emit is a function of (byte, position in the run, run length): the bytes
// do not depend on the tiling.  There is no float atomic and no kernel waits for another workgroup; integer atomics only
// OR disjoint bits or take a maximum: two runs give identical bytes, and a file's bytes do not depend on its neighbours.
// LDS per workgroup: png_write 4096 (stream) + 4624 (bits) + 3 KiB (scans) = 11.8 KiB, png_plan 7.1 KiB, png_finish 2 KiB,
// all static.
#include <math.h>

#include "common.h"
#include "nppc_hip.h"
#include "png_core.h"

namespace {

constexpr int T = 256;
constexpr int PER = PNG_TILE / T;                                  // 16 stream bytes per thread
constexpr int BUFW = (9 * PNG_TILE + 3 + 31) / 32 + 2;             // words of a tile's bits at any bit offset
constexpr int NONE = 0x7fffffff;
typedef unsigned long long u64;
struct Plte {
  unsigned char b[PNG_PLTE];
};

struct Img {
  const unsigned char* idx;
  long W, H, n;
};

__device__ bool image_of(const long* meta, int nimg, int i, const unsigned char* pix, long pix_elems, Img* im) {
  if (i < 0 || i >= nimg) return false;
  const long po = meta[4L * i], W = meta[4L * i + 1], H = meta[4L * i + 2];
  if (!png_dims_ok(W, H) || po < 0 || po > pix_elems - W * H) return false;
  im->idx = pix + po, im->W = W, im->H = H, im->n = png_stream_len(W, H);
  return true;
}

// The tile's view of the stream: its bytes in LDS and, for the runs that leave the tile, their true first and last byte.
struct Tile {
  long i0;                                                         // the tile's first byte in the stream
  int len;
  long back, fwd;                                                  // first byte of the run of byte 0, last byte of the run of byte len - 1
};

// the first byte of the run that holds byte i - 1 (value v), i > 0: the whole workgroup looks back PNG_TILE bytes at a time
__device__ long run_back(const Img& im, long i, unsigned v, int* found) {
  for (long base = i; base > 0; base -= PNG_TILE) {
    __syncthreads();
    if (threadIdx.x == 0) *found = -1;
    __syncthreads();
    int best = -1;
    for (int k = 0; k < PER; ++k) {
      const int d = (int)threadIdx.x * PER + k;                    // distance below base - 1
      const long pos = base - 1 - d;
      if (pos >= 0 && png_filt(im.idx, im.W, pos) != v && PNG_TILE - 1 - d > best) best = PNG_TILE - 1 - d;
    }
    if (best >= 0) atomicMax(found, best);
    __syncthreads();
    const int f = *found;
    if (f >= 0) return base - PNG_TILE + f + 1;                    // the byte behind the nearest different one
  }
  return 0;
}
// the last byte of the run that holds byte i (value v), i < n
__device__ long run_fwd(const Img& im, long i, unsigned v, int* found) {
  for (long base = i; base < im.n; base += PNG_TILE) {
    __syncthreads();
    if (threadIdx.x == 0) *found = -1;
    __syncthreads();
    int best = -1;
    for (int k = 0; k < PER; ++k) {
      const int d = (int)threadIdx.x * PER + k;
      const long pos = base + d;
      if (pos < im.n && png_filt(im.idx, im.W, pos) != v && PNG_TILE - 1 - d > best) best = PNG_TILE - 1 - d;
    }
    if (best >= 0) atomicMax(found, best);
    __syncthreads();
    const int f = *found;
    if (f >= 0) return base + (PNG_TILE - 1 - f) - 1;
  }
  return im.n - 1;
}

struct TileLds {
  unsigned char s[PNG_TILE];
  int last_start[T];                                               // inclusive maximum over the threads up to t
  int first_end[T];                                                // inclusive minimum over the threads from t
  unsigned scan[T];
  int found;
};

__device__ __forceinline__ bool starts(const TileLds& L, const Tile& tl, int j, int prev) {
  return j ? L.s[j] != L.s[j - 1] : prev != (int)L.s[0];
}
__device__ __forceinline__ bool ends(const TileLds& L, const Tile& tl, int j, int next) {
  return j + 1 < tl.len ? L.s[j] != L.s[j + 1] : next != (int)L.s[j];
}

// loads the tile and resolves the runs; every thread returns with the same Tile.  prev / next: the bytes around the tile, -1
// at the stream's ends
__device__ void tile_load(const Img& im, long i0, TileLds& L, Tile* tl, int* prev, int* next) {
  const int t = threadIdx.x;
  tl->i0 = i0;
  tl->len = im.n - i0 < PNG_TILE ? (int)(im.n - i0) : PNG_TILE;
  for (int j = t; j < tl->len; j += T) L.s[j] = (unsigned char)png_filt(im.idx, im.W, i0 + j);
  *prev = i0 > 0 ? (int)png_filt(im.idx, im.W, i0 - 1) : -1;
  *next = i0 + tl->len < im.n ? (int)png_filt(im.idx, im.W, i0 + tl->len) : -1;
  __syncthreads();
  const int c0 = t * PER, c1 = c0 + PER < tl->len ? c0 + PER : tl->len;
  int ls = -1, fe = NONE;
  for (int j = c0; j < c1; ++j) {
    if (starts(L, *tl, j, *prev)) ls = j;
    if (fe == NONE && ends(L, *tl, j, *next)) fe = j;
  }
  L.last_start[t] = ls, L.first_end[t] = fe;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const int a = t >= d ? L.last_start[t - d] : -1, b = t + d < T ? L.first_end[t + d] : NONE;
    __syncthreads();
    if (a > L.last_start[t]) L.last_start[t] = a;
    if (b < L.first_end[t]) L.first_end[t] = b;
    __syncthreads();
  }
  // uniform: prev, next and s[] are the same for every thread
  tl->back = *prev == (int)L.s[0] ? run_back(im, i0, L.s[0], &L.found) : i0;
  tl->fwd = *next == (int)L.s[tl->len - 1] ? run_fwd(im, i0 + tl->len, L.s[tl->len - 1], &L.found) : i0 + tl->len - 1;
  __syncthreads();
}

__device__ __forceinline__ void lds_put(unsigned* buf, long bit, unsigned v, int n) {     // LSB first, 0 <= n <= 24, v < 2^n
  if (!v) return;
  const int w = (int)(bit >> 5), r = (int)(bit & 31);
  const u64 x = (u64)v << r;
  const unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);
  if (lo) atomicOr(&buf[w], lo);
  if (hi) atomicOr(&buf[w + 1], hi);
}

// this thread's 16 bytes, run by run: returns their bits; with buf, puts them at bit `at` of buf
__device__ long tile_walk(const TileLds& L, const Tile& tl, int prev, int next, unsigned* buf, long at) {
  const int t = threadIdx.x, c0 = t * PER, c1 = c0 + PER < tl.len ? c0 + PER : tl.len;
  if (c0 >= c1) return 0;
  long start;                                                      // the run of byte c0
  if (starts(L, tl, c0, prev)) start = tl.i0 + c0;
  else {
    const int before = t ? L.last_start[t - 1] : -1;
    start = before >= 0 ? tl.i0 + before : tl.back;
  }
  long bits = 0;
  int j = c0;
  while (j < c1) {
    int e = j;
    while (e < c1 && !ends(L, tl, e, next)) ++e;
    long end;                                                      // the run's last byte
    int seg;                                                       // the last byte of it in this chunk
    if (e < c1) end = tl.i0 + e, seg = e;
    else {
      const int after = t + 1 < T ? L.first_end[t + 1] : NONE;
      end = after != NONE ? tl.i0 + after : tl.fwd;
      seg = c1 - 1;
    }
    const long len = end - start + 1;
    const unsigned v = L.s[j];
    for (int q = j; q <= seg; ++q) {
      int nb;
      const unsigned code = png_emit(v, tl.i0 + q - start, len, &nb);
      if (buf) lds_put(buf, at + bits, code, nb);
      bits += nb;
    }
    j = seg + 1;
    start = tl.i0 + j;
  }
  return bits;
}

__device__ bool tile_of(long g, const int* ttab, const long* meta, int nimg, const unsigned char* pix, long pix_elems, Img* im,
                        long* i0) {
  const int i = ttab[2 * g], number = ttab[2 * g + 1];
  if (number < 0 || !image_of(meta, nimg, i, pix, pix_elems, im)) return false;
  *i0 = (long)number * PNG_TILE;
  return *i0 < im->n;
}

// plan [ntiles][4]: token bits, Adler a, Adler b, bytes of the tile (all 0 for a tile past its image's end)
__global__ __launch_bounds__(T) void png_plan_kernel(const unsigned char* __restrict__ pix, long pix_elems, const long* __restrict__ meta,
                                                     int nimg, const int* __restrict__ ttab, int* __restrict__ plan) {
  __shared__ TileLds L;
  __shared__ unsigned sums[3];
  const long g = blockIdx.x;
  const int t = threadIdx.x;
  Img im;
  long i0;
  if (!tile_of(g, ttab, meta, nimg, pix, pix_elems, &im, &i0)) {
    if (t < 4) plan[4 * g + t] = 0;
    return;
  }
  if (t < 3) sums[t] = 0;
  Tile tl;
  int prev, next;
  tile_load(im, i0, L, &tl, &prev, &next);
  const unsigned bits = (unsigned)tile_walk(L, tl, prev, next, nullptr, 0);
  unsigned a = 0, b = 0;                                           // at most 16 * 255 and 16 * 4096 * 255
  for (int j = t * PER; j < t * PER + PER && j < tl.len; ++j) a += L.s[j], b += (unsigned)(tl.len - j) * L.s[j];
  atomicAdd(&sums[0], bits), atomicAdd(&sums[1], a), atomicAdd(&sums[2], b);   // below 2^32: 4096 * 4097 / 2 * 255
  __syncthreads();
  if (t == 0) {
    plan[4 * g] = (int)sums[0], plan[4 * g + 1] = (int)(sums[1] % PNG_ADLER), plan[4 * g + 2] = (int)(sums[2] % PNG_ADLER);
    plan[4 * g + 3] = tl.len;
  }
}

// stats [nimg + 1][4]: file begin, file end, Adler-32, token bits; stats[nimg][0] = the batch's bytes.  toff [ntiles]: the
// tile's first bit inside its deflate block
constexpr int ST = 1024;
__global__ __launch_bounds__(ST) void png_scan_kernel(const int* __restrict__ plan, const int* __restrict__ tfirst, const long* __restrict__ meta,
                                                      int nimg, long ntiles, long* __restrict__ toff, long* __restrict__ stats) {
  __shared__ long part[ST];
  const int t = threadIdx.x;
  const int chunk = (nimg + ST - 1) / ST, f0 = t * chunk, f1 = f0 + chunk < nimg ? f0 + chunk : nimg;
  long sum = 0;
  for (int f = f0; f < f1; ++f) {
    long g0 = tfirst[f], g1 = tfirst[f + 1];
    g0 = g0 < 0 ? 0 : g0, g1 = g1 > ntiles ? ntiles : g1;
    long run = 3;
    unsigned A = 1, B = 0;
    for (long g = g0; g < g1; ++g) {
      toff[g] = run;
      run += plan[4 * g];
      png_adler_append(&A, &B, (unsigned)plan[4 * g + 1], (unsigned)plan[4 * g + 2], plan[4 * g + 3]);
    }
    const bool ok = png_dims_ok(meta[4L * f + 1], meta[4L * f + 2]) && g1 > g0;
    stats[4L * f + 1] = ok ? png_file_bytes(run - 3) : 0;         // the size, until the offsets are known
    stats[4L * f + 2] = ((long)B << 16) | A;
    stats[4L * f + 3] = run - 3;
    sum += stats[4L * f + 1];
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long run = 0;
    for (int i = 0; i < ST; ++i) {
      const long v = part[i];
      part[i] = run;
      run += v;
    }
    stats[4L * nimg] = run;
  }
  __syncthreads();
  long run = part[t];
  for (int f = f0; f < f1; ++f) {
    const long size = stats[4L * f + 1];
    stats[4L * f] = run, stats[4L * f + 1] = run + size;
    run += size;
  }
}

__global__ __launch_bounds__(T) void png_write_kernel(const unsigned char* __restrict__ pix, long pix_elems, const long* __restrict__ meta,
                                                      int nimg, const int* __restrict__ ttab, const int* __restrict__ plan,
                                                      const long* __restrict__ toff, const long* __restrict__ stats,
                                                      unsigned char* __restrict__ out, long out_cap) {
  __shared__ TileLds L;
  __shared__ unsigned buf[BUFW];
  const long g = blockIdx.x;
  const int t = threadIdx.x;
  Img im;
  long i0;
  if (!tile_of(g, ttab, meta, nimg, pix, pix_elems, &im, &i0)) return;
  const int f = ttab[2 * g];
  const long begin = stats[4L * f], end = stats[4L * f + 1], rel = toff[g];
  const int nbits = plan[4 * g];
  // everything the tile's place depends on is checked: a plan that is not this tile's writes nothing
  if (begin < 0 || end > out_cap || end - begin != png_file_bytes(stats[4L * f + 3]) || rel < 3 || nbits < 0 || nbits > 9 * PNG_TILE ||
      rel + nbits > 3 + stats[4L * f + 3])
    return;
  for (int i = t; i < BUFW; i += T) buf[i] = 0;
  Tile tl;
  int prev, next;
  tile_load(im, i0, L, &tl, &prev, &next);
  const long mine = tile_walk(L, tl, prev, next, nullptr, 0);
  L.scan[t] = (unsigned)mine;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const unsigned v = t >= d ? L.scan[t - d] : 0u;
    __syncthreads();
    L.scan[t] += v;
    __syncthreads();
  }
  if (L.scan[T - 1] != (unsigned)nbits) return;                   // uniform
  // bit `abs` of the output buffer (LSB first inside little-endian words): the tile's first bit; the header bits ride in tile 0
  const long first = rel == 3 && i0 == 0 ? 0 : rel;
  const long abs0 = 8 * (begin + PNG_HEAD) + first, abs1 = 8 * (begin + PNG_HEAD) + rel + nbits;
  const long w0 = abs0 >> 5, w1 = (abs1 + 31) >> 5;                // words [w0, w1)
  if (w1 - w0 > BUFW) return;
  const long base = w0 << 5;
  if (t == 0 && first == 0) lds_put(buf, abs0 - base, 3u, 3);      // BFINAL = 1, BTYPE = 01
  tile_walk(L, tl, prev, next, buf, 8 * (begin + PNG_HEAD) + rel - base + (t ? (long)L.scan[t - 1] : 0L));
  __syncthreads();
  unsigned* dst = reinterpret_cast<unsigned*>(out) + w0;          // out is 4-byte aligned (checked by the entry point)
  for (long w = t; w < w1 - w0; w += T) {
    if (w == 0 || w == w1 - w0 - 1) {
      if (buf[w]) atomicOr(&dst[w], buf[w]);                       // shared with the neighbour tiles, or with the zlib header
    } else {
      dst[w] = buf[w];
    }
  }
}

__global__ __launch_bounds__(T) void png_finish_kernel(const long* __restrict__ meta, int nimg, const long* __restrict__ stats, Plte plte,
                                                       unsigned char* __restrict__ out, long out_cap) {
  __shared__ unsigned table[256];
  __shared__ unsigned acc;
  __shared__ unsigned char head[48];
  const int f = blockIdx.x, t = threadIdx.x;
  const long W = meta[4L * f + 1], H = meta[4L * f + 2];
  const long begin = stats[4L * f], end = stats[4L * f + 1], bits = stats[4L * f + 3];
  if (!png_dims_ok(W, H) || begin < 0 || end > out_cap || bits < 0 || end - begin != png_file_bytes(bits)) return;
  const long db = png_deflate_bytes(bits);
  const unsigned adler = (unsigned)stats[4L * f + 2];
  unsigned char* file = out + begin;
  table[t] = png_crc_entry((unsigned)t);
  if (t == 0) {
    acc = 0;
    png_ihdr(head, W, H);
    png_idat_head(head + 33, db);
  }
  __syncthreads();
  for (int i = t; i < 33; i += T) file[i] = head[i];
  for (int i = t; i < PNG_PLTE; i += T) file[33 + i] = plte.b[i];
  // IDAT's length and type, 78 01: the deflate block's first byte lies behind them and is not touched
  if (t < 10) file[33 + PNG_PLTE + t] = head[33 + t];
  // CRC-32 of IDAT's type, 78 01, the deflate block and the Adler-32: message byte j
  const long len = 6 + db + 4, cb = (len + T - 1) / T, j0 = t * cb, j1 = j0 + cb < len ? j0 + cb : len;
  if (j0 < j1) {
    unsigned c = 0xffffffffu;
    for (long j = j0; j < j1; ++j) {
      const unsigned byte = j < 6 ? head[37 + j] : j < 6 + db ? file[PNG_HEAD + j - 6] : (adler >> (8 * (3 - (int)(j - 6 - db)))) & 0xffu;
      c = table[(c ^ byte) & 0xffu] ^ (c >> 8);
    }
    c = png_crc_shift(c ^ 0xffffffffu, len - j1);
    if (c) atomicXor(&acc, c);
  }
  __syncthreads();
  if (t == 0) png_tail(file + PNG_HEAD + db, adler, acc);
}

// ------------------------------------------------------------------------------------------------------------------ render
constexpr int CELL = NPPC_SPEC_CELL, IMG = NPPC_SPEC_IMG;

// win [B][4]: t0, t1, marker 0, marker 1 (frames; -1: none).  mask [B][T]: 0 inside the gap.  The gap [s, e) is widened by its
// own length on each side and clamped; an item without a gap shows the whole clip
__global__ __launch_bounds__(T) void spec_windows_kernel(const float* __restrict__ mask, int B, int Tn, int* __restrict__ win) {
  __shared__ int lo, hi;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) lo = NONE, hi = -1;
  __syncthreads();
  int l = NONE, h = -1;
  for (int i = threadIdx.x; i < Tn; i += T)
    if (mask[(long)b * Tn + i] == 0.0f) l = l < i ? l : i, h = h > i ? h : i;
  if (h >= 0) atomicMin(&lo, l), atomicMax(&hi, h);
  __syncthreads();
  if (threadIdx.x == 0) {
    int* w = win + 4 * b;
    if (hi < 0) w[0] = 0, w[1] = Tn, w[2] = -1, w[3] = -1;
    else {
      const int s = lo, e = hi + 1, d = e - s;
      w[0] = s - d > 0 ? s - d : 0, w[1] = e + d < Tn ? e + d : Tn, w[2] = s, w[3] = e;
    }
  }
}

struct Planes {
  const float* x;
  int B, NP, CH, F, Tn;
};

__device__ bool window_of(const int* win, const Planes& pl, int b, int* t0, int* t1) {
  if (b < 0 || b >= pl.B) return false;
  *t0 = win[4 * b], *t1 = win[4 * b + 1];
  return *t0 >= 0 && *t1 > *t0 && *t1 <= pl.Tn;
}

// g(P + alpha Q) at (f, t) of item b.  Real planes: every operation is a separately rounded fp32 operation
__device__ float cell_value(const Planes& pl, const int* c, int b, int f, int t) {
#pragma clang fp contract(off)
  const int p = c[0], q = c[1], g = c[2];
  const float alpha = __int_as_float(c[4]);
  const long plane = (long)pl.F * pl.Tn, at = (long)f * pl.Tn + t;
  float v[2] = {0.0f, 0.0f};
  for (int ch = 0; ch < pl.CH; ++ch) {
    const float P = p >= 0 ? pl.x[(((long)b * pl.NP + p) * pl.CH + ch) * plane + at] : 0.0f;
    if (q >= 0) {
      const float prod = alpha * pl.x[(((long)b * pl.NP + q) * pl.CH + ch) * plane + at];
      v[ch] = p >= 0 ? P + prod : prod;
    } else {
      v[ch] = P;
    }
  }
  if (pl.CH == 1) return g == 1 ? fabsf(v[0]) : v[0];
  if (g == 0) return v[0];
  const float mag = sqrtf(v[0] * v[0] + v[1] * v[1]);
  return g == 1 ? mag : 20.0f * log10f(mag + 1e-8f);
}

__device__ bool cell_ok(const int* c, const Planes& pl) {
  return c[0] >= -1 && c[0] < pl.NP && c[1] >= -1 && c[1] < pl.NP && c[2] >= 0 && c[2] <= 2 && (c[2] < 2 || pl.CH == 2);
}

__device__ __forceinline__ int level(float v, float vmin, float scale) {
#pragma clang fp contract(off)
  const float d = v - vmin;
  const float x = floorf(d * scale);
  return !(x >= 0.0f) ? 0 : x > 253.0f ? 253 : (int)x;             // NaN: 0
}

// meta [nimg][4]: pixel offset (given), W, H (written here), the pixels the image may take (given).  An image that does not
// fit, or whose description cannot be, gets W = H = 0 and is left out by everything behind
__global__ __launch_bounds__(T) void spec_layout_kernel(const int* __restrict__ img, int nimg, const int* __restrict__ win, Planes pl,
                                                        int ncells, long* __restrict__ meta) {
  const int i = blockIdx.x * T + threadIdx.x;
  if (i >= nimg) return;
  const int* d = img + (long)IMG * i;
  const int R = d[1], C = d[2], first = d[3], sx = d[4], sy = d[5], gut = d[6];
  long W = 0, H = 0;
  int t0, t1;
  if (window_of(win, pl, d[0], &t0, &t1) && R >= 1 && C >= 1 && R <= 4096 && C <= 4096 && first >= 0 && (long)first + (long)R * C <= ncells &&
      sx >= 1 && sy >= 1 && sx <= 64 && sy <= 64 && gut >= 0 && gut <= 1024) {
    W = (long)C * (t1 - t0) * sx + (long)(C - 1) * gut;
    H = (long)R * pl.F * sy + (long)(R - 1) * gut;
    if (!png_dims_ok(W, H) || W * H > meta[4L * i + 3]) W = 0, H = 0;
  }
  meta[4L * i + 1] = W, meta[4L * i + 2] = H;
}

// rng [ncells][2]: vmin and scale of a cell: its own, or for an autoscaled cell from the finite values of its window
__global__ __launch_bounds__(T) void spec_autoscale_kernel(const int* __restrict__ img, int nimg, const int* __restrict__ cell, int ncells,
                                                           const int* __restrict__ win, Planes pl, float* __restrict__ rng) {
  __shared__ float mn[T], mx[T];
  const int ci = blockIdx.x, t = threadIdx.x;
  const int* c = cell + (long)CELL * ci;
  float vmin = __int_as_float(c[5]), scale = __int_as_float(c[6]);
  const int i = c[7];
  int t0, t1;
  const bool live = (c[3] & 1) && (c[0] >= 0 || c[1] >= 0) && cell_ok(c, pl) && i >= 0 && i < nimg &&
                    window_of(win, pl, img[(long)IMG * i], &t0, &t1);               // uniform
  if (live) {
    const int b = img[(long)IMG * i], w = t1 - t0;
    float lo = INFINITY, hi = -INFINITY;
    for (long e = t; e < (long)pl.F * w; e += T) {
      const float v = cell_value(pl, c, b, (int)(e / w), t0 + (int)(e % w));
      if (fabsf(v) < INFINITY) lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    mn[t] = lo, mx[t] = hi;
    __syncthreads();
    for (int d = T / 2; d; d >>= 1) {
      if (t < d) mn[t] = fminf(mn[t], mn[t + d]), mx[t] = fmaxf(mx[t], mx[t + d]);
      __syncthreads();
    }
    vmin = mn[0] <= mx[0] ? mn[0] : 0.0f;
    scale = mn[0] < mx[0] ? 254.0f / (mx[0] - mn[0]) : 0.0f;      // a constant panel: all zeros
  }
  if (t == 0) rng[2L * ci] = vmin, rng[2L * ci + 1] = scale;
}

__global__ __launch_bounds__(T) void spec_render_kernel(const int* __restrict__ img, int nimg, const int* __restrict__ cell,
                                                        const int* __restrict__ win, Planes pl, const float* __restrict__ rng,
                                                        const long* __restrict__ meta, unsigned char* __restrict__ pix, long pix_elems) {
  const int i = blockIdx.y;
  const long po = meta[4L * i], W = meta[4L * i + 1], H = meta[4L * i + 2];
  if (!png_dims_ok(W, H) || po < 0 || po > pix_elems - W * H) return;
  const int* d = img + (long)IMG * i;
  const int b = d[0], C = d[2], first = d[3], sx = d[4], sy = d[5], gut = d[6];
  int t0, t1;
  if (!window_of(win, pl, b, &t0, &t1)) return;
  const int m0 = win[4 * b + 2], m1 = win[4 * b + 3];
  const long cw = (long)(t1 - t0) * sx, ch = (long)pl.F * sy;
  for (long e = (long)blockIdx.x * T + threadIdx.x; e < W * H; e += (long)gridDim.x * T) {
    const long y = e / W, x = e - y * W;
    const long r = y / (ch + gut), yy = y - r * (ch + gut), cc = x / (cw + gut), xx = x - cc * (cw + gut);
    int v = 255;
    if (yy < ch && xx < cw) {
      const long ci = first + r * C + cc;
      const int* c = cell + CELL * ci;
      if ((c[0] >= 0 || c[1] >= 0) && cell_ok(c, pl)) {
        const int f = pl.F - 1 - (int)(yy / sy), t = t0 + (int)(xx / sx);
        if ((c[3] & 2) && (t == m0 || t == m1) && xx % sx == 0 && (yy / 4) % 2 == 0) v = 254;
        else v = level(cell_value(pl, c, b, f, t), rng[2 * ci], rng[2 * ci + 1]);
      }
    }
    pix[po + e] = (unsigned char)v;
  }
}

bool planes_ok(const float* x, int B, int NP, int CH, int F, int Tn) {
  return x && B >= 1 && NP >= 1 && (CH == 1 || CH == 2) && F >= 1 && Tn >= 1 && F <= PNG_MAX_DIM && Tn <= PNG_MAX_DIM && B <= 65535 &&
         NP <= 65535;
}

int encode_launch(const unsigned char* pix, long pix_elems, const long* meta, int nimg, const int* ttab, const int* tfirst, long ntiles,
                  const unsigned char* palette, int* plan, long* toff, long* stats, unsigned char* out, long out_cap, hipStream_t s) {
  Plte plte;
  png_plte(plte.b, palette);
  if (hipMemsetAsync(out, 0, (size_t)out_cap, s) != hipSuccess) return NPPC_ELAUNCH;
  hipLaunchKernelGGL(png_plan_kernel, dim3((unsigned)ntiles), dim3(T), 0, s, pix, pix_elems, meta, nimg, ttab, plan);
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(ST), 0, s, plan, tfirst, meta, nimg, ntiles, toff, stats);
  hipLaunchKernelGGL(png_write_kernel, dim3((unsigned)ntiles), dim3(T), 0, s, pix, pix_elems, meta, nimg, ttab, plan, toff, stats, out,
                     out_cap);
  hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)nimg), dim3(T), 0, s, meta, nimg, stats, plte, out, out_cap);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

bool encode_args_ok(const void* pix, long pix_elems, const void* meta, int nimg, const void* ttab, const void* tfirst, long ntiles,
                    const void* palette, const void* plan, const void* toff, const void* stats, const void* out, long out_cap) {
  return pix && meta && ttab && tfirst && palette && plan && toff && stats && out && pix_elems >= 1 && nimg >= 1 && nimg < (1 << 24) &&
         ntiles >= 1 && ntiles < (1L << 31) && out_cap >= 4 && ((uintptr_t)out & 3) == 0 && (out_cap & 3) == 0;     // whole words
}

int render_launch(const float* planes, int B, int NP, int CH, int F, int Tn, const int* img, int nimg, const int* cell, int ncells,
                  const int* win, float* rng, long* meta, unsigned char* pix, long pix_elems, long max_pixels, hipStream_t s) {
  const Planes pl{planes, B, NP, CH, F, Tn};
  hipLaunchKernelGGL(spec_layout_kernel, dim3((unsigned)((nimg + T - 1) / T)), dim3(T), 0, s, img, nimg, win, pl, ncells, meta);
  hipLaunchKernelGGL(spec_autoscale_kernel, dim3((unsigned)ncells), dim3(T), 0, s, img, nimg, cell, ncells, win, pl, rng);
  long bx = (max_pixels + 8L * T - 1) / (8L * T);
  bx = bx < 1 ? 1 : bx > 1024 ? 1024 : bx;
  hipLaunchKernelGGL(spec_render_kernel, dim3((unsigned)bx, (unsigned)nimg), dim3(T), 0, s, img, nimg, cell, win, pl, rng, meta, pix,
                     pix_elems);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

bool render_args_ok(const float* planes, int B, int NP, int CH, int F, int Tn, const void* img, int nimg, const void* cell, int ncells,
                    const void* win, const void* rng, const void* meta, const void* pix, long pix_elems, long max_pixels) {
  return planes_ok(planes, B, NP, CH, F, Tn) && img && cell && win && rng && meta && pix && nimg >= 1 && nimg <= 65535 && ncells >= 1 &&
         ncells < (1 << 24) && pix_elems >= 1 && max_pixels >= 1 && max_pixels <= PNG_MAX_PIXELS;
}

}  // namespace

extern "C" {

int nppc_png_bound(long W, long H, long* bytes) {
  if (!bytes || !png_dims_ok(W, H)) return NPPC_EBADARG;
  *bytes = png_bound(W, H);
  return NPPC_OK;
}

int nppc_png_encode_host(const unsigned char* idx, long W, long H, const unsigned char* palette, unsigned char* out, long cap,
                         long* nbytes) {
  if (!idx || !palette || !out || !nbytes || !png_dims_ok(W, H) || cap < png_bound(W, H)) return NPPC_EBADARG;
  *nbytes = png_encode_serial(idx, W, H, palette, out, cap);
  return NPPC_OK;
}

int nppc_png_encode(const unsigned char* pix, long pix_elems, const long* meta, int nimg, const int* ttab, const int* tfirst,
                    long ntiles, const unsigned char* palette, int* plan, long* toff, long* stats, unsigned char* out, long out_cap,
                    void* stream) {
  if (!encode_args_ok(pix, pix_elems, meta, nimg, ttab, tfirst, ntiles, palette, plan, toff, stats, out, out_cap)) return NPPC_EBADARG;
  return encode_launch(pix, pix_elems, meta, nimg, ttab, tfirst, ntiles, palette, plan, toff, stats, out, out_cap, (hipStream_t)stream);
}

int nppc_spec_windows(const float* mask, int B, int T_frames, int* win, void* stream) {
  if (!mask || !win || B < 1 || B > 65535 || T_frames < 1 || T_frames > PNG_MAX_DIM) return NPPC_EBADARG;
  hipLaunchKernelGGL(spec_windows_kernel, dim3((unsigned)B), dim3(T), 0, (hipStream_t)stream, mask, B, T_frames, win);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_spec_render(const float* planes, int B, int NP, int CH, int F, int T_frames, const int* img, int nimg, const int* cell,
                     int ncells, const int* win, float* rng, long* meta, unsigned char* pix, long pix_elems, long max_pixels,
                     void* stream) {
  if (!render_args_ok(planes, B, NP, CH, F, T_frames, img, nimg, cell, ncells, win, rng, meta, pix, pix_elems, max_pixels))
    return NPPC_EBADARG;
  return render_launch(planes, B, NP, CH, F, T_frames, img, nimg, cell, ncells, win, rng, meta, pix, pix_elems, max_pixels,
                       (hipStream_t)stream);
}

int nppc_spec_render_png(const float* planes, int B, int NP, int CH, int F, int T_frames, const int* img, int nimg, const int* cell,
                         int ncells, const int* win, float* rng, long* meta, unsigned char* pix, long pix_elems, long max_pixels,
                         const int* ttab, const int* tfirst, long ntiles, const unsigned char* palette, int* plan, long* toff,
                         long* stats, unsigned char* out, long out_cap, void* stream) {
  if (!render_args_ok(planes, B, NP, CH, F, T_frames, img, nimg, cell, ncells, win, rng, meta, pix, pix_elems, max_pixels) ||
      !encode_args_ok(pix, pix_elems, meta, nimg, ttab, tfirst, ntiles, palette, plan, toff, stats, out, out_cap))
    return NPPC_EBADARG;
  const int rc = render_launch(planes, B, NP, CH, F, T_frames, img, nimg, cell, ncells, win, rng, meta, pix, pix_elems, max_pixels,
                               (hipStream_t)stream);
  if (rc) return rc;
  return encode_launch(pix, pix_elems, meta, nimg, ttab, tfirst, ntiles, palette, plan, toff, stats, out, out_cap, (hipStream_t)stream);
}

}  // extern "C"
