// Curve sheets (pitch contours over frames, with axes box, grid, tick labels and legend) drawn as index images on gfx950
// and handed to the PNG encoder of csrc/spec_png.hip (nppc_audio/curve_png.py).  Every decision of the
// drawing is csrc/curve_core.h, shared with the serial host renderer below and with tools/check/curve_host_check.cc;
// specification tests/curve_ref.py.
//   nppc_curve_shape        host only: W, H and the margins of one sheet for a window of `frames` frames
//   nppc_curve_render_host  host only, serial
//   nppc_curve_render       layout (W, H of every image), autoscale (finite minimum and maximum of a panel), render
//   nppc_curve_render_png   nppc_curve_render then nppc_png_encode
// The render kernel is a gather: a workgroup belongs to one panel of one image, stages the quantised rows of that panel's
// curves over the frames t0 - 1 .. t1 in LDS (16 bits each, computed once per workgroup) and then walks the panel's pixels
// four at a time; a lane composes its four index bytes in a register and writes them with one 32-bit store (images start at
// multiples of four bytes; the last one to three pixels of an image go as bytes).  A plot pixel looks at the at most five
// columns its curves' widths can reach it from, a margin pixel at its panel's stamps.  No atomics, no workspace beyond the
// index images and the panels' ranges, no kernel waits for another workgroup: the pixels are a function of the inputs.
// LDS per workgroup: 32 KiB of rows (CURVE_LDS_ROWS) + the geometry, static.
#include <math.h>

#include "common.h"
#include "curve_core.h"
#include "nppc_hip.h"

namespace {

constexpr int TH = 256;
constexpr int CHUNKS = 8;                                         // workgroups per panel

__global__ __launch_bounds__(TH) void curve_layout_kernel(const float* __restrict__ values, CurveTabs tb, const int* __restrict__ win,
                                                          long* __restrict__ meta, long pix_elems) {
  const int i = blockIdx.x * TH + threadIdx.x;
  if (i >= tb.nimg) return;
  CurveGeo G;
  int t0, t1;
  long W = 0, H = 0;
  const long po = meta[4L * i];
  if (curve_window(win, tb, tb.sheet[(long)CURVE_SHEET * i], &t0, &t1) && curve_geo(tb, i, t1 - t0, &G) && G.W * G.H <= meta[4L * i + 3] &&
      po >= 0 && (po & 3) == 0 && po <= pix_elems - G.W * G.H)
    W = G.W, H = G.H;
  meta[4L * i + 1] = W, meta[4L * i + 2] = H;
}

// rng [npanels][2]: ymin and scale of a panel: its own, or for an autoscaled panel from the finite values of its curves inside
// the window.  One workgroup per (image, panel); fminf and fmaxf of finite values do not depend on the order
__global__ __launch_bounds__(TH) void curve_autoscale_kernel(const float* __restrict__ values, CurveTabs tb, const int* __restrict__ win,
                                                             const long* __restrict__ meta, float* __restrict__ rng) {
  __shared__ float mn[TH], mx[TH];
  const int i = blockIdx.y, p = blockIdx.x, t = threadIdx.x;
  if (meta[4L * i + 1] < 1) return;                                // the layout kernel checked everything below
  const int* sh = tb.sheet + (long)CURVE_SHEET * i;
  if (p >= sh[2]) return;
  const int* pn = tb.panel + (long)CURVE_PANEL * (sh[1] + p);
  const int t0 = win[4 * sh[0]], frames = win[4 * sh[0] + 1] - t0;
  float ymin = curve_bits(pn[3]), scale = curve_bits(pn[4]);
  if (pn[2] & 1) {                                                 // uniform
    float lo = INFINITY, hi = -INFINITY;
    for (long e = t; e < (long)pn[1] * frames; e += TH) {
      const int row = tb.curve[(long)CURVE_CURVE * (pn[0] + (int)(e / frames))];
      const float v = values[(long)row * tb.T + t0 + (int)(e % frames)];
      if (fabsf(v) < INFINITY) lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    mn[t] = lo, mx[t] = hi;
    __syncthreads();
    for (int d = TH / 2; d; d >>= 1) {
      if (t < d) mn[t] = fminf(mn[t], mn[t + d]), mx[t] = fmaxf(mx[t], mx[t + d]);
      __syncthreads();
    }
    curve_range(mn[0], mx[0], sh[4], &ymin, &scale);
  }
  if (t == 0) rng[2L * (sh[1] + p)] = ymin, rng[2L * (sh[1] + p) + 1] = scale;
}

__global__ __launch_bounds__(TH) void curve_render_kernel(const float* __restrict__ values, CurveTabs tb, const int* __restrict__ win,
                                                          const float* __restrict__ rng, const long* __restrict__ meta,
                                                          unsigned char* __restrict__ pix, long pix_elems) {
  __shared__ short rows[CURVE_LDS_ROWS];
  __shared__ CurveGeo Gs;
  __shared__ int tops[2];                                          // the panel's first row and its height
  const int i = blockIdx.y, p = blockIdx.x / CHUNKS, chunk = blockIdx.x % CHUNKS, t = threadIdx.x;
  const long po = meta[4L * i], W = meta[4L * i + 1], H = meta[4L * i + 2];
  if (!png_dims_ok(W, H) || po < 0 || (po & 3) || po > pix_elems - W * H) return;
  const int item = tb.sheet[(long)CURVE_SHEET * i];
  if (p >= tb.sheet[(long)CURVE_SHEET * i + 2]) return;
  const int t0 = win[4 * item], frames = win[4 * item + 1] - t0;
  if (t == 0) {
    CurveGeo G;
    const bool ok = curve_geo(tb, i, frames, &G) && G.W == W && G.H == H;      // as the layout kernel found it
    int top = 0;
    for (int q = 0; ok && q < p; ++q) top += curve_panel_height(tb, G, q);
    Gs = G;
    tops[0] = ok ? top : -1, tops[1] = ok ? curve_panel_height(tb, G, p) : 0;
  }
  __syncthreads();
  const int top = tops[0], hp = tops[1];
  if (top < 0) return;
  const CurveGeo G = Gs;
  const int* pn = tb.panel + (long)CURVE_PANEL * (G.p0 + p);
  const float ymin = rng[2 * (G.p0 + p)], scale = rng[2 * (G.p0 + p) + 1];
  const int staged = pn[1] * (frames + 2);                         // at most CURVE_LDS_ROWS (curve_geo)
  for (int e = t; e < staged; e += TH) rows[e] = curve_stage(values, tb, pn, t0, frames, ymin, scale, G.PH, e);
  __syncthreads();
  // the quads whose first pixel lies in this panel's rows
  const long n = W * H, q0 = ((long)top * W + 3) / 4, q1 = p + 1 == G.np ? (n + 3) / 4 : ((long)(top + hp) * W + 3) / 4;
  for (long q = q0 + (long)chunk * TH + t; q < q1; q += (long)CHUNKS * TH) {
    unsigned word = 0;
    const long e0 = 4 * q;
    const int cnt = n - e0 < 4 ? (int)(n - e0) : 4;
    long y = (long)((unsigned)e0 / (unsigned)W), x = e0 - y * W;   // W H <= 2^26: one 32-bit division per quad
    for (int k = 0; k < cnt; ++k, ++x) {
      if (x == W) x = 0, ++y;
      int v;
      if (y < top + hp) v = curve_pixel(tb, G, p, top, win, rng, rows, x, y);
      else {                                                       // the first row of the next panel: margin, never plot area
        int ntop;
        const int np_ = curve_panel_at(tb, G, y, &ntop);
        v = np_ < 0 ? CURVE_BACKGROUND : curve_pixel(tb, G, np_, ntop, win, rng, nullptr, x, y);
      }
      word |= (unsigned)(v & 0xff) << (8 * k);
    }
    if (cnt == 4) *reinterpret_cast<unsigned*>(pix + po + e0) = word;
    else
      for (int k = 0; k < cnt; ++k) pix[po + e0 + k] = (unsigned char)(word >> (8 * k));
  }
}

bool tabs_ok(const float* values, int N, int T, const int* sheet, int nimg, const int* panel, int npanels, const int* curve, int ncurves,
             const int* stamp, int nstamps, const int* win, int nitems) {
  return values && sheet && panel && curve && win && (stamp || nstamps == 0) && N >= 1 && N < (1 << 24) && T >= 1 && T <= PNG_MAX_DIM &&
         nimg >= 1 && nimg <= 65535 && npanels >= 1 && npanels < (1 << 20) && ncurves >= 0 && ncurves < (1 << 24) && nstamps >= 0 &&
         nstamps < (1 << 24) && nitems >= 1 && nitems < (1 << 24);
}

CurveTabs tabs(int N, int T, const int* sheet, int nimg, const int* panel, int npanels, const int* curve, int ncurves, const int* stamp,
               int nstamps, int nitems) {
  return CurveTabs{sheet, panel, curve, stamp, nimg, npanels, ncurves, nstamps, N, T, nitems};
}

int render_launch(const float* values, const CurveTabs& tb, const int* win, int max_panels, float* rng, long* meta, unsigned char* pix,
                  long pix_elems, hipStream_t s) {
  hipLaunchKernelGGL(curve_layout_kernel, dim3((unsigned)((tb.nimg + TH - 1) / TH)), dim3(TH), 0, s, values, tb, win, meta, pix_elems);
  hipLaunchKernelGGL(curve_autoscale_kernel, dim3((unsigned)max_panels, (unsigned)tb.nimg), dim3(TH), 0, s, values, tb, win, meta, rng);
  hipLaunchKernelGGL(curve_render_kernel, dim3((unsigned)(max_panels * CHUNKS), (unsigned)tb.nimg), dim3(TH), 0, s, values, tb, win, rng,
                     meta, pix, pix_elems);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

bool render_args_ok(int max_panels, const void* rng, const void* meta, const void* pix, long pix_elems) {
  return rng && meta && pix && pix_elems >= 1 && max_panels >= 1 && max_panels <= CURVE_MAX_PANELS && ((uintptr_t)pix & 3) == 0;
}

}  // namespace

extern "C" {

int nppc_curve_shape(const int* sheet, int nimg, const int* panel, int npanels, const int* curve, int ncurves, const int* stamp,
                     int nstamps, int N, int T_frames, int i, int frames, long* W, long* H, int* margins) {
  if (!sheet || !panel || !curve || (!stamp && nstamps) || !W || !H || nimg < 1 || npanels < 1 || ncurves < 0 || nstamps < 0 || N < 1 ||
      T_frames < 1 || T_frames > PNG_MAX_DIM)
    return NPPC_EBADARG;
  const CurveTabs tb = tabs(N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, 1 << 24);
  CurveGeo G;
  if (!curve_geo(tb, i, frames, &G)) return NPPC_EBADARG;
  *W = G.W, *H = G.H;
  if (margins) margins[0] = G.ML, margins[1] = G.MR, margins[2] = G.PW, margins[3] = G.maxc;
  return NPPC_OK;
}

int nppc_curve_render_host(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                           const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, float* rng,
                           long* meta, unsigned char* pix, long pix_elems) {
  if (!tabs_ok(values, N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, win, nitems) || !rng || !meta || !pix ||
      pix_elems < 1)
    return NPPC_EBADARG;
  curve_render_serial(values, tabs(N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, nitems), win, rng, meta, pix,
                      pix_elems);
  return NPPC_OK;
}

int nppc_curve_render(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                      const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, int max_panels,
                      float* rng, long* meta, unsigned char* pix, long pix_elems, void* stream) {
  if (!tabs_ok(values, N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, win, nitems) ||
      !render_args_ok(max_panels, rng, meta, pix, pix_elems))
    return NPPC_EBADARG;
  return render_launch(values, tabs(N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, nitems), win, max_panels, rng,
                       meta, pix, pix_elems, (hipStream_t)stream);
}

int nppc_curve_render_png(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                          const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, int max_panels,
                          float* rng, long* meta, unsigned char* pix, long pix_elems, const int* ttab, const int* tfirst, long ntiles,
                          const unsigned char* palette, int* plan, long* toff, long* stats, unsigned char* out, long out_cap,
                          void* stream) {
  if (!tabs_ok(values, N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, win, nitems) ||
      !render_args_ok(max_panels, rng, meta, pix, pix_elems) || !ttab || !tfirst || !palette || !plan || !toff || !stats || !out ||
      ntiles < 1 || out_cap < 4 || ((uintptr_t)out & 3) || (out_cap & 3))
    return NPPC_EBADARG;
  const int rc = render_launch(values, tabs(N, T_frames, sheet, nimg, panel, npanels, curve, ncurves, stamp, nstamps, nitems), win,
                               max_panels, rng, meta, pix, pix_elems, (hipStream_t)stream);
  if (rc) return rc;
  return nppc_png_encode(pix, pix_elems, meta, nimg, ttab, tfirst, ntiles, palette, plan, toff, stats, out, out_cap, stream);
}

}  // extern "C"
