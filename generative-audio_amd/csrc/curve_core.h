// Curve-sheet core (specification tests/curve_ref.py): plain C++ that compiles as __host__ __device__
// under hipcc and as ordinary inline functions under any host compiler, so the serial host renderer, the device kernels
// (csrc/curve_png.hip) and the sanitizer program (tools/check/curve_host_check.cc) take every decision with the same text.
//
// A sheet stacks panels over the frames [t0, t1) of one item's window; a panel draws curves (rows of values [N][T], NaN: no
// point at that frame) into a plot area of PW = (t1 - t0) sx by PH pixels.  Everything below is integer arithmetic on the
// tables, the window and the quantised rows; the only floating point is the quantisation itself.
//
// Quantisation.  row(v) = floor((v - ymin) * scale), subtraction, product and floor each rounded to fp32 on its own (no
//   contraction); NaN and negatives (-inf too) give row 0 of a POINT THAT EXISTS only if v is not NaN: a NaN v is no point,
//   every other v is clamped to [0, PH - 1].  Row 0 is the bottom pixel row.  scale = fp32(PH / (ymax - ymin)) from the host;
//   an autoscaled panel takes mn, mx from the finite values of its curves inside the window: ymin = mn,
//   scale = fp32(PH) / (mx - mn); mn == mx: ymin = mn - 0.5, scale = fp32(PH) (a range of one, the value in the middle);
//   no finite value: ymin = 0, scale = fp32(PH).  A frame outside the clip [0, T) holds no point.
// Columns.  Frame t owns plot columns [(t - t0) sx, (t - t0 + 1) sx); its point sits in column c(t) = (t - t0) sx + sx / 2.
// Core pixels of a curve, for plot columns 0 <= x < PW only (the sheet is the crop of the whole curve; the half-segments
//   from t0 - 1 and to t1 are drawn where they fall inside): u = x - sx / 2, t = t0 + floor(u / sx), j = u mod sx in [0, sx).
//   With points at t and t + 1 (rows ra, rb): R(j) = ra + floor((rb - ra) j / sx) (floor division), a = R(j), b = R(j + 1);
//   the column lights rows a .. b - 1 (b > a), b + 1 .. a (b < a) or a (b == a): from its own row towards, and short of, the
//   next column's, so a jump is one connected vertical run.  With a point at t only, column c(t) (j == 0) lights ra: the
//   end of a segment, or a dot.
// Width w in 1..5 lights, for every core pixel (x, r), the pixels (x + dx, r + dy), dx and dy in -(w - 1) / 2 .. w / 2
//   (integer division: an even width grows towards higher columns and higher rows), clipped to the plot area.
// Paint order of a plot pixel, last wins: background 255; grid 251 (the row of every y tick; the centre column of every
//   frame t with t mod xtick_every == 0); markers 254 (centre column of frames marker0 and marker1, pixel rows py from the top
//   with (py / 4) mod 2 == 0); the curves in table order.
// A y tick of value v has x = floor((v - ymin) * scale) as above and is drawn when 0 <= x <= PH, at row min(x, PH - 1).
//
// Layout, g = glyph scale: a glyph cell is 6g x 7g (5 x 7 dots and one blank column).  ML = 6g maxY + 2g (maxY: the longest
//   y label of the sheet; 0: ML = 0); MR = 11g + 6g maxL when any panel has a legend (maxL: its longest text), else 0.
//   W = ML + PW + 2 + MR.  Panel height Hp = 4g + PH + 2 + (9g with an x label, else 4g); H is their sum.  The axes box
//   (250) is the rectangle [ML, ML + PW + 1] x [top + 4g, top + 4g + PH + 1]; the plot area lies inside it.
//   y label: right-aligned, x from ML - g - 6g n, y from (pixel row of the tick) - 3g.
//   x label of frame t (t0 <= t < t1): x from ML + 1 + c(t) - (6g n - g) / 2, y from box bottom + 1 + g.
//   legend entry i: swatch [xs, xs + 7g) x [ys, ys + 7g), xs = box right + 1 + 2g, ys = box top + g + 8g i; text from xs + 8g.
//   A stamp is clipped to its own panel's band of rows and to the image; later stamps paint over earlier ones.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "png_core.h"

#define CURVE_SHEET 8          // ints: item, first panel, panels, sx, plot height PH, glyph scale g, 0, 0
#define CURVE_PANEL 8          // ints: first curve, curves, flags (1 autoscale, 2 markers), ymin, scale (floats' bits), first stamp,
                               //       stamps, xtick_every (0: no vertical grid)
#define CURVE_CURVE 4          // ints: row of values, colour, width, 0
#define CURVE_STAMP 8          // ints: kind (0 y tick, 1 x label, 2 legend entry), value (float's bits / frame / entry number),
                               //       colour (legend swatch), characters n, glyph codes 4 bits each (two ints), 0, 0
#define CURVE_MAX_PANELS 64
#define CURVE_MAX_CHARS 16
#define CURVE_MAX_WIDTH 5
#define CURVE_MAX_SX 64
#define CURVE_MAX_GLYPH_SCALE 8
#define CURVE_GLYPHS 13        // 0-9 . - space
#define CURVE_LDS_ROWS 16384   // 16-bit rows a workgroup stages: curves of a panel x (window + 2) may not be more
#define CURVE_INK 250
#define CURVE_GRID 251
#define CURVE_MARKER 254
#define CURVE_BACKGROUND 255

// the 5 x 7 font: 7 rows per glyph, bit 4 the leftmost dot
PNG_HD unsigned curve_font_row(int glyph, int row) {
  constexpr unsigned char F[CURVE_GLYPHS * 7] = {
      0x0e, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0e,   // 0
      0x04, 0x0c, 0x04, 0x04, 0x04, 0x04, 0x0e,   // 1
      0x0e, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1f,   // 2
      0x1e, 0x01, 0x01, 0x0e, 0x01, 0x01, 0x1e,   // 3
      0x02, 0x06, 0x0a, 0x12, 0x1f, 0x02, 0x02,   // 4
      0x1f, 0x10, 0x1e, 0x01, 0x01, 0x11, 0x0e,   // 5
      0x06, 0x08, 0x10, 0x1e, 0x11, 0x11, 0x0e,   // 6
      0x1f, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08,   // 7
      0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e,   // 8
      0x0e, 0x11, 0x11, 0x0f, 0x01, 0x02, 0x0c,   // 9
      0x00, 0x00, 0x00, 0x00, 0x00, 0x0c, 0x0c,   // .
      0x00, 0x00, 0x00, 0x1f, 0x00, 0x00, 0x00,   // -
      0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};  // space
  return F[glyph * 7 + row];
}

struct CurveTabs {
  const int *sheet, *panel, *curve, *stamp;
  int nimg, npanels, ncurves, nstamps;
  int N, T, nitems;                                                // values [N][T], win [nitems][4]
};

struct CurveGeo {
  int item, p0, np, sx, PH, g, PW, ML, MR, maxc;                   // maxc: the most curves of a panel
  long W, H;
  unsigned long long magic;                                        // curve_magic(sx)
};

PNG_HD float curve_bits(int b) {
  union {
    int i;
    float f;
  } u;
  u.i = b;
  return u.f;
}

// floor(a / sx) without a division: for 0 <= n < 2^26 and sx in 1..64, n / sx == (n * (2^32 / sx + 1)) >> 32 exactly (the
// product's excess over n / sx is at most n / 2^32 < 1 / 64 <= 1 / sx, less than the distance of n / sx to the next integer)
PNG_HD unsigned long long curve_magic(int sx) { return (1ull << 32) / (unsigned)sx + 1ull; }
PNG_HD int curve_floordiv(int a, int sx, unsigned long long magic) {          // |a| < 2^26 - 64
  if (a >= 0) return (int)(((unsigned long long)a * magic) >> 32);
  return -(int)(((unsigned long long)(-a + sx - 1) * magic) >> 32);           // floor(a / sx) = -ceil(-a / sx)
}

// floor((v - ymin) * scale) as a float; every operation rounded on its own
PNG_HD float curve_pos(float v, float ymin, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = v - ymin;
  const float x = d * scale;
  return floorf(x);
}
// the row of a value, -1 for NaN
PNG_HD int curve_row(float v, float ymin, float scale, int PH) {
  if (v != v) return -1;
  const float x = curve_pos(v, ymin, scale);
  return !(x >= 0.0f) ? 0 : x > (float)(PH - 1) ? PH - 1 : (int)x;
}
PNG_HD int curve_tick_row(float v, float ymin, float scale, int PH) {
  const float x = curve_pos(v, ymin, scale);
  if (!(x >= 0.0f) || !(x <= (float)PH)) return -1;
  return x > (float)(PH - 1) ? PH - 1 : (int)x;
}

PNG_HD void curve_range(float mn, float mx, int PH, float* ymin, float* scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(mn <= mx)) *ymin = 0.0f, *scale = (float)PH;
  else if (mn == mx) *ymin = mn - 0.5f, *scale = (float)PH;
  else {
    const float d = mx - mn;
    *ymin = mn, *scale = (float)PH / d;
  }
}

PNG_HD bool curve_panel_has_xlabel(const CurveTabs& tb, const int* pn) {
  for (int s = 0; s < pn[6]; ++s) {
    const int* st = tb.stamp + (long)CURVE_STAMP * (pn[5] + s);
    if (st[0] == 1 && st[3] > 0) return true;
  }
  return false;
}
PNG_HD int curve_panel_height(const CurveTabs& tb, const CurveGeo& G, int p) {
  return 4 * G.g + G.PH + 2 + (curve_panel_has_xlabel(tb, tb.panel + (long)CURVE_PANEL * (G.p0 + p)) ? 9 * G.g : 4 * G.g);
}

// Everything sheet i's drawing will index is checked here; false: the sheet cannot be drawn.  frames = t1 - t0
PNG_HD bool curve_geo(const CurveTabs& tb, int i, int frames, CurveGeo* G) {
  if (i < 0 || i >= tb.nimg) return false;
  const int* sh = tb.sheet + (long)CURVE_SHEET * i;
  G->item = sh[0], G->p0 = sh[1], G->np = sh[2], G->sx = sh[3], G->PH = sh[4], G->g = sh[5];
  if (G->item < 0 || G->item >= tb.nitems || G->np < 1 || G->np > CURVE_MAX_PANELS || G->p0 < 0 || G->p0 > tb.npanels - G->np ||
      G->sx < 1 || G->sx > CURVE_MAX_SX || G->PH < 1 || G->PH > PNG_MAX_DIM || G->g < 1 || G->g > CURVE_MAX_GLYPH_SCALE || frames < 1 ||
      frames > PNG_MAX_DIM || frames > tb.T)
    return false;
  int maxY = 0, maxL = 0, legend = 0;
  long H = 0;
  G->maxc = 0;
  for (int p = 0; p < G->np; ++p) {
    const int* pn = tb.panel + (long)CURVE_PANEL * (G->p0 + p);
    if (pn[0] < 0 || pn[1] < 0 || pn[1] > tb.ncurves || pn[0] > tb.ncurves - pn[1] || pn[5] < 0 || pn[6] < 0 || pn[6] > tb.nstamps ||
        pn[5] > tb.nstamps - pn[6] || pn[7] < 0)
      return false;
    if ((long)pn[1] * (frames + 2) > CURVE_LDS_ROWS) return false;
    G->maxc = pn[1] > G->maxc ? pn[1] : G->maxc;
    for (int c = 0; c < pn[1]; ++c) {
      const int* cv = tb.curve + (long)CURVE_CURVE * (pn[0] + c);
      if (cv[0] < 0 || cv[0] >= tb.N || cv[1] < 0 || cv[1] > 255 || cv[2] < 1 || cv[2] > CURVE_MAX_WIDTH) return false;
    }
    for (int s = 0; s < pn[6]; ++s) {
      const int* st = tb.stamp + (long)CURVE_STAMP * (pn[5] + s);
      if (st[0] < 0 || st[0] > 2 || st[3] < 0 || st[3] > CURVE_MAX_CHARS || st[2] < 0 || st[2] > 255) return false;
      for (int k = 0; k < st[3]; ++k)
        if (((st[4 + k / 8] >> (4 * (k % 8))) & 15) >= CURVE_GLYPHS) return false;
      if (st[0] == 2 && (st[1] < 0 || st[1] > PNG_MAX_DIM)) return false;
      if (st[0] == 0 && st[3] > maxY) maxY = st[3];
      if (st[0] == 2) legend = 1, maxL = st[3] > maxL ? st[3] : maxL;
    }
    H += 4 * G->g + G->PH + 2 + (curve_panel_has_xlabel(tb, pn) ? 9 * G->g : 4 * G->g);
  }
  G->PW = frames * G->sx;
  G->magic = curve_magic(G->sx);
  G->ML = maxY ? 6 * G->g * maxY + 2 * G->g : 0;
  G->MR = legend ? 11 * G->g + 6 * G->g * maxL : 0;
  G->W = (long)G->ML + G->PW + 2 + G->MR, G->H = H;
  return png_dims_ok(G->W, G->H);
}

// the window of an item, checked against the clip
PNG_HD bool curve_window(const int* win, const CurveTabs& tb, int item, int* t0, int* t1) {
  if (item < 0 || item >= tb.nitems) return false;
  *t0 = win[4 * item], *t1 = win[4 * item + 1];
  return *t0 >= 0 && *t1 > *t0 && *t1 <= tb.T;
}

// the panel of image row y and its first row
PNG_HD int curve_panel_at(const CurveTabs& tb, const CurveGeo& G, long y, int* top) {
  int at = 0;
  for (int p = 0; p < G.np; ++p) {
    const int hp = curve_panel_height(tb, G, p);
    if (y < at + hp) return *top = at, p;
    at += hp;
  }
  return -1;
}

// rows [curves][frames + 2] of panel pn: frames t0 - 1 .. t1, entry e
PNG_HD short curve_stage(const float* values, const CurveTabs& tb, const int* pn, int t0, int frames, float ymin, float scale, int PH,
                         int e) {
  const int k = e / (frames + 2), t = t0 - 1 + e % (frames + 2);
  if (t < 0 || t >= tb.T) return -1;
  const int* cv = tb.curve + (long)CURVE_CURVE * (pn[0] + k);
  return (short)curve_row(values[(long)cv[0] * tb.T + t], ymin, scale, PH);
}

// a pixel of the plot area: px in [0, PW), py in [0, PH) from the top
PNG_HD int curve_plot_pixel(const CurveTabs& tb, const CurveGeo& G, const int* pn, int t0, int frames, int m0, int m1, float ymin,
                            float scale, const short* rows, int px, int py) {
  const int r = G.PH - 1 - py, sx = G.sx, half = sx / 2;
  for (int k = pn[1] - 1; k >= 0; --k) {
    const int* cv = tb.curve + (long)CURVE_CURVE * (pn[0] + k);
    const int w = cv[2], lo = (w - 1) / 2, hi = w / 2;
    const short* rw = rows + (long)k * (frames + 2);
    const int x0 = px - hi < 0 ? 0 : px - hi, x1 = px + lo > G.PW - 1 ? G.PW - 1 : px + lo;
    for (int x = x0; x <= x1; ++x) {
      const int u = x - half, tr = curve_floordiv(u, sx, G.magic), j = u - tr * sx;       // tr in [-1, frames - 1]
      const int ra = rw[tr + 1], rb = rw[tr + 2];
      int a, b;
      if (ra >= 0 && rb >= 0) {
        const int d = rb - ra, Ra = ra + curve_floordiv(d * j, sx, G.magic), Rb = ra + curve_floordiv(d * (j + 1), sx, G.magic);
        if (Rb > Ra) a = Ra, b = Rb - 1;
        else if (Rb < Ra) a = Rb + 1, b = Ra;
        else a = b = Ra;
      } else if (j == 0 && ra >= 0) {
        a = b = ra;
      } else {
        continue;
      }
      if (a <= r + lo && b >= r - hi) return cv[1];
    }
  }
  const int u = px - half;
  const bool centre = u >= 0 && u % sx == 0;
  const int t = t0 + (u >= 0 ? u / sx : 0);
  if ((pn[2] & 2) && centre && (t == m0 || t == m1) && (py / 4) % 2 == 0) return CURVE_MARKER;
  if (pn[7] > 0 && centre && t % pn[7] == 0) return CURVE_GRID;
  for (int s = 0; s < pn[6]; ++s) {
    const int* st = tb.stamp + (long)CURVE_STAMP * (pn[5] + s);
    if (st[0] == 0 && curve_tick_row(curve_bits(st[1]), ymin, scale, G.PH) == r) return CURVE_GRID;
  }
  return CURVE_BACKGROUND;
}

PNG_HD bool curve_text_hit(const int* st, int g, long dx, long dy) {
  if (dx < 0 || dy < 0 || dy >= 7 * g || dx >= (long)6 * g * st[3]) return false;
  const int ci = (int)(dx / (6 * g)), gx = (int)(dx % (6 * g)) / g, gy = (int)dy / g;
  if (gx > 4) return false;
  const int code = (st[4 + ci / 8] >> (4 * (ci % 8))) & 15;
  return (curve_font_row(code, gy) >> (4 - gx)) & 1u;
}

// a pixel of panel p (first row `top`) outside its plot area: x, y in image coordinates
PNG_HD int curve_margin_pixel(const CurveTabs& tb, const CurveGeo& G, const int* pn, int top, int t0, int t1, float ymin, float scale,
                              long x, long y) {
  const int g = G.g;
  const long bx0 = G.ML, bx1 = G.ML + G.PW + 1, by0 = top + 4 * g, by1 = by0 + G.PH + 1;
  if (x >= bx0 && x <= bx1 && y >= by0 && y <= by1 && (x == bx0 || x == bx1 || y == by0 || y == by1)) return CURVE_INK;
  int v = CURVE_BACKGROUND;
  for (int s = 0; s < pn[6]; ++s) {
    const int* st = tb.stamp + (long)CURVE_STAMP * (pn[5] + s);
    const int n = st[3];
    if (st[0] == 0) {
      const int row = curve_tick_row(curve_bits(st[1]), ymin, scale, G.PH);
      if (row < 0) continue;
      if (curve_text_hit(st, g, x - (G.ML - g - (long)6 * g * n), y - (by0 + 1 + (G.PH - 1 - row) - 3 * g))) v = CURVE_INK;
    } else if (st[0] == 1) {
      const int t = st[1];
      if (t < t0 || t >= t1) continue;
      const long cx = G.ML + 1 + (long)(t - t0) * G.sx + G.sx / 2;
      if (curve_text_hit(st, g, x - (cx - (6 * g * n - g) / 2), y - (by1 + 1 + g))) v = CURVE_INK;
    } else {
      const long xs = bx1 + 1 + 2 * g, ys = by0 + g + (long)8 * g * st[1];
      if (x >= xs && x < xs + 7 * g && y >= ys && y < ys + 7 * g) v = st[2];
      else if (curve_text_hit(st, g, x - (xs + 8 * g), y - ys)) v = CURVE_INK;
    }
  }
  return v;
}

// pixel (x, y) of a sheet whose panel `p` (first row top) holds row y; rows: that panel's staged rows, or null for a pixel
// that cannot lie in a plot area
PNG_HD int curve_pixel(const CurveTabs& tb, const CurveGeo& G, int p, int top, const int* win, const float* rng, const short* rows, long x,
                       long y) {
  const int* pn = tb.panel + (long)CURVE_PANEL * (G.p0 + p);
  const int t0 = win[4 * G.item], t1 = win[4 * G.item + 1];
  const float ymin = rng[2 * (G.p0 + p)], scale = rng[2 * (G.p0 + p) + 1];
  const long px = x - G.ML - 1, py = y - top - 4 * G.g - 1;
  if (rows && px >= 0 && px < G.PW && py >= 0 && py < G.PH)
    return curve_plot_pixel(tb, G, pn, t0, t1 - t0, win[4 * G.item + 2], win[4 * G.item + 3], ymin, scale, rows, (int)px, (int)py);
  return curve_margin_pixel(tb, G, pn, top, t0, t1, ymin, scale, x, y);
}

// ymin and scale of panel pn of a sheet with window [t0, t1): its own, or from the finite values (serial form)
inline void curve_autoscale_serial(const float* values, const CurveTabs& tb, const int* pn, int t0, int t1, int PH, float* ymin,
                                   float* scale) {
  *ymin = curve_bits(pn[3]), *scale = curve_bits(pn[4]);
  if (!(pn[2] & 1)) return;
  float mn = INFINITY, mx = -INFINITY;
  for (int c = 0; c < pn[1]; ++c)
    for (int t = t0; t < t1; ++t) {
      const float v = values[(long)tb.curve[(long)CURVE_CURVE * (pn[0] + c)] * tb.T + t];
      if (fabsf(v) < INFINITY) mn = fminf(mn, v), mx = fmaxf(mx, v);
    }
  curve_range(mn, mx, PH, ymin, scale);
}

// The serial renderer.  meta [nimg][4]: first pixel (given), W, H (written), pixels allowed (given); a sheet that cannot be
// drawn or needs more pixels than allowed gets W = H = 0.  rng [npanels][2] is written.  All tables are host memory.
inline void curve_render_serial(const float* values, const CurveTabs& tb, const int* win, float* rng, long* meta, unsigned char* pix,
                                long pix_elems) {
  for (int i = 0; i < tb.nimg; ++i) {
    CurveGeo G;
    int t0 = 0, t1 = 0;
    long* m = meta + 4L * i;
    m[1] = m[2] = 0;
    const int item = tb.sheet[(long)CURVE_SHEET * i];
    if (!curve_window(win, tb, item, &t0, &t1) || !curve_geo(tb, i, t1 - t0, &G)) continue;
    if (G.W * G.H > m[3] || m[0] < 0 || m[0] > pix_elems - G.W * G.H) continue;
    m[1] = G.W, m[2] = G.H;
    const int frames = t1 - t0;
    short* rows = (short*)malloc(sizeof(short) * (size_t)(G.maxc > 0 ? G.maxc : 1) * (size_t)(frames + 2));
    int top = 0;
    for (int p = 0; p < G.np; ++p) {
      const int* pn = tb.panel + (long)CURVE_PANEL * (G.p0 + p);
      float* r = rng + 2L * (G.p0 + p);
      curve_autoscale_serial(values, tb, pn, t0, t1, G.PH, r, r + 1);
      for (int e = 0; e < pn[1] * (frames + 2); ++e) rows[e] = curve_stage(values, tb, pn, t0, frames, r[0], r[1], G.PH, e);
      const int hp = curve_panel_height(tb, G, p);
      for (long y = top; y < top + hp; ++y)
        for (long x = 0; x < G.W; ++x) pix[m[0] + y * G.W + x] = (unsigned char)curve_pixel(tb, G, p, top, win, rng, rows, x, y);
      top += hp;
    }
    free(rows);
  }
}
