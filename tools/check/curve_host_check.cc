// Sanitizer program of the curve-sheet core (csrc/curve_core.h).  Stand-alone, CPU only:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igenerative-audio_amd/csrc \
//       tools/check/curve_host_check.cc -o curve_host_check && ./curve_host_check
//
// Every table, the values, the windows and every index image live in heap blocks of exactly their size, so a read or a write
// one element outside any of them is an AddressSanitizer report.  Generated cases: T in {1, 2, 3, 12, 40}, sx in {1, 2, 3, 8},
// plot heights 7 and 64, glyph scales 1 and 2, one to three panels of zero to four curves of every width, values with NaN,
// infinities and values on and outside the range, autoscaled panels, random windows and markers, ticks, labels of random
// glyphs, legends.  The serial renderer (curve_render_serial, which walks the same per-pixel functions the device kernel
// walks) is compared pixel for pixel with a straightforward implementation of the rule in this file that PAINTS: background,
// stamps, box, grid, markers, then every curve's core pixels grown by its width.  Then the refusals: tables the layout must
// not accept (a width of 6, a colour of 256, 65 panels, curves x (window + 2) beyond the cap, an item or a window outside the
// data, a glyph code of 13, too few pixels allowed) leave W = H = 0 and every pixel untouched.  Exit status 0 and a line of counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "curve_core.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                                  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
int pick(int n) { return (int)(rnd() % (uint32_t)n); }

[[noreturn]] void fail(const char* what, long a = 0, long b = 0, long c = 0) {
  fprintf(stderr, "curve_host_check: %s (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}

template <class T>
T* exact(const std::vector<T>& v) {                               // a heap block of exactly v.size() elements (at least one byte)
  T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

int f2i(float f) {
  int i;
  memcpy(&i, &f, 4);
  return i;
}

struct Case {
  int N, T, nitems;
  std::vector<float> values;
  std::vector<int> sheet, panel, curve, stamp, win;
};

// ---- the straightforward implementation ------------------------------------------------------------------------------------------
const unsigned char FONT[13][7] = {
    {0x0e, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0e}, {0x04, 0x0c, 0x04, 0x04, 0x04, 0x04, 0x0e}, {0x0e, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1f},
    {0x1e, 0x01, 0x01, 0x0e, 0x01, 0x01, 0x1e}, {0x02, 0x06, 0x0a, 0x12, 0x1f, 0x02, 0x02}, {0x1f, 0x10, 0x1e, 0x01, 0x01, 0x11, 0x0e},
    {0x06, 0x08, 0x10, 0x1e, 0x11, 0x11, 0x0e}, {0x1f, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e},
    {0x0e, 0x11, 0x11, 0x0f, 0x01, 0x02, 0x0c}, {0, 0, 0, 0, 0, 0x0c, 0x0c},                {0, 0, 0, 0x1f, 0, 0, 0},
    {0, 0, 0, 0, 0, 0, 0}};

struct Canvas {
  long W, H;
  std::vector<unsigned char> px;
  long band0, band1;                                              // rows a stamp may touch
  void block(int colour, long x0, long y0, long w, long h) {
    for (long y = y0 < band0 ? band0 : y0; y < y0 + h && y < band1; ++y)
      for (long x = x0 < 0 ? 0 : x0; x < x0 + w && x < W; ++x) px[(size_t)(y * W + x)] = (unsigned char)colour;
  }
  void text(const int* st, int g, long x0, long y0) {
    for (int ci = 0; ci < st[3]; ++ci) {
      const int code = (st[4 + ci / 8] >> (4 * (ci % 8))) & 15;
      for (int gy = 0; gy < 7; ++gy)
        for (int gx = 0; gx < 5; ++gx)
          if ((FONT[code][gy] >> (4 - gx)) & 1) block(CURVE_INK, x0 + (long)ci * 6 * g + gx * g, y0 + (long)gy * g, g, g);
    }
  }
};

volatile float sink;
float quant_pos(float v, float ymin, float scale) {              // separately rounded: through a volatile
  sink = v - ymin;
  const float d = sink;
  sink = d * scale;
  return floorf(sink);
}
int ref_row(float v, float ymin, float scale, int PH) {
  if (std::isnan(v)) return -1;
  const float x = quant_pos(v, ymin, scale);
  if (!(x >= 0.0f)) return 0;
  return x > (float)(PH - 1) ? PH - 1 : (int)x;
}
int ref_tick(float v, float ymin, float scale, int PH) {
  const float x = quant_pos(v, ymin, scale);
  if (!(x >= 0.0f) || !(x <= (float)PH)) return -1;
  return x > (float)(PH - 1) ? PH - 1 : (int)x;
}
int fdiv(int a, int b) { return (int)floor((double)a / (double)b); }

// sheet i of the case -> the image, or an empty one when the window is empty
Canvas ref_render(const Case& c, int i) {
  const int* sh = &c.sheet[(size_t)CURVE_SHEET * i];
  const int item = sh[0], p0 = sh[1], np = sh[2], sx = sh[3], PH = sh[4], g = sh[5];
  const int t0 = c.win[4 * item], t1 = c.win[4 * item + 1], m0 = c.win[4 * item + 2], m1 = c.win[4 * item + 3];
  const int frames = t1 - t0, PW = frames * sx;
  int maxY = 0, maxL = 0, legend = 0;
  std::vector<int> hp(np);
  long H = 0;
  for (int p = 0; p < np; ++p) {
    const int* pn = &c.panel[(size_t)CURVE_PANEL * (p0 + p)];
    bool hasx = false;
    for (int s = 0; s < pn[6]; ++s) {
      const int* st = &c.stamp[(size_t)CURVE_STAMP * (pn[5] + s)];
      if (st[0] == 0 && st[3] > maxY) maxY = st[3];
      if (st[0] == 1 && st[3] > 0) hasx = true;
      if (st[0] == 2) legend = 1, maxL = st[3] > maxL ? st[3] : maxL;
    }
    hp[p] = 4 * g + PH + 2 + (hasx ? 9 * g : 4 * g);
    H += hp[p];
  }
  const int ML = maxY ? 6 * g * maxY + 2 * g : 0, MR = legend ? 11 * g + 6 * g * maxL : 0;
  Canvas cv{(long)ML + PW + 2 + MR, H, {}, 0, 0};
  cv.px.assign((size_t)(cv.W * cv.H), CURVE_BACKGROUND);
  long top = 0;
  for (int p = 0; p < np; ++p) {
    const int* pn = &c.panel[(size_t)CURVE_PANEL * (p0 + p)];
    float ymin, scale;
    memcpy(&ymin, &pn[3], 4), memcpy(&scale, &pn[4], 4);
    if (pn[2] & 1) {
      float mn = INFINITY, mx = -INFINITY;
      for (int k = 0; k < pn[1]; ++k)
        for (int t = t0; t < t1; ++t) {
          const float v = c.values[(size_t)c.curve[(size_t)CURVE_CURVE * (pn[0] + k)] * c.T + t];
          if (std::isfinite(v)) mn = v < mn ? v : mn, mx = v > mx ? v : mx;
        }
      if (!(mn <= mx)) ymin = 0.0f, scale = (float)PH;
      else if (mn == mx) sink = mn - 0.5f, ymin = sink, scale = (float)PH;
      else sink = mx - mn, sink = (float)PH / sink, scale = sink, ymin = mn;
    }
    cv.band0 = top, cv.band1 = top + hp[p];
    const long bx0 = ML, bx1 = ML + PW + 1, by0 = top + 4 * g, by1 = by0 + PH + 1;
    for (int s = 0; s < pn[6]; ++s) {
      const int* st = &c.stamp[(size_t)CURVE_STAMP * (pn[5] + s)];
      if (st[0] == 0) {
        float v;
        memcpy(&v, &st[1], 4);
        const int r = ref_tick(v, ymin, scale, PH);
        if (r >= 0) cv.text(st, g, ML - g - 6L * g * st[3], by0 + 1 + (PH - 1 - r) - 3 * g);
      } else if (st[0] == 1) {
        if (st[1] >= t0 && st[1] < t1) cv.text(st, g, ML + 1 + (long)(st[1] - t0) * sx + sx / 2 - (6 * g * st[3] - g) / 2, by1 + 1 + g);
      } else {
        const long xs = bx1 + 1 + 2 * g, ys = by0 + g + 8L * g * st[1];
        cv.block(st[2], xs, ys, 7 * g, 7 * g);
        cv.text(st, g, xs + 8 * g, ys);
      }
    }
    for (long x = bx0; x <= bx1; ++x) cv.px[(size_t)(by0 * cv.W + x)] = cv.px[(size_t)(by1 * cv.W + x)] = CURVE_INK;
    for (long y = by0; y <= by1; ++y) cv.px[(size_t)(y * cv.W + bx0)] = cv.px[(size_t)(y * cv.W + bx1)] = CURVE_INK;
    std::vector<unsigned char> plot((size_t)PH * PW, CURVE_BACKGROUND);           // [row from the bottom][column]
    for (int s = 0; s < pn[6]; ++s) {
      const int* st = &c.stamp[(size_t)CURVE_STAMP * (pn[5] + s)];
      if (st[0]) continue;
      float v;
      memcpy(&v, &st[1], 4);
      const int r = ref_tick(v, ymin, scale, PH);
      if (r >= 0)
        for (int x = 0; x < PW; ++x) plot[(size_t)r * PW + x] = CURVE_GRID;
    }
    for (int t = t0; t < t1; ++t)
      if (pn[7] > 0 && t % pn[7] == 0)
        for (int r = 0; r < PH; ++r) plot[(size_t)r * PW + (t - t0) * sx + sx / 2] = CURVE_GRID;
    if (pn[2] & 2)
      for (int m : {m0, m1})
        if (m >= t0 && m < t1)
          for (int py = 0; py < PH; ++py)
            if ((py / 4) % 2 == 0) plot[(size_t)(PH - 1 - py) * PW + (m - t0) * sx + sx / 2] = CURVE_MARKER;
    for (int k = 0; k < pn[1]; ++k) {
      const int* cu = &c.curve[(size_t)CURVE_CURVE * (pn[0] + k)];
      const int w = cu[2];
      std::vector<int> row(frames + 2);
      for (int j = 0; j < frames + 2; ++j) {
        const int t = t0 - 1 + j;
        row[j] = t < 0 || t >= c.T ? -1 : ref_row(c.values[(size_t)cu[0] * c.T + t], ymin, scale, PH);
      }
      auto light = [&](int x, int r) {
        if (x < 0 || x >= PW) return;
        for (int yy = r - (w - 1) / 2; yy <= r + w / 2; ++yy)
          for (int xx = x - (w - 1) / 2; xx <= x + w / 2; ++xx)
            if (xx >= 0 && xx < PW && yy >= 0 && yy < PH) plot[(size_t)yy * PW + xx] = (unsigned char)cu[1];
      };
      for (int j = 0; j < frames + 2; ++j) {
        if (row[j] < 0) continue;
        const int cx = (j - 1) * sx + sx / 2;
        light(cx, row[j]);
        if (j + 1 < frames + 2 && row[j + 1] >= 0)
          for (int q = 0; q < sx; ++q) {
            const int a = row[j] + fdiv((row[j + 1] - row[j]) * q, sx), b = row[j] + fdiv((row[j + 1] - row[j]) * (q + 1), sx);
            light(cx + q, a);
            for (int r = a; r != b; r += b > a ? 1 : -1) light(cx + q, r);
          }
      }
    }
    for (int py = 0; py < PH; ++py)
      for (int x = 0; x < PW; ++x) cv.px[(size_t)((by0 + 1 + py) * cv.W + bx0 + 1 + x)] = plot[(size_t)(PH - 1 - py) * PW + x];
    top += hp[p];
  }
  return cv;
}

// ---- cases -----------------------------------------------------------------------------------------------------------------------
float value() {
  switch (pick(12)) {
    case 0: return NAN;
    case 1: return INFINITY;
    case 2: return -INFINITY;
    case 3: return 0.0f;
    case 4: return 1.0f;
    case 5: return 1.0000001f;
    case 6: return -1e-7f;
    case 7: return (float)pick(65) / 64.0f;
    default: return (float)(rnd() % 100000) / 80000.0f - 0.1f;
  }
}

void add_stamp(Case& c, int kind, int val, int colour) {
  const int n = pick(CURVE_MAX_CHARS + 1);
  int g[2] = {0, 0};
  for (int k = 0; k < n; ++k) g[k / 8] |= pick(CURVE_GLYPHS) << (4 * (k % 8));
  c.stamp.insert(c.stamp.end(), {kind, val, colour, kind == 1 && pick(3) == 0 ? 0 : n, g[0], g[1], 0, 0});
}

Case make_case(int T, int sx, int PH, int g) {
  Case c;
  c.N = 6, c.T = T, c.nitems = 3;
  for (int i = 0; i < c.N * T; ++i) c.values.push_back(value());
  for (int t = 0; t < T; ++t) c.values[(size_t)4 * T + t] = t == T / 2 ? 3.5f : NAN;          // one finite value
  for (int t = 0; t < T; ++t) c.values[(size_t)5 * T + t] = NAN;
  for (int it = 0; it < c.nitems; ++it) {
    int a = it == 0 ? 0 : pick(T), b = it == 0 ? T : a + 1 + pick(T - a);
    c.win.insert(c.win.end(), {a, b, it == 0 ? -1 : a + pick(b - a), it == 1 ? b - 1 : pick(T + 2) - 1});
    const int np = 1 + pick(3);
    c.sheet.insert(c.sheet.end(), {it, (int)c.panel.size() / CURVE_PANEL, np, sx, PH, g, 0, 0});
    for (int p = 0; p < np; ++p) {
      const int c0 = (int)c.curve.size() / CURVE_CURVE, s0 = (int)c.stamp.size() / CURVE_STAMP, nc = pick(5);
      for (int k = 0; k < nc; ++k) c.curve.insert(c.curve.end(), {pick(c.N), pick(256), 1 + pick(CURVE_MAX_WIDTH), 0});
      const bool autos = pick(3) == 0;
      if (pick(4)) {
        for (int k = pick(4); k > 0; --k) add_stamp(c, 0, f2i(autos ? 3.0f + 0.25f * k : 0.25f * k), 0);
        if (pick(2))
          for (int t = 0; t < T; t += 2) add_stamp(c, 1, t, 0);
        for (int k = pick(3), n = 0; n < k; ++n) add_stamp(c, 2, n, pick(256));
      }
      c.panel.insert(c.panel.end(), {c0, nc, (autos ? 1 : 0) | (pick(2) ? 2 : 0), f2i(0.0f), f2i((float)PH), s0,
                                     (int)c.stamp.size() / CURVE_STAMP - s0, pick(3) ? 1 + pick(4) : 0});
    }
  }
  return c;
}

struct Run {
  float *values, *rng;
  int *sheet, *panel, *curve, *stamp, *win;
  long* meta;
  unsigned char* pix;
  long total;
  CurveTabs tb;
};

Run stage(const Case& c, const std::vector<long>& allow) {
  Run r;
  r.values = exact(c.values), r.sheet = exact(c.sheet), r.panel = exact(c.panel), r.curve = exact(c.curve), r.stamp = exact(c.stamp);
  r.win = exact(c.win);
  const int nimg = (int)c.sheet.size() / CURVE_SHEET, npanels = (int)c.panel.size() / CURVE_PANEL;
  std::vector<long> meta;
  r.total = 0;
  for (int i = 0; i < nimg; ++i) meta.insert(meta.end(), {r.total, -7, -7, allow[i]}), r.total += (allow[i] + 3) & ~3L;
  r.meta = exact(meta);
  r.pix = (unsigned char*)malloc((size_t)(r.total ? r.total : 1));
  memset(r.pix, 77, (size_t)r.total);
  r.rng = (float*)malloc(sizeof(float) * 2 * (size_t)npanels);
  r.tb = CurveTabs{r.sheet, r.panel, r.curve, r.stamp, nimg, npanels, (int)c.curve.size() / CURVE_CURVE, (int)c.stamp.size() / CURVE_STAMP,
                   c.N, c.T, c.nitems};
  return r;
}
void release(Run& r) {
  free(r.values), free(r.sheet), free(r.panel), free(r.curve), free(r.stamp), free(r.win), free(r.meta), free(r.pix), free(r.rng);
}

long images = 0, pixels = 0, refusals = 0;

void check_case(const Case& c) {
  const int nimg = (int)c.sheet.size() / CURVE_SHEET;
  std::vector<Canvas> want;
  std::vector<long> allow;
  for (int i = 0; i < nimg; ++i) want.push_back(ref_render(c, i)), allow.push_back(want.back().W * want.back().H);
  Run r = stage(c, allow);
  curve_render_serial(r.values, r.tb, r.win, r.rng, r.meta, r.pix, r.total);
  for (int i = 0; i < nimg; ++i) {
    const long* m = r.meta + 4L * i;
    CurveGeo G;
    const int frames = c.win[4 * c.sheet[(size_t)CURVE_SHEET * i] + 1] - c.win[4 * c.sheet[(size_t)CURVE_SHEET * i]];
    if (!curve_geo(r.tb, i, frames, &G) || G.W != want[i].W || G.H != want[i].H) fail("layout", i, G.W, want[i].W);
    if (m[1] != want[i].W || m[2] != want[i].H) fail("size", i, m[1], m[2]);
    for (long e = 0; e < m[1] * m[2]; ++e)
      if (r.pix[m[0] + e] != want[i].px[(size_t)e]) fail("pixel", i, e % m[1], e / m[1]);
    for (long e = m[1] * m[2]; e < ((m[1] * m[2] + 3) & ~3L); ++e)
      if (r.pix[m[0] + e] != 77) fail("wrote behind an image", i, e);
    ++images, pixels += m[1] * m[2];
  }
  release(r);
}

// a broken copy of a good case: nothing may be drawn
void check_refused(Case c, const char* what, long allow = 1L << 22) {
  const int nimg = (int)c.sheet.size() / CURVE_SHEET;
  Run r = stage(c, std::vector<long>((size_t)nimg, allow));
  curve_render_serial(r.values, r.tb, r.win, r.rng, r.meta, r.pix, r.total);
  if (r.meta[1] != 0 || r.meta[2] != 0) fail(what, r.meta[1], r.meta[2]);
  for (long e = 0; e < ((allow + 3) & ~3L); ++e)
    if (r.pix[e] != 77) fail(what, e);
  release(r);
  ++refusals;
}

}  // namespace

int main() {
  for (int T : {1, 2, 3, 12, 40})
    for (int sx : {1, 2, 3, 8})
      for (int PH : {7, 64})
        for (int g : {1, 2})
          for (int rep = 0; rep < 3; ++rep) check_case(make_case(T, sx, PH, g));
  // refusals: sheet 0 of a small case, one field at a time
  Case good = make_case(12, 2, 16, 1);
  while (good.panel[1] == 0 || good.panel[6] == 0) good = make_case(12, 2, 16, 1);   // sheet 0's first panel has a curve and a stamp
  check_case(good);
  Case c = good;
  c.curve[2] = 6, check_refused(c, "width 6");
  c = good, c.curve[2] = 0, check_refused(c, "width 0");
  c = good, c.curve[1] = 256, check_refused(c, "colour 256");
  c = good, c.curve[0] = good.N, check_refused(c, "row N");
  c = good, c.curve[0] = -1, check_refused(c, "row -1");
  c = good, c.sheet[2] = 65, check_refused(c, "65 panels");
  c = good, c.sheet[2] = 0, check_refused(c, "no panel");
  c = good, c.sheet[1] = (int)good.panel.size() / CURVE_PANEL, check_refused(c, "first panel past the table");
  c = good, c.sheet[0] = good.nitems, check_refused(c, "item past the windows");
  c = good, c.sheet[0] = -1, check_refused(c, "item -1");
  c = good, c.sheet[3] = 65, check_refused(c, "sx 65");
  c = good, c.sheet[4] = PNG_MAX_DIM + 1, check_refused(c, "plot height");
  c = good, c.sheet[5] = 9, check_refused(c, "glyph scale 9");
  c = good, c.win[1] = good.T + 1, check_refused(c, "window past the clip");
  c = good, c.win[0] = 12, c.win[1] = 12, check_refused(c, "empty window");
  c = good, c.win[0] = -1, check_refused(c, "window from -1");
  c = good, c.panel[1] = 1 << 20, check_refused(c, "curves past the table");
  c = good, c.panel[0] = -1, check_refused(c, "first curve -1");
  c = good, c.panel[6] = 1 << 20, check_refused(c, "stamps past the table");
  c = good, c.panel[7] = -1, check_refused(c, "xtick_every -1");
  c = good, c.stamp[(size_t)CURVE_STAMP * good.panel[5]] = 3, check_refused(c, "stamp kind 3");
  c = good, c.stamp[(size_t)CURVE_STAMP * good.panel[5] + 3] = 17, check_refused(c, "17 characters");
  c = good, c.stamp[(size_t)CURVE_STAMP * good.panel[5] + 3] = 1, c.stamp[(size_t)CURVE_STAMP * good.panel[5] + 4] = 13,
  check_refused(c, "glyph 13");
  check_refused(good, "too few pixels allowed", 16);
  {  // curves x (window + 2) beyond the cap: 2 curves over 8191 frames fit (16386 > 16384 does not)
    Case big;
    big.N = 1, big.T = 8191, big.nitems = 1;
    big.values.assign(8191, 0.5f);
    big.win = {0, 8191, -1, -1};
    big.sheet = {0, 0, 1, 1, 8, 1, 0, 0};
    big.curve = {0, 1, 1, 0, 0, 2, 1, 0};
    big.panel = {0, 2, 0, f2i(0.0f), f2i(8.0f), 0, 0, 0};
    check_refused(big, "curves x (window + 2) = 16386");
    big.win[1] = 8190;
    check_case(big);                                              // 16384: the cap itself is drawn
  }
  printf("curve_host_check: %ld images, %ld pixels equal to the straightforward renderer; %ld refusals drew nothing\n", images, pixels,
         refusals);
  return 0;
}
