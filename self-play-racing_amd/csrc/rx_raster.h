// rx_raster.h -- the raster rules of the renderer (rx_raster_static / _trail /
// _frame, ABI v25 additive) as one set of inline functions compiled twice: by
// hipcc for gfx950 (rx_render.hip) and for the host twins in rx_api.cpp.  The
// pixel tests are integer-only; the two places that touch doubles
// (convert_coords and the car corners) use single IEEE-754 operations in a
// fixed order plus rx_math.h's rx_sincos, and both translation units are
// compiled with -ffp-contract=off.  Device and host therefore give the same
// bytes (tests/test_render_gpu.py).
//
// Rules (DESIGN.md §4 "Rendering"):
//  * all tests run in doubled integer coordinates: a vertex (X, Y) is (2X, 2Y),
//    pixel (i, j) -- column i, row j -- is sampled at (2i+1, 2j+1), so a sample
//    never shares a row or a column with a vertex;
//  * polygon fill: even-odd.  Edge a->b counts for sample s when
//    (a.y < s.y) != (b.y < s.y) and the edge meets the row strictly to the
//    right of s; a sample on the edge does not count it;
//  * thick line of width w: the capsule of pixel centres within w/2 of the
//    segment (round ends); in doubled coordinates the distance bound is w;
//  * screen coordinates of moving things are clamped to [-4096, 8191] before
//    the truncation to int; NaN makes the point invisible.  With sizes up to
//    2048 every difference below is under 2^15 in magnitude, a cross product
//    under 2^31 and its square under 2^62: exact in int64.
#pragma once

#include <stdint.h>

#include "rx.h"
#include "rx_math.h"

#define RX_RASTER_TILE 16       // k_raster_static: pixels per tile side
#define RX_RASTER_EDGE_W 6      // int32 per edge: ax, ay, bx, by, class, width (0 = fill edge)
#define RX_RASTER_LO (-4096.0)  // clamp of moving screen coordinates
#define RX_RASTER_HI 8191.0
#define RX_RASTER_TRAIL_W 3     // path width (visualization.py:113)
#define RX_RASTER_CAR_W 2       // car outline width (visualization.py:120)

// One car of one image in screen coordinates, and the pixel box outside which
// it cannot colour anything.
struct rx_car_quad {
  int32_t c[4][2];
  int32_t valid;
  int32_t lo_x, hi_x, lo_y, hi_y;
};

RX_FN int32_t rx_rs_min(int32_t a, int32_t b) { return a < b ? a : b; }
RX_FN int32_t rx_rs_max(int32_t a, int32_t b) { return a > b ? a : b; }

// convert_coords (visualization.py:6-9) with the clamp; false for a NaN result.
RX_FN bool rx_rs_screen(double x, double y, double scale, double ox, double oy, int size, int32_t* X, int32_t* Y) {
  double sx = (x + ox) * scale;
  double sy = (double)size - (y + oy) * scale;
  if (sx != sx || sy != sy) return false;
  sx = sx < RX_RASTER_LO ? RX_RASTER_LO : (sx > RX_RASTER_HI ? RX_RASTER_HI : sx);
  sy = sy < RX_RASTER_LO ? RX_RASTER_LO : (sy > RX_RASTER_HI ? RX_RASTER_HI : sy);
  *X = (int32_t)sx;  // int(): toward zero
  *Y = (int32_t)sy;
  return true;
}

// Even-odd crossing of edge a->b for sample s (all doubled).
RX_FN int rx_rs_cross(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t sx, int32_t sy) {
  if ((ay < sy) == (by < sy)) return 0;
  const int64_t cr = (int64_t)(bx - ax) * (sy - ay) - (int64_t)(by - ay) * (sx - ax);
  return by > ay ? cr > 0 : cr < 0;
}

// Sample s inside the capsule of width w around a->b (all doubled).
RX_FN int rx_rs_capsule(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t sx, int32_t sy, int32_t w) {
  const int64_t dx = bx - ax, dy = by - ay, px = sx - ax, py = sy - ay;
  const int64_t L = dx * dx + dy * dy, u = px * dx + py * dy, w2 = (int64_t)w * w;
  if (L == 0 || u <= 0) return px * px + py * py <= w2;
  if (u >= L) {
    const int64_t qx = sx - bx, qy = sy - by;
    return qx * qx + qy * qy <= w2;
  }
  const int64_t cr = px * dy - py * dx;
  return cr * cr <= w2 * L;
}

// Can edge e (RX_RASTER_EDGE_W ints, screen coordinates) change any pixel of
// columns i0..i1, rows j0..j1?  Conservative: a true answer costs time only.
RX_FN bool rx_rs_edge_hits_tile(const int32_t* e, int i0, int j0, int i1, int j1) {
  const int32_t X0 = 2 * i0 + 1, X1 = 2 * i1 + 1, Y0 = 2 * j0 + 1, Y1 = 2 * j1 + 1;
  const int32_t ax = 2 * e[0], ay = 2 * e[1], bx = 2 * e[2], by = 2 * e[3], w = e[5];
  const int32_t xlo = rx_rs_min(ax, bx), xhi = rx_rs_max(ax, bx), ylo = rx_rs_min(ay, by), yhi = rx_rs_max(ay, by);
  if (w > 0) return !(xhi + w < X0 || xlo - w > X1 || yhi + w < Y0 || ylo - w > Y1);
  // a fill edge counts for s only when ylo < s.y <= yhi and it passes right of s
  return !(yhi < Y0 || ylo >= Y1 || xhi <= X0);
}

// Edge e against the sample of pixel (i, j): fill edges toggle bit `class` of
// *parity, capsules raise *cls to their class.
RX_FN void rx_rs_edge_px(const int32_t* e, int32_t sx, int32_t sy, uint32_t* parity, int32_t* cls) {
  const int32_t ax = 2 * e[0], ay = 2 * e[1], bx = 2 * e[2], by = 2 * e[3], c = e[4] & 7, w = e[5];
  if (w > 0) {
    if (c > *cls && rx_rs_capsule(ax, ay, bx, by, sx, sy, w)) *cls = c;
  } else if (rx_rs_cross(ax, ay, bx, by, sx, sy)) {
    *parity ^= 1u << c;
  }
}

// Later classes overwrite earlier ones: the highest class that covers the pixel.
RX_FN uint8_t rx_rs_static_class(uint32_t parity, int32_t cls) {
  for (int32_t c = 7; c > cls; --c)
    if (parity >> c & 1u) return (uint8_t)c;
  return (uint8_t)cls;
}

// Car.get_corners (environment/car.py:26-43) through convert_coords.  The
// rotation is written out with separate multiplies and adds.
RX_FN void rx_rs_car(double x, double y, double angle, double scale, double ox, double oy, int size, rx_car_quad* q) {
  const double lx[4] = {2.0, 2.0, -2.0, -2.0}, ly[4] = {1.0, -1.0, -1.0, 1.0};
  q->valid = 0;
  q->lo_x = q->lo_y = 0;
  q->hi_x = q->hi_y = -1;
  for (int i = 0; i < 4; ++i) q->c[i][0] = q->c[i][1] = 0;
  if (!((x - x) == 0.0 && (y - y) == 0.0 && (angle - angle) == 0.0)) return;  // NaN or inf pose
  if (angle < -1048576.0 || angle > 1048576.0) return;  // outside rx_sincos' range
  double s, c;
  rx_sincos(angle, &s, &c);
  int32_t lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
  for (int i = 0; i < 4; ++i) {
    const double wx = (c * lx[i] - s * ly[i]) + x;
    const double wy = (s * lx[i] + c * ly[i]) + y;
    int32_t X, Y;
    if (!rx_rs_screen(wx, wy, scale, ox, oy, size, &X, &Y)) return;
    q->c[i][0] = X;
    q->c[i][1] = Y;
    lo_x = i ? rx_rs_min(lo_x, X) : X;
    hi_x = i ? rx_rs_max(hi_x, X) : X;
    lo_y = i ? rx_rs_min(lo_y, Y) : Y;
    hi_y = i ? rx_rs_max(hi_y, Y) : Y;
  }
  // sample 2i+1 within [2 lo - w, 2 hi + w], w = 2: i in [lo - 1, hi]; one more each side
  q->lo_x = lo_x - 2;
  q->hi_x = hi_x + 1;
  q->lo_y = lo_y - 2;
  q->hi_y = hi_y + 1;
  q->valid = 1;
}

// 0: the car leaves pixel (i, j) alone; 1: fill; 2: outline (drawn after the fill).
RX_FN int rx_rs_car_px(const rx_car_quad* q, int32_t i, int32_t j) {
  if (!q->valid || i < q->lo_x || i > q->hi_x || j < q->lo_y || j > q->hi_y) return 0;
  const int32_t sx = 2 * i + 1, sy = 2 * j + 1;
  int par = 0, line = 0;
  for (int a = 0; a < 4; ++a) {
    const int b = (a + 1) & 3;
    const int32_t ax = 2 * q->c[a][0], ay = 2 * q->c[a][1], bx = 2 * q->c[b][0], by = 2 * q->c[b][1];
    par ^= rx_rs_cross(ax, ay, bx, by, sx, sy);
    line |= rx_rs_capsule(ax, ay, bx, by, sx, sy, RX_RASTER_CAR_W);
  }
  return line ? 2 : par;
}

// Byte select: byte p of the result is byte sel.byte[p] (0..7) of the eight
// bytes hi:lo -- one v_perm_b32 on the device.
RX_FN uint32_t rx_rs_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = (uint64_t)hi << 32 | lo;
  uint32_t r = 0;
  for (int p = 0; p < 4; ++p) r |= (uint32_t)(v >> (8 * (sel >> (8 * p) & 7)) & 0xff) << (8 * p);
  return r;
#endif
}

// Four pixels at once, byte p of every word = pixel p.  cw: static classes, tw:
// trail bytes -> the red, green and blue bytes (visualization.py:103-107, :113,
// :243).  A palette index per byte -- 0..3 the class (above 3: background),
// 4 trail 0, 5 trail 1 over it -- then one byte select per channel.
RX_FN void rx_rs_base_colour4(uint32_t cw, uint32_t tw, uint32_t* R, uint32_t* G, uint32_t* B) {
  const uint32_t hi = cw & 0xfcfcfcfcu;
  const uint32_t nz = (((hi & 0x7f7f7f7fu) + 0x7f7f7f7fu) | hi) & 0x80808080u;  // bit 7 of a byte: its class is above 3
  uint32_t idx = cw & 0x03030303u & ~((nz >> 7) * 0xffu);
  const uint32_t m0 = (tw >> 4 & 0x01010101u) * 0xffu, m1 = (tw >> 5 & 0x01010101u) * 0xffu;
  idx = (idx & ~m0) | (0x04040404u & m0);
  idx = (idx & ~m1) | (0x05050505u & m1);
  // palette bytes 0..5: (50,50,50) (180,180,180) (0,0,0) (0,255,0) (255,100,100) (100,100,255)
  *R = rx_rs_perm(0x000064ffu, 0x0000b432u, idx);
  *G = rx_rs_perm(0x00006464u, 0xff00b432u, idx);
  *B = rx_rs_perm(0x0000ff64u, 0x0000b432u, idx);
}

// Do the 4 pixels of columns i0..i0+3, row j meet a car's box?  Conservative.
RX_FN bool rx_rs_near_cars(const rx_car_quad* cars, int32_t i0, int32_t j) {
  bool near = false;
  for (int q = 0; q < 2; ++q)
    near |= cars[q].valid && j >= cars[q].lo_y && j <= cars[q].hi_y && i0 + 3 >= cars[q].lo_x && i0 <= cars[q].hi_x;
  return near;
}

// The 12 bytes R G B R G B ... of pixels (i0..i0+3, j) as three little-endian
// words: the base colours with the cars over them, car 1 last (car 0 fill
// (255,0,0), outline (150,0,0); car 1 (0,0,255), (0,0,150)).  cars[2]: a car
// that does not exist has valid = 0.
RX_FN void rx_rs_group(uint32_t cw, uint32_t tw, const rx_car_quad* cars, int32_t i0, int32_t j, uint32_t* o) {
  uint32_t R, G, B;
  rx_rs_base_colour4(cw, tw, &R, &G, &B);
  if (rx_rs_near_cars(cars, i0, j)) {
    for (int p = 0; p < 4; ++p)
      for (int q = 0; q < 2; ++q) {
        const int what = rx_rs_car_px(&cars[q], i0 + p, j);
        if (!what) continue;
        const uint32_t m = 0xffu << (8 * p), v = (what == 2 ? 150u : 255u) << (8 * p);
        R = (R & ~m) | (q == 0 ? v : 0u);
        G = G & ~m;
        B = (B & ~m) | (q == 0 ? 0u : v);
      }
  }
  o[0] = rx_rs_perm(B, rx_rs_perm(G, R, 0x01000400u), 0x03040100u);  // R0 G0 B0 R1
  o[1] = rx_rs_perm(B, rx_rs_perm(G, R, 0x06020005u), 0x03020500u);  // G1 B1 R2 G2
  o[2] = rx_rs_perm(B, rx_rs_perm(G, R, 0x00070300u), 0x07020106u);  // B2 R3 G3 B3
}

// The pixel box (clipped to the image) that the trail capsule a->b can touch;
// false when it is empty.
RX_FN bool rx_rs_trail_box(int32_t ax, int32_t ay, int32_t bx, int32_t by, int size, int32_t* i0, int32_t* j0,
                           int32_t* i1, int32_t* j1) {
  *i0 = rx_rs_max(rx_rs_min(ax, bx) - 2, 0);
  *i1 = rx_rs_min(rx_rs_max(ax, bx) + 2, size - 1);
  *j0 = rx_rs_max(rx_rs_min(ay, by) - 2, 0);
  *j1 = rx_rs_min(rx_rs_max(ay, by) + 2, size - 1);
  return *i0 <= *i1 && *j0 <= *j1;
}
