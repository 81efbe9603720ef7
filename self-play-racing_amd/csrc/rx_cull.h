// rx_cull.h -- the culling tables of a track table (include/rx.h, rx_cull_tables)
// as one set of inline functions compiled twice: by hipcc for gfx950
// (rx_cull.hip, a wavefront per slot) and for the host (rx_build_cull_tables_host
// and, through it, rx_upload_tracks in rx_api.cpp).  One statement of the rules:
// the box of a run of segments or waypoints, the union of boxes, the outward
// float32 rounding, the quadrant permutation, the circle and the longest segment.
//
// Every value is a min / max of inputs (exact in any order, so a lane-strided
// reduction gives the host loop's values), a float conversion, or a short chain
// of separately rounded binary64 operations (-ffp-contract=off in both builds).
// The one exception is the circle radius: hypot is ocml's on the device and
// libm's on the host.  A min / max of +0.0 and -0.0 may keep
// either zero: the tables are equal by value, not by bytes.
//
// The functions that walk a slot take (lane, n_lanes): the kernel passes its lane
// and 64, the host twin 0 and 1.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rx_internal.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define RX_CULL_HD __host__ __device__ inline
#else
#define RX_CULL_HD static inline
#endif

#define RX_CULL_MAX_W (64 * RX_WP_CHUNK * RX_WP_SUPER)  // the closest-waypoint super-chunk mask is 64 bits
#define RX_CULL_MAX_SUPER 64

// boxes per slot: leaf and super boxes over both sides, waypoint chunks and super-chunks
struct rx_cull_counts {
  int32_t leaf, super, wchunk, wsuper;
};

RX_CULL_HD int32_t rx_cull_ceil_div(int32_t a, int32_t b) { return (int32_t)(((int64_t)a + b - 1) / b); }

RX_CULL_HD rx_cull_counts rx_cull_slot_counts(int32_t W, int32_t G, int32_t SG) {
  rx_cull_counts c = {0, 0, 0, 0};
  if (G <= 0) return c;
  const int32_t nch = rx_cull_ceil_div(W, G);
  c.leaf = 2 * nch;
  c.super = SG > 0 ? 2 * rx_cull_ceil_div(nch, SG) : 0;
  c.wchunk = rx_cull_ceil_div(W, RX_WP_CHUNK);
  c.wsuper = rx_cull_ceil_div(c.wchunk, RX_WP_SUPER);
  return c;
}

RX_CULL_HD double rx_cull_lo(double a, double b) { return b < a ? b : a; }
RX_CULL_HD double rx_cull_hi(double a, double b) { return b > a ? b : a; }

RX_CULL_HD void rx_cull_box_empty(double b[4]) {
  b[0] = b[1] = 1e300;
  b[2] = b[3] = -1e300;
}

RX_CULL_HD void rx_cull_box_point(double b[4], double x, double y) {
  b[0] = rx_cull_lo(b[0], x);
  b[1] = rx_cull_lo(b[1], y);
  b[2] = rx_cull_hi(b[2], x);
  b[3] = rx_cull_hi(b[3], y);
}

// union of boxes (a wave's partial boxes; a super box is the union of its leaves,
// which equals the box of their segments: rx_cull_seg_box over the longer run)
RX_CULL_HD void rx_cull_box_union(double b[4], const double o[4]) {
  b[0] = rx_cull_lo(b[0], o[0]);
  b[1] = rx_cull_lo(b[1], o[1]);
  b[2] = rx_cull_hi(b[2], o[2]);
  b[3] = rx_cull_hi(b[3], o[3]);
}

// both end points of segment g = (start.x, start.y, v2.x, v2.y)
RX_CULL_HD void rx_cull_box_segment(double b[4], const double* g) {
  rx_cull_box_point(b, g[0], g[1]);
  rx_cull_box_point(b, g[0] + g[2], g[1] + g[3]);
}

// the box of segments [j0, j1) of a slot's segment rows s
RX_CULL_HD void rx_cull_seg_box(const double* s, int64_t j0, int64_t j1, double b[4]) {
  rx_cull_box_empty(b);
  for (int64_t j = j0; j < j1; ++j) rx_cull_box_segment(b, s + 4 * j);
}

// the box of waypoints [i0, i1) of a slot's waypoint rows w
RX_CULL_HD void rx_cull_wp_box(const double* w, int64_t i0, int64_t i1, double b[4]) {
  rx_cull_box_empty(b);
  for (int64_t i = i0; i < i1; ++i) rx_cull_box_point(b, w[2 * i], w[2 * i + 1]);
}

// float32 rounded towards -inf / +inf: the nearest float, stepped once when it
// landed on the wrong side
RX_CULL_HD float rx_cull_f32_down(double x) {
  float v = (float)x;
  if ((double)v > x) v = nextafterf(v, -HUGE_VALF);
  return v;
}
RX_CULL_HD float rx_cull_f32_up(double x) {
  float v = (float)x;
  if ((double)v < x) v = nextafterf(v, HUGE_VALF);
  return v;
}

// the float32 box that contains the float64 box: a test that keeps it keeps the f64 one
RX_CULL_HD void rx_cull_box_f32(const double b[4], float f[4]) {
  f[0] = rx_cull_f32_down(b[0]);
  f[1] = rx_cull_f32_down(b[1]);
  f[2] = rx_cull_f32_up(b[2]);
  f[3] = rx_cull_f32_up(b[3]);
}

// quadrant q: (near.x, near.y, far.x, far.y) for a ray direction whose x (bit 0) /
// y (bit 1) component is negative -- the slab planes the ray enters and leaves through
RX_CULL_HD void rx_cull_quadrant(int q, const float b[4], float o[4]) {
  o[0] = (q & 1) ? b[2] : b[0];
  o[1] = (q & 2) ? b[3] : b[1];
  o[2] = (q & 1) ? b[0] : b[2];
  o[3] = (q & 2) ? b[1] : b[3];
}

// box i of a float table of `count` boxes: block 0 and the four quadrant blocks
RX_CULL_HD void rx_cull_store_f32(float* tab, int64_t count, int64_t i, const double b[4]) {
  float f[4], o[4];
  rx_cull_box_f32(b, f);
  for (int c = 0; c < 4; ++c) tab[4 * i + c] = f[c];
  for (int q = 0; q < 4; ++q) {
    rx_cull_quadrant(q, f, o);
    for (int c = 0; c < 4; ++c) tab[4 * ((q + 1) * count + i) + c] = o[c];
  }
}

RX_CULL_HD void rx_cull_store_f64(double* tab, int64_t i, const double b[4]) {
  for (int c = 0; c < 4; ++c) tab[4 * i + c] = b[c];
}

// Pass 1 over the 2 W segments of a slot: seg_f (nearest rounding), and this
// lane's share of the box of all end points and of the longest segment
RX_CULL_HD void rx_cull_extent(const double* s, int32_t W, int lane, int n_lanes, float* seg_f, double b[4],
                               double* longest) {
  rx_cull_box_empty(b);
  double L = 0.0;
  for (int32_t j = lane; j < 2 * W; j += n_lanes) {
    const double* g = s + 4 * (int64_t)j;
    for (int c = 0; c < 4; ++c) seg_f[4 * (int64_t)j + c] = (float)g[c];
    rx_cull_box_segment(b, g);
    L = rx_cull_hi(L, __builtin_sqrt(g[2] * g[2] + g[3] * g[3]));
  }
  *longest = L;
}

// Pass 2: this lane's share of the largest distance from (cx, cy) to an end point
RX_CULL_HD double rx_cull_reach(const double* s, int32_t W, int lane, int n_lanes, double cx, double cy) {
  double r = 0.0;
  for (int32_t j = lane; j < 2 * W; j += n_lanes) {
    const double* g = s + 4 * (int64_t)j;
    const double ex = g[0] + g[2], ey = g[1] + g[3];
    r = rx_cull_hi(r, hypot(g[0] - cx, g[1] - cy));
    r = rx_cull_hi(r, hypot(ex - cx, ey - cy));
  }
  return r;
}

// slot_geo from the box of all end points, the reach and the longest segment;
// both lengths rounded up: the kernels need upper bounds
RX_CULL_HD void rx_cull_geo(const double b[4], double reach, double longest, double geo[4]) {
  geo[0] = 0.5 * (b[0] + b[2]);
  geo[1] = 0.5 * (b[1] + b[3]);
  geo[2] = reach * (1.0 + 1e-12) + 1e-9;
  geo[3] = longest * (1.0 + 1e-12) + 1e-12;
}

// where a slot's boxes go: the slot's first box in each of the four arrays, the
// arrays' totals (the quadrant blocks' stride) and the arrays
struct rx_cull_slot {
  int32_t chunk0, super0, wchunk0, wsuper0;
  int64_t n_leaf, n_super;
  double *chunk_box, *super_box, *wchunk_box, *wsuper_box;
  float *chunk_box_f, *super_box_f;
};

// Pass 3: this lane's share of the slot's four box tables (a box per iteration)
RX_CULL_HD void rx_cull_boxes(const double* s, const double* w, int32_t W, int32_t G, int32_t SG, int lane,
                              int n_lanes, const rx_cull_slot* o) {
  const rx_cull_counts n = rx_cull_slot_counts(W, G, SG);
  double b[4];
  const int32_t nch = n.leaf / 2, nsup = n.super / 2;
  for (int32_t i = lane; i < n.leaf; i += n_lanes) {  // G segments of one side
    const int32_t side = i / nch, c = i % nch;
    const int64_t j0 = (int64_t)c * G, j1 = j0 + G < W ? j0 + G : W;
    rx_cull_seg_box(s, (int64_t)side * W + j0, (int64_t)side * W + j1, b);
    rx_cull_store_f64(o->chunk_box, o->chunk0 + (int64_t)i, b);
    rx_cull_store_f32(o->chunk_box_f, o->n_leaf, o->chunk0 + (int64_t)i, b);
  }
  for (int32_t i = lane; i < n.super; i += n_lanes) {  // SG leaves = SG * G segments of one side
    const int32_t side = i / nsup, u = i % nsup;
    const int64_t j0 = (int64_t)u * SG * G, j1 = j0 + (int64_t)SG * G < W ? j0 + (int64_t)SG * G : W;
    rx_cull_seg_box(s, (int64_t)side * W + j0, (int64_t)side * W + j1, b);
    rx_cull_store_f64(o->super_box, o->super0 + (int64_t)i, b);
    rx_cull_store_f32(o->super_box_f, o->n_super, o->super0 + (int64_t)i, b);
  }
  for (int32_t i = lane; i < n.wchunk; i += n_lanes) {
    const int64_t i0 = (int64_t)i * RX_WP_CHUNK, i1 = i0 + RX_WP_CHUNK < W ? i0 + RX_WP_CHUNK : W;
    rx_cull_wp_box(w, i0, i1, b);
    rx_cull_store_f64(o->wchunk_box, o->wchunk0 + (int64_t)i, b);
  }
  for (int32_t i = lane; i < n.wsuper; i += n_lanes) {
    const int64_t span = RX_WP_CHUNK * RX_WP_SUPER, i0 = (int64_t)i * span, i1 = i0 + span < W ? i0 + span : W;
    rx_cull_wp_box(w, i0, i1, b);
    rx_cull_store_f64(o->wsuper_box, o->wsuper0 + (int64_t)i, b);
  }
}

// rx_patch_tracks: this lane's share of n rows of S doubles copied from src to dst
// (a row per iteration: 16 B per lane for wp / nrm rows, 32 B for seg rows)
template <int S>
RX_CULL_HD void rx_cull_copy_rows(const double* src, double* dst, int32_t n, int lane, int n_lanes) {
  for (int32_t i = lane; i < n; i += n_lanes)
    for (int c = 0; c < S; ++c) dst[S * (int64_t)i + c] = src[S * (int64_t)i + c];
}

// what rx_patch_tracks' kernel is told of a listed slot, 8 int32 per slot
struct rx_patch_slot {
  int32_t slot, src0, wp0, W;  // the slot, its first source and destination waypoint row, its waypoints
  int32_t chunk0, super0, wchunk0, wsuper0;  // the slot's first box in the four box arrays
};

// the slot's 128-byte header row (geo: the slot's slot_geo row; zeros without culling tables)
RX_CULL_HD void rx_cull_header(rx_slot_hdr* r, int32_t wp0, int32_t W, const rx_cull_slot* o, const double* geo,
                               const double* meta) {
  r->wp0 = wp0;
  r->W = W;
  r->chunk_off = o->chunk0;
  r->super_off = o->super0;
  r->wchunk_off = o->wchunk0;
  r->wsuper_off = o->wsuper0;
  r->pad0 = r->pad1 = 0;
  for (int i = 0; i < 4; ++i) r->geo[i] = geo[i];
  for (int i = 0; i < 8; ++i) r->meta[i] = meta[i];
}
