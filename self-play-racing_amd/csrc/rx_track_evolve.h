// rx_track_evolve.h -- the rules of TRACK EVOLUTION (rx_track_evolve_plan /
// rx_track_evolve, ABI v25 additive): what goes into the track slots the curriculum
// retires.  A retired slot is filled on the device, either by a fresh track of the
// host generator's distribution or by a small edit of a track the replay scores
// still rank high (ACCEL, Parker-Holder et al. 2022).  As rx_track_replay.h, one set
// of inline functions compiled twice: by hipcc for gfx950 (rx_track_evolve.hip) and
// as plain C++ for the host twins (rx_track_evolve_host.cpp), both with
// -ffp-contract=off.  Floating point is float64 and every step is ONE separately
// rounded + - * / sqrt; the only transcendental is rx_sincos (rx_math.h), which is
// bit-identical on host and device.  No atan2, no hypot, no pow, no ocml call: the
// kernels, the host twins and a Python restatement (tests/test_track_evolve_cpu.py)
// agree byte for byte.
//
// Rules (DESIGN.md §4 "Track evolution"):
//  * The hash stream of spawned slot k at generation g:
//      h0 = splitmix64(seed ^ splitmix64(((uint64)g << 32) ^ k)),  h_{i+1} = splitmix64(h_i)
//    Every draw consumes one h, in the order written below.  An integer below n is
//    mulhi64(h, n); a unit real is u = (double)(h >> 11) * 2^-53; a bit is h >> 63.
//  * draw 0, the kind: EDIT when u < edit_frac and F = cdf_score[n - 1] > 0, else FRESH.
//  * FRESH (the distribution of the host generator's gen_tracks / gen_random_track,
//    not its MT19937 stream), draws 1..6 then P offsets then P radii:
//      P = 10 + mulhi(h, 5);  base = 50 + mulhi(h, 30);  var = 10 + mulhi(h, base / 2 - 20)
//      jitter = 0.2 + 0.5 * u;  smooth = 0.2 + 0.5 * u;  width = 6 + mulhi(h, 4)
//      spacing = 2pi / P;  half = (jitter * spacing) / 2
//      angle_i = i * spacing + (-half + (2 * half) * u_i)                  (P draws)
//      v_i = base + (-var + (2 * var) * u_i)                               (P draws)
//      r_0 = v_0;  r_i = (1 - smooth) * v_i + smooth * r_{i-1};  at the end r_0 = (r_0 + r_{P-1}) / 2
//      cp_i = (r_i * cos(angle_i), r_i * sin(angle_i))  through rx_sincos
//    The angles are NOT reduced mod 2pi and NOT sorted, as the host generator does:
//    |offset| <= 0.35 * spacing cannot reorder the points, and a negative angle_0
//    names the same closed polygon.  Radii lie in [base - var, base + var], within
//    [36, 107] = [50 - 14, 79 + 28] over all draws.
//  * EDIT, draws 1..3 then four per edit:
//      parent = search(cdf_score, n, mulhi(h, F))   -- the rank table as it stands, the
//               OLD control points: a slot that is being replaced may be a parent
//      width' = clip((width + (double)mulhi(h, 3)) - 1, 6, 9);  n_edits = 1 + mulhi(h, 3)
//      the child starts as the parent's P points; then per edit, on the child so far:
//      i = mulhi(h, P);  radial = (h >> 63 == 0);  nb = h >> 63 ? next : previous;  u
//      r = sqrt(x * x + y * y) of p_i
//      radial:   r' = clip(r * (0.8 + 0.4 * u), 36, 107);  q = p_i * (r' / r)
//      angular:  q = p_i + (0.35 * u) * (p_nb - p_i);  q = q * (r / sqrt(qx * qx + qy * qy))
//      (all four draws are consumed whichever the kind).
//    The edit is ACCEPTED when q differs from p_i, cross(p_prev, q) > 0,
//    cross(q, p_next) > 0 and both squared chords |q - p_prev|^2, |p_next - q|^2 are
//    at least 23.04 (4.8^2; the generator's own smallest chord is
//    2 * 36 * sin(0.15 * 2pi / 14) ~ 4.84).  Otherwise it is DROPPED, not repaired
//    (a NaN fails every comparison and is dropped).  The number applied is plan[.][3].
//  * The plan row of spawned slot j is (kind, parent or -1, P, edits applied).  A
//    slot that is not spawned is copied: its points and its width, bit for bit.
//  * A slot whose span in the new offsets is not the P of its rule (the caller's
//    offsets do not follow the plan) is not written at all; its width becomes NaN,
//    which rx_build_tracks marks as a bad track.  The kernel never writes outside
//    [cp_off_new[k], cp_off_new[k + 1]).
//
// Rules of the IN-PLACE form (rx_track_evolve_classes / _inplace / _commit; DESIGN.md §4
// "Track evolution in place"): a spawned slot keeps its point count, so no offset moves.
//  * The class table.  P_k = cp_off[k + 1] - cp_off[k]; w_k = cdf_score[k] - cdf_score[k - 1]
//    (w_0 = cdf_score[0]).  order[n_tracks] holds the slots sorted by (P_k, k) ascending: a
//    stable counting sort by point count.  A slot whose P_k lies outside [1, RX_TRACK_MAX_P]
//    belongs to no class: it weighs 0 and follows the last class, in slot order.
//    cdf_class[i] is the inclusive integer scan of w[order[i]], through the classes without
//    restarting; class_end[p] = the number of slots with 1 <= P <= p (class_end[0] = 0), for
//    p <= RX_TRACK_MAX_P.  All integers: the table is unique whatever order it is built in.
//  * The stream of spawned slot k at generation g is rx_te_stream, the draws keep their places.
//  * draw 0, the kind: with c = P_k, lo = class_end[c - 1], hi = class_end[c],
//    base = lo ? cdf_class[lo - 1] : 0 and F = cdf_class[hi - 1] - base: EDIT when
//    u < edit_frac and F > 0, else FRESH.
//  * draw 1, EDIT: t = base + mulhi(h, F); parent = order[i] for the smallest i in [lo, hi)
//    with t < cdf_class[i].  The parent has the slot's point count; it may be the slot itself
//    or another slot that is being replaced: parents are read from the pool as it stood.
//    The child is rx_te_edit.  FRESH: the draw is consumed and discarded (the point count is
//    the slot's own) and the track is rx_te_fresh(h0, P_k): bit for bit the track
//    rx_track_evolve writes for the same (seed, g, k) whenever that path draws the same P.
//  * The plan row is (kind, parent or -1, P_k, edits applied).  The track goes into a compact
//    staging buffer, cp_out[out_off[j] .. out_off[j + 1]) and width_out[j], never into the pool.
//    A slot whose staging span is not P_k, or whose P_k lies outside [1, RX_TRACK_MAX_P], or
//    whose slot index lies outside the pool, is not written at all: width_out[j] becomes NaN
//    and its plan row is (FRESH, -1, P_k, 0).  Nothing is written outside the slot's span.
//  * The commit copies the staging rows over the spawned slots' spans of cp and width; every
//    other byte of the pool stays.  A slot that was not written (the same three conditions)
//    takes the NaN width and keeps its points.
#pragma once

#include <stdint.h>

#include "rx.h"
#include "rx_curriculum.h"  // rx_tc_mulhi64, rx_tc_search
#include "rx_league.h"      // rx_lg_splitmix64
#include "rx_math.h"        // rx_sincos, rx_clip, RX_SQRT
#include "rx_spline.h"      // RX_TRACK_MAX_P

#define RX_TRACK_EVOLVE_W 4          // plan row: kind, parent, P, edits applied
#define RX_TRACK_EVOLVE_FRESH 0
#define RX_TRACK_EVOLVE_EDIT 1
#define RX_TRACK_EVOLVE_R_MIN 36.0
#define RX_TRACK_EVOLVE_R_MAX 107.0
#define RX_TRACK_EVOLVE_CHORD2 23.04
#define RX_TRACK_EVOLVE_TWO_PI 6.283185307179586  // the double 2 * pi

RX_FN uint64_t rx_te_stream(uint64_t seed, uint32_t g, uint32_t k) {
  return rx_lg_splitmix64(seed ^ rx_lg_splitmix64(((uint64_t)g << 32) ^ (uint64_t)k));
}

RX_FN double rx_te_unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }

RX_FN double rx_te_nan() {
  const uint64_t b = 0x7FF8000000000000ull;
  double x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

// the position of slot k in the ascending array slots[0 .. n_spawn - 1], -1 when it is not there
RX_FN int32_t rx_te_find(const int32_t* slots, int32_t n_spawn, int32_t k) {
  int32_t lo = 0, hi = n_spawn;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (slots[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo < n_spawn && slots[lo] == k ? lo : -1;
}

// draw 0: the kind of the slot whose stream starts at h0
RX_FN int rx_te_kind(uint64_t h0, double edit_frac, uint64_t F) {
  return rx_te_unit(h0) < edit_frac && F > 0 ? RX_TRACK_EVOLVE_EDIT : RX_TRACK_EVOLVE_FRESH;
}

RX_FN int32_t rx_te_fresh_points(uint64_t h0) { return 10 + (int32_t)rx_tc_mulhi64(rx_lg_splitmix64(h0), 5); }

RX_FN int32_t rx_te_parent(uint64_t h0, const int64_t* cdf_score, int32_t n_tracks, uint64_t F) {
  return rx_tc_search(cdf_score, n_tracks, rx_tc_mulhi64(rx_lg_splitmix64(h0), F));
}

// one plan row: (kind, parent or -1, P, 0)
RX_FN void rx_te_plan_row(const rx_track_evolve_io* ev, uint32_t g, double edit_frac, int32_t j) {
  const int32_t n = ev->n_tracks;
  const uint64_t F = (uint64_t)ev->cdf_score[n - 1];
  const uint64_t h0 = rx_te_stream(ev->seed, g, (uint32_t)ev->slots[j]);
  int32_t* row = ev->plan + (size_t)j * RX_TRACK_EVOLVE_W;
  if (rx_te_kind(h0, edit_frac, F) == RX_TRACK_EVOLVE_EDIT) {
    const int32_t parent = rx_te_parent(h0, ev->cdf_score, n, F);
    row[0] = RX_TRACK_EVOLVE_EDIT;
    row[1] = parent;
    row[2] = ev->cp_off[parent + 1] - ev->cp_off[parent];
  } else {
    row[0] = RX_TRACK_EVOLVE_FRESH;
    row[1] = -1;
    row[2] = rx_te_fresh_points(h0);
  }
  row[3] = 0;
}

// a fresh track of P points into out[P][2]; h0: the slot's stream (P was drawn from it by rx_te_fresh_points)
RX_FN double rx_te_fresh(uint64_t h0, int32_t P, double* out) {
  uint64_t h = rx_lg_splitmix64(rx_lg_splitmix64(h0));  // past the kind and P
  const int32_t base = 50 + (int32_t)rx_tc_mulhi64(h, 30);
  h = rx_lg_splitmix64(h);
  const int32_t var = 10 + (int32_t)rx_tc_mulhi64(h, (uint64_t)(base / 2 - 20));
  h = rx_lg_splitmix64(h);
  const double jitter = 0.2 + 0.5 * rx_te_unit(h);
  h = rx_lg_splitmix64(h);
  const double smooth = 0.2 + 0.5 * rx_te_unit(h);
  h = rx_lg_splitmix64(h);
  const double width = (double)(6 + (int32_t)rx_tc_mulhi64(h, 4));
  uint64_t ha = h;                                  // the P offsets follow ...
  uint64_t hr = h;                                  // ... and the P radii follow them
  for (int32_t i = 0; i < P; ++i) hr = rx_lg_splitmix64(hr);
  const double spacing = RX_TRACK_EVOLVE_TWO_PI / (double)P;
  const double half = (jitter * spacing) / 2.0;
  const double span = 2.0 * half;
  const double b = (double)base, lo = -(double)var, wide = 2.0 * (double)var;
  const double keep = 1.0 - smooth;
  double r0 = 0.0, a0 = 0.0, r = 0.0;
  for (int32_t i = 0; i < P; ++i) {
    ha = rx_lg_splitmix64(ha);
    hr = rx_lg_splitmix64(hr);
    const double angle = (double)i * spacing + (-half + span * rx_te_unit(ha));
    const double v = b + (lo + wide * rx_te_unit(hr));
    if (i == 0) {
      r = v;
      r0 = v;
      a0 = angle;
    } else {
      r = keep * v + smooth * r;
      double s, c;
      rx_sincos(angle, &s, &c);
      out[2 * i] = r * c;
      out[2 * i + 1] = r * s;
    }
  }
  r0 = (r0 + r) / 2.0;
  double s, c;
  rx_sincos(a0, &s, &c);
  out[0] = r0 * c;
  out[1] = r0 * s;
  return width;
}

RX_FN double rx_te_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

RX_FN double rx_te_chord2(double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  return dx * dx + dy * dy;
}

// an edited child of `parent` (P points, width w) into out[P][2] (no overlap); -> edits applied
RX_FN int32_t rx_te_edit(uint64_t h0, int32_t P, const double* parent, double w, double* out, double* width) {
  uint64_t h = rx_lg_splitmix64(rx_lg_splitmix64(h0));  // past the kind and the parent
  *width = rx_clip((w + (double)rx_tc_mulhi64(h, 3)) - 1.0, 6.0, 9.0);
  h = rx_lg_splitmix64(h);
  const int32_t n_edits = 1 + (int32_t)rx_tc_mulhi64(h, 3);
  for (int32_t i = 0; i < 2 * P; ++i) out[i] = parent[i];
  int32_t applied = 0;
  for (int32_t e = 0; e < n_edits; ++e) {
    h = rx_lg_splitmix64(h);
    const int32_t i = (int32_t)rx_tc_mulhi64(h, (uint64_t)P);
    h = rx_lg_splitmix64(h);
    const int angular = (int)(h >> 63);
    h = rx_lg_splitmix64(h);
    const int forward = (int)(h >> 63);
    h = rx_lg_splitmix64(h);
    const double u = rx_te_unit(h);
    const int32_t ip = i == 0 ? P - 1 : i - 1, in = i == P - 1 ? 0 : i + 1;
    const double x = out[2 * i], y = out[2 * i + 1];
    const double px = out[2 * ip], py = out[2 * ip + 1], nx = out[2 * in], ny = out[2 * in + 1];
    const double r = RX_SQRT(x * x + y * y);
    double qx, qy;
    if (angular) {
      const double t = 0.35 * u;
      const double bx = forward ? nx : px, by = forward ? ny : py;
      qx = x + t * (bx - x);
      qy = y + t * (by - y);
      const double f = r / RX_SQRT(qx * qx + qy * qy);
      qx = qx * f;
      qy = qy * f;
    } else {
      const double f = rx_clip(r * (0.8 + 0.4 * u), RX_TRACK_EVOLVE_R_MIN, RX_TRACK_EVOLVE_R_MAX) / r;
      qx = x * f;
      qy = y * f;
    }
    const int ok = (qx != x || qy != y) && rx_te_cross(px, py, qx, qy) > 0.0 && rx_te_cross(qx, qy, nx, ny) > 0.0 &&
                   rx_te_chord2(px, py, qx, qy) >= RX_TRACK_EVOLVE_CHORD2 &&
                   rx_te_chord2(qx, qy, nx, ny) >= RX_TRACK_EVOLVE_CHORD2;
    if (ok) {
      out[2 * i] = qx;
      out[2 * i + 1] = qy;
      applied += 1;
    }
  }
  return applied;
}

// slot k of the new pool: a copy, a fresh track or an edited child, by the plan
RX_FN void rx_te_slot(const rx_track_evolve_io* ev, uint32_t g, int32_t k) {
  const int32_t o_new = ev->cp_off_new[k], span = ev->cp_off_new[k + 1] - o_new;
  double* out = ev->cp_new + 2 * (size_t)o_new;
  const int32_t j = rx_te_find(ev->slots, ev->n_spawn, k);
  if (j < 0) {  // kept
    const int32_t o = ev->cp_off[k];
    if (ev->cp_off[k + 1] - o != span) {
      ev->width_new[k] = rx_te_nan();
      return;
    }
    const double* in = ev->cp + 2 * (size_t)o;
    for (int32_t i = 0; i < 2 * span; ++i) out[i] = in[i];
    ev->width_new[k] = ev->width[k];
    return;
  }
  int32_t* row = ev->plan + (size_t)j * RX_TRACK_EVOLVE_W;
  const uint64_t h0 = rx_te_stream(ev->seed, g, (uint32_t)k);
  if (row[0] == RX_TRACK_EVOLVE_EDIT) {
    const int32_t parent = row[1];
    if (parent < 0 || parent >= ev->n_tracks || ev->cp_off[parent + 1] - ev->cp_off[parent] != span || span < 1) {
      ev->width_new[k] = rx_te_nan();
      return;
    }
    double w;
    row[3] = rx_te_edit(h0, span, ev->cp + 2 * (size_t)ev->cp_off[parent], ev->width[parent], out, &w);
    ev->width_new[k] = w;
  } else {
    if (rx_te_fresh_points(h0) != span) {
      ev->width_new[k] = rx_te_nan();
      return;
    }
    ev->width_new[k] = rx_te_fresh(h0, span, out);
    row[3] = 0;
  }
}

// ---- in place: the class table, the staging buffer, the commit ------------------------------------------

#define RX_TRACK_EVOLVE_BINS (RX_TRACK_MAX_P + 2)  // bin P for 1 <= P <= RX_TRACK_MAX_P, the last bin for no class

// the bin of a point count: P itself, or the bin behind the last class
RX_FN int32_t rx_te_bin(int32_t P) { return P >= 1 && P <= RX_TRACK_MAX_P ? P : RX_TRACK_MAX_P + 1; }

RX_FN int32_t rx_te_points(const int32_t* cp_off, int32_t k) { return cp_off[k + 1] - cp_off[k]; }

// w_k of the rank table, 0 for a slot of no class
RX_FN uint64_t rx_te_class_weight(const int64_t* cdf_score, int32_t k, int32_t bin) {
  if (bin > RX_TRACK_MAX_P) return 0;
  return (uint64_t)cdf_score[k] - (k ? (uint64_t)cdf_score[k - 1] : 0ull);
}

// whether spawned slot j has a place to be written to: its slot in the pool, a point count
// of a class, a staging span of that many points
RX_FN int rx_te_inplace_ok(const rx_track_evolve_inplace_io* ev, int32_t j, int32_t* k_out, int32_t* P_out) {
  const int32_t k = ev->slots[j];
  *k_out = k;
  *P_out = 0;
  if (k < 0 || k >= ev->n_tracks) return 0;
  const int32_t P = rx_te_points(ev->cp_off, k);
  *P_out = P;
  return P >= 1 && P <= RX_TRACK_MAX_P && ev->out_off[j + 1] - ev->out_off[j] == P;
}

// spawned slot j: its plan row and its track in the staging buffer
RX_FN void rx_te_inplace_slot(const rx_track_evolve_inplace_io* ev, uint32_t g, double edit_frac, int32_t j) {
  int32_t* row = ev->plan + (size_t)j * RX_TRACK_EVOLVE_W;
  int32_t k, P;
  row[0] = RX_TRACK_EVOLVE_FRESH;
  row[1] = -1;
  row[3] = 0;
  if (!rx_te_inplace_ok(ev, j, &k, &P)) {
    row[2] = P;
    ev->width_out[j] = rx_te_nan();
    return;
  }
  row[2] = P;
  double* out = ev->cp_out + 2 * (size_t)ev->out_off[j];
  const uint64_t h0 = rx_te_stream(ev->seed, g, (uint32_t)k);
  const int32_t lo = ev->class_end[P - 1], hi = ev->class_end[P];
  uint64_t base = 0, F = 0;
  if (lo >= 0 && lo < hi && hi <= ev->n_tracks) {  // (a table that was built for this pool always has k itself in here)
    base = lo ? (uint64_t)ev->cdf_class[lo - 1] : 0ull;
    F = (uint64_t)ev->cdf_class[hi - 1] - base;
  }
  if (rx_te_kind(h0, edit_frac, F) == RX_TRACK_EVOLVE_EDIT) {
    const uint64_t t = base + rx_tc_mulhi64(rx_lg_splitmix64(h0), F);
    const int32_t parent = ev->order[lo + rx_tc_search(ev->cdf_class + lo, hi - lo, t)];
    if (parent < 0 || parent >= ev->n_tracks || rx_te_points(ev->cp_off, parent) != P) {  // not this pool's table
      ev->width_out[j] = rx_te_nan();
      return;
    }
    double w;
    row[0] = RX_TRACK_EVOLVE_EDIT;
    row[1] = parent;
    row[3] = rx_te_edit(h0, P, ev->cp + 2 * (size_t)ev->cp_off[parent], ev->width[parent], out, &w);
    ev->width_out[j] = w;
  } else {
    ev->width_out[j] = rx_te_fresh(h0, P, out);
  }
}

// the commit of spawned slot j (whose slot is k), one point at a time
RX_FN void rx_te_commit_point(const rx_track_evolve_inplace_io* ev, int32_t j, int32_t k, int32_t i) {
  const size_t src = 2 * ((size_t)ev->out_off[j] + (size_t)i), dst = 2 * ((size_t)ev->cp_off[k] + (size_t)i);
  ev->cp[dst] = ev->cp_out[src];
  ev->cp[dst + 1] = ev->cp_out[src + 1];
}

RX_FN void rx_te_commit_slot(const rx_track_evolve_inplace_io* ev, int32_t j) {
  int32_t k, P;
  const int ok = rx_te_inplace_ok(ev, j, &k, &P);
  if (k < 0 || k >= ev->n_tracks) return;
  if (ok)
    for (int32_t i = 0; i < P; ++i) rx_te_commit_point(ev, j, k, i);
  ev->width[k] = ev->width_out[j];
}

// the class table, one slot after the other (the host twin; the kernel gives the same integers)
RX_FN void rx_te_classes_serial(const rx_track_evolve_inplace_io* ev) {
  int32_t start[RX_TRACK_EVOLVE_BINS + 1];
  for (int32_t b = 0; b <= RX_TRACK_EVOLVE_BINS; ++b) start[b] = 0;
  for (int32_t k = 0; k < ev->n_tracks; ++k) start[rx_te_bin(rx_te_points(ev->cp_off, k)) + 1] += 1;
  for (int32_t b = 1; b <= RX_TRACK_EVOLVE_BINS; ++b) start[b] += start[b - 1];  // start[b]: the slots of bins < b
  for (int32_t p = 0; p <= RX_TRACK_MAX_P; ++p) ev->class_end[p] = start[p + 1];
  for (int32_t k = 0; k < ev->n_tracks; ++k) {
    const int32_t b = rx_te_bin(rx_te_points(ev->cp_off, k));
    const int32_t pos = start[b]++;
    ev->order[pos] = k;
    ev->cdf_class[pos] = (int64_t)rx_te_class_weight(ev->cdf_score, k, b);
  }
  uint64_t run = 0;
  for (int32_t i = 0; i < ev->n_tracks; ++i) {
    run += (uint64_t)ev->cdf_class[i];
    ev->cdf_class[i] = (int64_t)run;
  }
}
