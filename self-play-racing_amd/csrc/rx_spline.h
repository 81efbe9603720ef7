// rx_spline.h -- track geometry (environment/track.py:82-148) as one set of
// inline functions compiled twice: by hipcc for gfx950 (rx_track.hip, a
// wavefront per track) and for the host (rx_build_tracks_host in rx_api.cpp, a
// plain loop).  Every operation is a single IEEE-754 binary64 add / sub / mul /
// div / sqrt in a fixed order and both translation units are compiled with
// -ffp-contract=off, so the device table and the host table are the same bits
// (tests/test_track_build_gpu.py).  The one exception is atan2 (meta[2]): ocml
// on the device, libm on the host.
//
// Formulation (one track: control points cp[P][2], width w, factor f):
//  * closed polygon cp + cp[0]; chord_i = sqrt(dx*dx + dy*dy); t = running sum
//    of the chords (np.cumsum order); W = P*f samples tw_j = j * (t[P] / W)
//    (np.linspace(0, t[-1], W, endpoint=False));
//  * periodic cubic spline per coordinate: the knot first derivatives s solve
//    the cyclic tridiagonal system  h_i s_{i-1} + 2 (h_{i-1} + h_i) s_i +
//    h_{i-1} s_{i+1} = 3 (h_i slope_{i-1} + h_{i-1} slope_i)  (indices mod P)
//    by Sherman-Morrison over two Thomas sweeps (strictly diagonally dominant:
//    no pivoting); power-basis coefficients as scipy's CubicSpline forms them,
//    evaluated as scipy's PPoly does (c3 + c2 z + c1 z^2 + c0 z^3, the powers
//    by repeated multiplication) at z = tw_j - t_k, k the last knot <= tw_j;
//  * everything after the waypoints follows TrackGeometry.from_waypoints
//    (rx/track.py) operation for operation.
// scipy solves the same system through LAPACK, so waypoints agree with it to
// rounding only; the rest is an exact function of the waypoints.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RX_HD __host__ __device__ inline
#define RX_SPL_SQRT(x) __builtin_sqrt(x)
#else
#include <math.h>
#define RX_HD static inline
#define RX_SPL_SQRT(x) sqrt(x)
#endif

#define RX_TRACK_MAX_P 64  // control points per track: one per lane of a wavefront

// what rx_track_check found wrong with a track (0 = nothing)
#define RX_TRACK_OK 0
#define RX_TRACK_BAD_COORD 1  // a control-point coordinate is not finite
#define RX_TRACK_BAD_CHORD 2  // two consecutive control points coincide (or their distance overflows)
#define RX_TRACK_BAD_WIDTH 3  // width negative or NaN

// Per-track workspace: LDS on the device (one per wavefront), the stack on the host.
struct rx_spline_ws {
  double t[RX_TRACK_MAX_P + 1];   // knot parameters, t[0] = 0
  double c[2][4][RX_TRACK_MAX_P]; // [x|y][power 3..0 as scipy's c0..c3][interval]
  double h[RX_TRACK_MAX_P];       // chords
  double slope[2][RX_TRACK_MAX_P];
  double s[2][RX_TRACK_MAX_P];    // knot first derivatives
  double tmp[2][3][RX_TRACK_MAX_P];  // Thomas sweeps of the x and the y solve
  double step;                    // t[P] / W
};

RX_HD bool rx_spl_finite(double v) { return (v - v) == 0.0; }

// Data checks of one track; *where = index of the offending control point / chord.
RX_HD int rx_track_check(int P, const double* cp, double width, int* where) {
  *where = 0;
  for (int i = 0; i < P; ++i)
    if (!rx_spl_finite(cp[2 * i]) || !rx_spl_finite(cp[2 * i + 1])) {
      *where = i;
      return RX_TRACK_BAD_COORD;
    }
  for (int i = 0; i < P; ++i) {
    const int n = i + 1 == P ? 0 : i + 1;
    const double dx = cp[2 * n] - cp[2 * i], dy = cp[2 * n + 1] - cp[2 * i + 1];
    const double ch = RX_SPL_SQRT(dx * dx + dy * dy);
    if (!(ch > 0.0) || !rx_spl_finite(ch)) {
      *where = i;
      return RX_TRACK_BAD_CHORD;
    }
  }
  if (!(width >= 0.0)) return RX_TRACK_BAD_WIDTH;
  return RX_TRACK_OK;
}

// Control point i into the workspace (c[d][3] = y_k is also scipy's constant coefficient).
RX_HD void rx_spline_load(int i, const double* cp, rx_spline_ws* ws) {
  ws->c[0][3][i] = cp[2 * i];
  ws->c[1][3][i] = cp[2 * i + 1];
}

// Chords, knot parameters and the sample step (serial: the running sum is np.cumsum's).
RX_HD void rx_spline_knots(int P, int W, rx_spline_ws* ws) {
  const double* px = ws->c[0][3];
  const double* py = ws->c[1][3];
  double acc = 0.0;
  ws->t[0] = 0.0;
  for (int i = 0; i < P; ++i) {
    const int n = i + 1 == P ? 0 : i + 1;
    const double dx = px[n] - px[i], dy = py[n] - py[i];
    const double ch = RX_SPL_SQRT(dx * dx + dy * dy);
    ws->h[i] = ch;
    acc = acc + ch;
    ws->t[i + 1] = acc;
    ws->slope[0][i] = dx / ch;
    ws->slope[1][i] = dy / ch;
  }
  ws->step = acc / (double)W;
}

// Knot first derivatives of coordinate d (0 = x, 1 = y): the cyclic system above.
// With A = B + u v^T (B tridiagonal, u = (g, 0, .., 0, c_{P-1}), v = (1, 0, .., 0, a_0 / g),
// g = -b_0), s = y - z (v.y) / (1 + v.z) where B y = r and B z = u.
RX_HD void rx_spline_solve(int P, int d, rx_spline_ws* ws) {
  const double* h = ws->h;
  const double* sl = ws->slope[d];
  double* cpr = ws->tmp[d][0];  // modified super-diagonal
  double* y = ws->tmp[d][1];
  double* z = ws->tmp[d][2];
  const double b0 = 2.0 * (h[P - 1] + h[0]);
  const double g = -b0;
  const double alpha = h[P - 2];  // A[P-1][0]: row P-1's super-diagonal h_{P-2}
  const double beta = h[0];       // A[0][P-1]: row 0's sub-diagonal h_0
  // forward sweep
  double den = b0 - g;
  cpr[0] = h[P - 1] / den;
  y[0] = 3.0 * (h[0] * sl[P - 1] + h[P - 1] * sl[0]) / den;
  z[0] = g / den;
  for (int i = 1; i < P; ++i) {
    const double a = h[i];
    double b = 2.0 * (h[i - 1] + h[i]);
    if (i == P - 1) b = b - alpha * beta / g;
    const double r = 3.0 * (h[i] * sl[i - 1] + h[i - 1] * sl[i]);
    const double u = i == P - 1 ? alpha : 0.0;
    den = b - a * cpr[i - 1];
    cpr[i] = h[i - 1] / den;
    y[i] = (r - a * y[i - 1]) / den;
    z[i] = (u - a * z[i - 1]) / den;
  }
  // back substitution
  for (int i = P - 2; i >= 0; --i) {
    y[i] = y[i] - cpr[i] * y[i + 1];
    z[i] = z[i] - cpr[i] * z[i + 1];
  }
  const double fact = (y[0] + beta * y[P - 1] / g) / (1.0 + z[0] + beta * z[P - 1] / g);
  for (int i = 0; i < P; ++i) ws->s[d][i] = y[i] - fact * z[i];
}

// Power-basis coefficients of interval k (scipy CubicSpline.__init__), both coordinates;
// c[d][3][k] = y_k is already there (rx_spline_load).
RX_HD void rx_spline_coef(int P, int k, rx_spline_ws* ws) {
  const int n = k + 1 == P ? 0 : k + 1;
  const double hk = ws->h[k];
  for (int d = 0; d < 2; ++d) {
    const double sk = ws->s[d][k], sn = ws->s[d][n], m = ws->slope[d][k];
    const double T = (sk + sn - 2.0 * m) / hk;
    ws->c[d][0][k] = T / hk;
    ws->c[d][1][k] = (m - sk) / hk - T;
    ws->c[d][2][k] = sk;
  }
}

// Waypoint j (0 <= j < W).
RX_HD void rx_spline_eval(int P, const rx_spline_ws* ws, int j, double* x, double* y) {
  const double tw = (double)j * ws->step;
  int lo = 0, hi = P;  // invariant: t[lo] <= tw, and tw < t[hi] or hi == P
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ws->t[mid] <= tw) lo = mid; else hi = mid;
  }
  const double z1 = tw - ws->t[lo];
  const double z2 = z1 * z1;
  const double z3 = z2 * z1;
  double rx = ws->c[0][3][lo], ry = ws->c[1][3][lo];
  rx = rx + ws->c[0][2][lo] * z1;
  ry = ry + ws->c[1][2][lo] * z1;
  rx = rx + ws->c[0][1][lo] * z2;
  ry = ry + ws->c[1][1][lo] * z2;
  rx = rx + ws->c[0][0][lo] * z3;
  ry = ry + ws->c[1][0][lo] * z3;
  *x = rx;
  *y = ry;
}

// Unit normal of waypoint a towards b = next waypoint (calc_normals, track.py:117-124).
RX_HD void rx_track_normal(double ax, double ay, double bx, double by, double* nx, double* ny) {
  const double tx = bx - ax, ty = by - ay;
  double l = RX_SPL_SQRT(tx * tx + ty * ty);
  if (l == 0.0) l = 1.0;
  *nx = -(ty / l);
  *ny = tx / l;
}

// Rows j of wp / nrm and rows j (left) and W + j (right) of seg, all relative to the track's base.
RX_HD void rx_track_point(int P, int W, const rx_spline_ws* ws, double width, int j, double* wp, double* nrm,
                          double* seg, double* px, double* py) {
  const int j1 = j + 1 == W ? 0 : j + 1;
  const int j2 = j1 + 1 == W ? 0 : j1 + 1;
  double x0, y0, x1, y1, x2, y2, nx0, ny0, nx1, ny1;
  rx_spline_eval(P, ws, j, &x0, &y0);
  rx_spline_eval(P, ws, j1, &x1, &y1);
  rx_spline_eval(P, ws, j2, &x2, &y2);
  rx_track_normal(x0, y0, x1, y1, &nx0, &ny0);
  rx_track_normal(x1, y1, x2, y2, &nx1, &ny1);
  wp[2 * j] = x0;
  wp[2 * j + 1] = y0;
  nrm[2 * j] = nx0;
  nrm[2 * j + 1] = ny0;
  const double lx0 = x0 + nx0 * width, ly0 = y0 + ny0 * width;
  const double lx1 = x1 + nx1 * width, ly1 = y1 + ny1 * width;
  const double rx0 = x0 - nx0 * width, ry0 = y0 - ny0 * width;
  const double rx1 = x1 - nx1 * width, ry1 = y1 - ny1 * width;
  double* sl = seg + 4 * (size_t)j;
  double* sr = seg + 4 * ((size_t)W + j);
  sl[0] = lx0;
  sl[1] = ly0;
  sl[2] = lx1 - lx0;
  sl[3] = ly1 - ly0;
  sr[0] = rx0;
  sr[1] = ry0;
  sr[2] = rx1 - rx0;
  sr[3] = ry1 - ry0;
  *px = x0;
  *py = y0;
}

// Running bounds (np.min / np.max: exact in any order).
RX_HD void rx_track_bounds(double x, double y, double* b) {
  b[0] = x < b[0] ? x : b[0];
  b[1] = x > b[1] ? x : b[1];
  b[2] = y < b[2] ? y : b[2];
  b[3] = y > b[3] ? y : b[3];
}

// meta row except the start angle (meta[2]: the caller's atan2 of (y1 - y0, x1 - x0)).
RX_HD void rx_track_meta(int P, int W, const rx_spline_ws* ws, double width, const double* b, double* meta,
                         double* dy, double* dx) {
  double x0, y0, x1, y1, nx, ny;
  rx_spline_eval(P, ws, 0, &x0, &y0);
  rx_spline_eval(P, ws, 1, &x1, &y1);
  rx_track_normal(x0, y0, x1, y1, &nx, &ny);
  const double ex = b[1] - b[0], ey = b[3] - b[2];  // b = (min x, max x, min y, max y)
  meta[0] = x0;
  meta[1] = y0;
  meta[3] = width;
  meta[4] = RX_SPL_SQRT(ex * ex + ey * ey);
  meta[5] = nx;
  meta[6] = ny;
  meta[7] = 0.0;
  *dy = y1 - y0;
  *dx = x1 - x0;
}
