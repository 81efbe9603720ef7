// rx_track.hip -- the track table built on the device (rx_build_tracks, ABI v24).
//
// k_build_tracks: one wavefront per track, kTrackWaves tracks per workgroup.
// The geometry is rx_spline.h, the same inline functions the host twin
// (rx_build_tracks_host) runs, compiled here for gfx950 under
// -ffp-contract=off: same operations, same order, same bits.
//
//   lanes < P   stage the control points into the wave's LDS workspace
//   lane 0      chords, knot parameters (a serial running sum, np.cumsum's order)
//   lanes 0, 1  the cyclic tridiagonal solve of x and of y (Sherman-Morrison
//               over Thomas sweeps, P <= 64 unknowns, sweeps in LDS)
//   lanes < P   power-basis coefficients of interval `lane`
//   all lanes   stride over the W = P * factor waypoints: lane j evaluates
//               waypoints j, j+1 and j+2 (re-evaluation gives the same bits as
//               the neighbour lane's value, so no LDS copy of the waypoints and
//               no fence) and stores rows j of wp / nrm and rows j, W + j of
//               seg -- 16 B and 32 B per lane, consecutive lanes consecutive
//               rows; the tail pass is masked by j < W
//   wave        min / max of the waypoints by xor-shuffles (exact in any
//               order), then lane 0 writes the meta row
//
// 96 B stored per waypoint against ~60 flops: store-bound.  The workspace is
// 10,256 B per wave, 41 KB per workgroup of 4 waves.
#include <hip/hip_runtime.h>

#include "rx_internal.h"
#include "rx_spline.h"

namespace {

constexpr int kTrackWaves = 4;

__global__ __launch_bounds__(64 * kTrackWaves) void k_build_tracks(int n_tracks, int factor,
                                                                    const int32_t* __restrict__ cp_off,
                                                                    const double* __restrict__ cp,
                                                                    const double* __restrict__ width,
                                                                    double* __restrict__ wp, double* __restrict__ nrm,
                                                                    double* __restrict__ seg,
                                                                    double* __restrict__ meta) {
  __shared__ rx_spline_ws ws_all[kTrackWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * kTrackWaves + wave;
  // the last workgroup's spare waves keep arriving at the barriers and do nothing else
  const bool live = k < n_tracks;
  rx_spline_ws* ws = &ws_all[wave];
  int P = 0, W = 0;
  int64_t base = 0;  // first waypoint row of the track = cp_off[k] * factor
  const double* c = cp;
  if (live) {
    const int c0 = cp_off[k];
    P = cp_off[k + 1] - c0;
    W = P * factor;
    base = (int64_t)c0 * factor;
    c = cp + 2 * (int64_t)c0;
    if (lane < P) rx_spline_load(lane, c, ws);
  }
  __syncthreads();
  if (live && lane == 0) rx_spline_knots(P, W, ws);
  __syncthreads();
  if (live && lane < 2) rx_spline_solve(P, lane, ws);
  __syncthreads();
  if (live && lane < P) rx_spline_coef(P, lane, ws);
  __syncthreads();
  if (!live) return;

  const double w = width[k];
  double* wpk = wp + 2 * base;
  double* nrmk = nrm + 2 * base;
  double* segk = seg + 8 * base;  // 2 * base rows of 4
  double b[4] = {__builtin_inf(), -__builtin_inf(), __builtin_inf(), -__builtin_inf()};
  for (int j = lane; j < W; j += 64) {
    double x, y;
    rx_track_point(P, W, ws, w, j, wpk, nrmk, segk, &x, &y);
    rx_track_bounds(x, y, b);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const double x0 = __shfl_xor(b[0], m, 64), x1 = __shfl_xor(b[1], m, 64);
    const double y0 = __shfl_xor(b[2], m, 64), y1 = __shfl_xor(b[3], m, 64);
    b[0] = x0 < b[0] ? x0 : b[0];  // a lane without waypoints (W < 64) holds +-inf
    b[1] = x1 > b[1] ? x1 : b[1];
    b[2] = y0 < b[2] ? y0 : b[2];
    b[3] = y1 > b[3] ? y1 : b[3];
  }
  if (lane == 0) {
    double* mk = meta + 8 * (int64_t)k;
    double dy, dx;
    rx_track_meta(P, W, ws, w, b, mk, &dy, &dx);
    mk[2] = atan2(dy, dx);
    // Data the host cannot see before the launch (rx.h): a track that fails
    // rx_track_check gets max_track_distance = NaN, which rx_upload_tracks refuses.
    int where;
    if (rx_track_check(P, c, w, &where) != RX_TRACK_OK) mk[4] = __builtin_nan("");
  }
}

}  // namespace

extern "C" int rx_launch_build_tracks(int n_tracks, int factor, const int32_t* cp_off, const double* cp,
                                      const double* width, double* wp, double* nrm, double* seg, double* meta,
                                      hipStream_t s) {
  const int n_wg = (n_tracks + kTrackWaves - 1) / kTrackWaves;
  hipLaunchKernelGGL(k_build_tracks, dim3(n_wg), dim3(64 * kTrackWaves), 0, s, n_tracks, factor, cp_off, cp, width,
                     wp, nrm, seg, meta);
  return (int)hipGetLastError();
}
