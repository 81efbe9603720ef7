// rx_cull.hip -- the culling tables of a device-resident track table
// (rx_build_cull_tables, rx_upload_tracks_device; include/rx.h).
//
// k_cull_tables: one wavefront per slot, kCullWaves slots per workgroup, no LDS
// and no barrier.  The rules are rx_cull.h, the same inline functions the host
// twin runs with (lane, n_lanes) = (0, 1).
//
//   pass 1  lanes stride over the slot's 2 W segment rows (32 B per lane,
//           consecutive lanes consecutive rows): seg_f (16 B stored per row), the
//           lane's share of the box of all end points and of the longest segment;
//           the wave combines them by xor-shuffles (min / max: exact in any order)
//   pass 2  the same rows again (the slot's 64 W bytes are L2-resident: at most
//           128 KB, typically 23 KB): the largest hypot distance from the box
//           centre, combined the same way -> slot_geo
//   pass 3  a lane per box: leaf boxes (G rows each), super boxes (their S * G
//           rows: equal to the union of the leaves, with no wait for another
//           lane's store), waypoint chunk and super-chunk boxes; f64 stored as
//           32 B per lane, the float tables as 5 x 16 B (block 0 + 4 quadrants)
//   lane 0  the slot's element of the four offset arrays and its 128-byte header
//
// The offsets come from the host (rx_api.cpp computes them from wp_off): `off`
// holds wp_off and the four box offset arrays back to back, n + 1 entries each.
// Reads 2 x 64 W + ~96 W bytes and stores ~(32 + 224 / G) W bytes per slot:
// bound by the table's bytes, like k_build_tracks.
//
// k_patch_slots (rx_patch_tracks): the same passes for a LIST of slots whose tracks
// are replaced in place, reading a small source table; see the kernel.
#include <hip/hip_runtime.h>

#include "rx_cull.h"
#include "rx_internal.h"

namespace {

constexpr int kCullWaves = 4;

__device__ __forceinline__ double wave_max(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = rx_cull_hi(v, __shfl_xor(v, m, 64));
  return v;
}

__global__ __launch_bounds__(64 * kCullWaves) void k_cull_tables(int n_tracks, int G, int SG,
                                                                  const int32_t* __restrict__ off,
                                                                  const double* __restrict__ wp,
                                                                  const double* __restrict__ seg,
                                                                  const double* __restrict__ meta, rx_cull_tables t,
                                                                  int64_t n_leaf, int64_t n_super) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * kCullWaves + wave;
  if (k >= n_tracks) return;  // whole waves leave: nothing below waits for another wave
  const size_t n1 = (size_t)n_tracks + 1;
  const int32_t wp0 = off[k], W = off[k + 1] - wp0;
  const double* s = seg + 8 * (int64_t)wp0;
  const double* w = wp + 2 * (int64_t)wp0;
  rx_cull_slot o = {0, 0, 0, 0, n_leaf, n_super, t.chunk_box, t.super_box, t.wchunk_box, t.wsuper_box,
                    t.chunk_box_f, t.super_box_f};
  double b[4], longest;
  rx_cull_extent(s, W, lane, 64, t.seg_f + 8 * (int64_t)wp0, b, &longest);
  double geo[4] = {0.0, 0.0, 0.0, 0.0};
  if (G > 0) {
    for (int m = 32; m >= 1; m >>= 1) {  // a lane without segments (2 W < 64) holds the empty box
      const double other[4] = {__shfl_xor(b[0], m, 64), __shfl_xor(b[1], m, 64), __shfl_xor(b[2], m, 64),
                               __shfl_xor(b[3], m, 64)};
      rx_cull_box_union(b, other);
    }
    longest = wave_max(longest);
    const double cx = 0.5 * (b[0] + b[2]), cy = 0.5 * (b[1] + b[3]);
    const double reach = wave_max(rx_cull_reach(s, W, lane, 64, cx, cy));
    rx_cull_geo(b, reach, longest, geo);
    o.chunk0 = off[n1 + k];
    o.super0 = SG > 0 ? off[2 * n1 + k] : 0;
    o.wchunk0 = off[3 * n1 + k];
    o.wsuper0 = off[4 * n1 + k];
    rx_cull_boxes(s, w, W, G, SG, lane, 64, &o);
  }
  if (lane != 0) return;
  if (G > 0) {
    const int last = k == n_tracks - 1;  // the slot that also owns the arrays' final entry
    for (int a = 0; a < 4; ++a) {
      int32_t* dst = a == 0 ? t.chunk_off : a == 1 ? t.super_off : a == 2 ? t.wchunk_off : t.wsuper_off;
      if (a == 1 && SG <= 0) continue;
      dst[k] = off[(a + 1) * n1 + k];
      if (last) dst[k + 1] = off[(a + 1) * n1 + k + 1];
    }
    for (int c = 0; c < 4; ++c) t.slot_geo[4 * (int64_t)k + c] = geo[c];
  }
  rx_cull_header((rx_slot_hdr*)t.slot_hdr + k, wp0, W, &o, geo, meta + 8 * (int64_t)k);
}

// k_patch_slots (rx_patch_tracks, rx_replace_tracks_device): a wavefront per LISTED
// slot writes a source track over that slot, at the offsets the slot already has
// (ps[j], computed by the host from wp_off).  Pass 1 also stores the wp / nrm / seg
// rows to the destination span; every pass reads the SOURCE rows, so no wave reads
// its own global stores back and no fence is needed.  The reductions are
// k_cull_tables' (the same lane strides and shuffles), so the bytes are its bytes.
// No offset entry is written.  t == nullptr-like (has_t == 0): the table rows only.
__global__ __launch_bounds__(64 * kCullWaves) void k_patch_slots(
    int n_upd, int G, int SG, const rx_patch_slot* __restrict__ ps, const double* __restrict__ src_wp,
    const double* __restrict__ src_nrm, const double* __restrict__ src_seg, const double* __restrict__ src_meta,
    double* __restrict__ wp, double* __restrict__ nrm, double* __restrict__ seg, double* __restrict__ meta, int has_t,
    rx_cull_tables t, int64_t n_leaf, int64_t n_super) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * kCullWaves + wave;
  if (j >= n_upd) return;  // whole waves leave: nothing below waits for another wave
  const rx_patch_slot d = ps[j];
  const int32_t k = d.slot, W = d.W;
  const double* s = src_seg + 8 * (int64_t)d.src0;
  const double* w = src_wp + 2 * (int64_t)d.src0;
  const double* m = src_meta + 8 * (int64_t)j;
  rx_cull_copy_rows<2>(w, wp + 2 * (int64_t)d.wp0, W, lane, 64);
  rx_cull_copy_rows<2>(src_nrm + 2 * (int64_t)d.src0, nrm + 2 * (int64_t)d.wp0, W, lane, 64);
  rx_cull_copy_rows<4>(s, seg + 8 * (int64_t)d.wp0, 2 * W, lane, 64);
  double geo[4] = {0.0, 0.0, 0.0, 0.0};
  rx_cull_slot o = {0, 0, 0, 0, n_leaf, n_super, t.chunk_box, t.super_box, t.wchunk_box, t.wsuper_box,
                    t.chunk_box_f, t.super_box_f};
  if (has_t) {
    double b[4], longest;
    rx_cull_extent(s, W, lane, 64, t.seg_f + 8 * (int64_t)d.wp0, b, &longest);
    if (G > 0) {
      for (int x = 32; x >= 1; x >>= 1) {
        const double other[4] = {__shfl_xor(b[0], x, 64), __shfl_xor(b[1], x, 64), __shfl_xor(b[2], x, 64),
                                 __shfl_xor(b[3], x, 64)};
        rx_cull_box_union(b, other);
      }
      longest = wave_max(longest);
      const double cx = 0.5 * (b[0] + b[2]), cy = 0.5 * (b[1] + b[3]);
      const double reach = wave_max(rx_cull_reach(s, W, lane, 64, cx, cy));
      rx_cull_geo(b, reach, longest, geo);
      o.chunk0 = d.chunk0;
      o.super0 = SG > 0 ? d.super0 : 0;
      o.wchunk0 = d.wchunk0;
      o.wsuper0 = d.wsuper0;
      rx_cull_boxes(s, w, W, G, SG, lane, 64, &o);
    }
  }
  if (lane != 0) return;
  for (int c = 0; c < 8; ++c) meta[8 * (int64_t)k + c] = m[c];
  if (!has_t) return;
  if (G > 0)
    for (int c = 0; c < 4; ++c) t.slot_geo[4 * (int64_t)k + c] = geo[c];
  rx_cull_header((rx_slot_hdr*)t.slot_hdr + k, d.wp0, W, &o, geo, m);
}

}  // namespace

extern "C" int rx_launch_patch_slots(int n_upd, int G, int SG, const rx_patch_slot* ps, const rx_track_patch* p,
                                     double* wp, double* nrm, double* seg, double* meta, const rx_cull_tables* t,
                                     int64_t n_leaf, int64_t n_super, hipStream_t s) {
  const int n_wg = (n_upd + kCullWaves - 1) / kCullWaves;
  const rx_cull_tables none = {};
  hipLaunchKernelGGL(k_patch_slots, dim3(n_wg), dim3(64 * kCullWaves), 0, s, n_upd, G, SG, ps, p->wp, p->nrm, p->seg,
                     p->meta, wp, nrm, seg, meta, t ? 1 : 0, t ? *t : none, n_leaf, n_super);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_cull_tables(int n_tracks, int G, int SG, const int32_t* off, const double* wp,
                                     const double* seg, const double* meta, const rx_cull_tables* t, int64_t n_leaf,
                                     int64_t n_super, hipStream_t s) {
  const int n_wg = (n_tracks + kCullWaves - 1) / kCullWaves;
  hipLaunchKernelGGL(k_cull_tables, dim3(n_wg), dim3(64 * kCullWaves), 0, s, n_tracks, G, SG, off, wp, seg, meta, *t,
                     n_leaf, n_super);
  return (int)hipGetLastError();
}
