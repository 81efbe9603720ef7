// rx_render.hip -- rgb_array rendering on the device (rx_raster_static / _trail /
// _frame, ABI v25 additive).  The pixel rules are rx_raster.h, the same inline
// functions the host twins in rx_api.cpp run: integer tests in doubled
// coordinates, so device and host give the same bytes.
//
// k_raster_static  once per track: a 16x16 pixel tile per block (a lane per
//                  pixel).  The track's ~4W edges come through LDS 256 at a
//                  time; the lane that stages an edge also tests it against
//                  the tile and marks it dead, so the pixel loop skips it with
//                  one broadcast LDS read.
// k_raster_trail   after each step: a block per image.  Car 0, barrier, car 1
//                  (the two cars set different bits of the same bytes).  Lanes
//                  stride over the clipped box of the new segment -- a few
//                  dozen pixels for a step of a car.
// k_raster_frame   per frame, the hot one: 3 B written per pixel against 2 B
//                  read.  A block belongs to one image; a lane owns 4
//                  consecutive pixels of a row at a time: one dword of classes,
//                  one of trail bits, 12 B out (one dwordx3 store when the rows
//                  are 4-byte aligned) -- a wave writes 768 consecutive bytes.
//                  The 4 colours come from byte selects (v_perm_b32) over a
//                  6-entry palette, with no branch.  Lanes 0..A-1 compute the
//                  image's car quads once per block into LDS (a sincos each);
//                  every wave then holds them in SGPRs (readfirstlane), and
//                  only lanes whose 4 pixels meet a car's box run the quad
//                  tests.  A block loops over kFrameIters = 8 groups per lane:
//                  with one group per lane the quad prologue and its barrier
//                  set the pace (measured on an MI355X, 200 x 800 x 800:
//                  0.67 ms at 1, 0.40 at 4, 0.36 at 8, 0.37 at 16 and 32 before
//                  the byte selects; 0.23 / 0.20 / 0.22 ms at 4 / 8 / 16 after).
#include <hip/hip_runtime.h>

#include "rx_internal.h"
#include "rx_raster.h"

namespace {

constexpr int kEdgeChunk = 256;
constexpr int kTile = RX_RASTER_TILE;
constexpr int kFrameIters = 8;  // 4-pixel groups per lane of k_raster_frame

__global__ __launch_bounds__(kTile * kTile) void k_raster_static(int size, int n_edges,
                                                                 const int32_t* __restrict__ edge_off,
                                                                 const int32_t* __restrict__ edges,
                                                                 uint8_t* __restrict__ layer) {
  __shared__ int32_t se[kEdgeChunk][RX_RASTER_EDGE_W];
  const int slot = blockIdx.z;
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
  const int i0 = blockIdx.x * kTile, j0 = blockIdx.y * kTile;
  const int i1 = min(i0 + kTile - 1, size - 1), j1 = min(j0 + kTile - 1, size - 1);
  const int i = i0 + tx, j = j0 + ty;
  const int e0 = min(max(edge_off[slot], 0), n_edges);
  const int e1 = min(max(edge_off[slot + 1], e0), n_edges);
  const int32_t sx = 2 * i + 1, sy = 2 * j + 1;
  uint32_t parity = 0;
  int32_t cls = RX_PX_BACKGROUND;
  for (int base = e0; base < e1; base += kEdgeChunk) {
    const int m = min(kEdgeChunk, e1 - base);
    __syncthreads();  // the previous chunk has been read
    if ((int)threadIdx.x < m) {
      const int32_t* e = edges + (int64_t)(base + threadIdx.x) * RX_RASTER_EDGE_W;
      int32_t v[RX_RASTER_EDGE_W];
      for (int c = 0; c < RX_RASTER_EDGE_W; ++c) v[c] = e[c];
      if (v[5] < 0) v[5] = 0;
      if (!rx_rs_edge_hits_tile(v, i0, j0, i1, j1)) v[5] = -1;  // dead for this tile
      for (int c = 0; c < RX_RASTER_EDGE_W; ++c) se[threadIdx.x][c] = v[c];
    }
    __syncthreads();
    for (int t = 0; t < m; ++t) {
      if (se[t][5] < 0) continue;
      rx_rs_edge_px(se[t], sx, sy, &parity, &cls);
    }
  }
  if (i < size && j < size) layer[((int64_t)slot * size + j) * size + i] = rx_rs_static_class(parity, cls);
}

__global__ __launch_bounds__(256) void k_raster_trail(rx_raster_io r) {
  const int k = blockIdx.x;
  const int S = r.size;
  const int e = r.env_ids[k];
  if (e < 0 || e >= r.n_envs) return;  // block-uniform
  const double scale = r.view[3 * k], ox = r.view[3 * k + 1], oy = r.view[3 * k + 2];
  uint8_t* tr = r.trail + (int64_t)k * S * S;
  for (int q = 0; q < r.A; ++q) {
    int32_t* last = r.last + ((int64_t)k * r.A + q) * 3;
    const int32_t px = last[0], py = last[1], had = last[2];
    const double x = r.x[(int64_t)e * r.A + q], y = r.y[(int64_t)e * r.A + q];
    int32_t X = 0, Y = 0;
    const bool ok = (x - x) == 0.0 && (y - y) == 0.0 && rx_rs_screen(x, y, scale, ox, oy, S, &X, &Y);
    int32_t i0, j0, i1, j1;
    if (ok && had && rx_rs_trail_box(px, py, X, Y, S, &i0, &j0, &i1, &j1)) {
      const uint8_t bit = q == 0 ? RX_PX_TRAIL0 : RX_PX_TRAIL1;
      const int bw = i1 - i0 + 1, n = bw * (j1 - j0 + 1);
      for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int i = i0 + t % bw, j = j0 + t / bw;
        if (rx_rs_capsule(2 * px, 2 * py, 2 * X, 2 * Y, 2 * i + 1, 2 * j + 1, RX_RASTER_TRAIL_W))
          tr[(int64_t)j * S + i] |= bit;
      }
    }
    __syncthreads();  // every lane has read `last`; car 0's bytes are written before car 1 reads them
    if (ok && threadIdx.x == 0) {
      last[0] = X;
      last[1] = Y;
      last[2] = 1;
    }
  }
}

__device__ __forceinline__ int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(256) void k_raster_frame(rx_raster_io r, int G, uint32_t G_inv, int iters) {
  __shared__ rx_car_quad sq[2];
  const int k = blockIdx.y;
  const int S = r.size;
  const int e = r.env_ids[k];
  if ((int)threadIdx.x < r.A) {
    rx_car_quad q = {};
    if (e >= 0 && e < r.n_envs) {
      const int64_t c = (int64_t)e * r.A + threadIdx.x;
      rx_rs_car(r.x[c], r.y[c], r.angle[c], r.view[3 * k], r.view[3 * k + 1], r.view[3 * k + 2], S, &q);
    }
    sq[threadIdx.x] = q;
  }
  __syncthreads();
  const int sl = r.layer_of[k];
  const int64_t off = r.out_off[k];
  // block-uniform: an image that has no layer or does not fit the buffer is not written
  if (sl < 0 || sl >= r.n_layers || off < 0 || off + (int64_t)(S - 1) * r.out_pitch + 3 * (int64_t)S > r.out_size) return;
  rx_car_quad cars[2];
  for (int q = 0; q < 2; ++q) {
    const rx_car_quad& s = sq[q < r.A ? q : 0];
    cars[q].valid = q < r.A ? uni(s.valid) : 0;
    for (int c = 0; c < 4; ++c) {
      cars[q].c[c][0] = uni(s.c[c][0]);
      cars[q].c[c][1] = uni(s.c[c][1]);
    }
    cars[q].lo_x = uni(s.lo_x);
    cars[q].hi_x = uni(s.hi_x);
    cars[q].lo_y = uni(s.lo_y);
    cars[q].hi_y = uni(s.hi_y);
  }
  const bool aligned_in = (S & 3) == 0 && ((uintptr_t)r.layer & 3) == 0 && ((uintptr_t)r.trail & 3) == 0;
  const bool aligned = (((uintptr_t)r.out + (uint64_t)off) & 3) == 0 && (r.out_pitch & 3) == 0;  // block-uniform
  for (int it = 0; it < iters; ++it) {
    const int g = (blockIdx.x * iters + it) * (int)blockDim.x + threadIdx.x;
    const int j = (int)__umulhi((uint32_t)g, G_inv), i0 = 4 * (g - j * G);  // j = g / G
    if (j >= S) break;
    const int n = min(4, S - i0);  // the row tail when S % 4 != 0
    const uint8_t* lp = r.layer + ((int64_t)sl * S + j) * S + i0;
    const uint8_t* tp = r.trail + ((int64_t)k * S + j) * S + i0;
    uint32_t cw = 0, tw = 0;
    if (aligned_in) {
      cw = *reinterpret_cast<const uint32_t*>(lp);
      tw = *reinterpret_cast<const uint32_t*>(tp);
    } else {
      for (int p = 0; p < n; ++p) {
        cw |= (uint32_t)lp[p] << (8 * p);
        tw |= (uint32_t)tp[p] << (8 * p);
      }
    }
    uint32_t o[3];
    rx_rs_group(cw, tw, cars, i0, j, o);
    uint8_t* op = r.out + off + (int64_t)j * r.out_pitch + 3 * (int64_t)i0;
    if (aligned && n == 4) {
      uint32_t* w = reinterpret_cast<uint32_t*>(op);  // 12 i0 bytes into a 4-byte aligned row
      w[0] = o[0];
      w[1] = o[1];
      w[2] = o[2];
    } else {
      for (int b = 0; b < 3 * n; ++b) op[b] = o[b >> 2] >> (8 * (b & 3)) & 0xff;
    }
  }
}

}  // namespace

extern "C" int rx_launch_raster_static(int n, int size, int n_edges, const int32_t* edge_off, const int32_t* edges,
                                       uint8_t* layer, hipStream_t s) {
  const int t = (size + kTile - 1) / kTile;
  hipLaunchKernelGGL(k_raster_static, dim3(t, t, n), dim3(kTile * kTile), 0, s, size, n_edges, edge_off, edges, layer);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_raster_trail(const rx_raster_io* r, hipStream_t s) {
  hipLaunchKernelGGL(k_raster_trail, dim3(r->K), dim3(256), 0, s, *r);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_raster_frame(const rx_raster_io* r, hipStream_t s) {
  const int G = (r->size + 3) / 4;
  // floor(g / G) = (g * ceil(2^32 / G)) >> 32, exact while g * G < 2^32: g < 2^20 and G <= 512 here
  const uint32_t G_inv = (uint32_t)(((1ull << 32) + G - 1) / G);
  const int64_t groups = (int64_t)G * r->size;
  const int iters = kFrameIters;
  const int64_t per_block = 256 * (int64_t)iters;
  hipLaunchKernelGGL(k_raster_frame, dim3((unsigned)((groups + per_block - 1) / per_block), r->K), dim3(256), 0, s, *r, G,
                     G_inv, iters);
  return (int)hipGetLastError();
}
