// rx_raster_host.cpp -- the host twins of the renderer's kernels
// (rx_raster_*_host, ABI v25 additive): the loops of rx_render.hip one pixel at
// a time over the same rx_raster.h functions.  Compiled as plain C++ (not as
// HIP), so rx_math.h and rx_raster.h take their host form; rx_api_tracks.cpp checks
// the arguments before it calls in here.  No HIP call.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rx.h"
#include "rx_raster.h"

extern "C" void rx_host_raster_static(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off,
                                      const int32_t* edges, uint8_t* layer) {
  std::vector<int32_t> live;
  for (int32_t slot = 0; slot < n; ++slot) {
    const int e0 = std::min(std::max(edge_off[slot], 0), n_edges);
    const int e1 = std::min(std::max(edge_off[slot + 1], e0), n_edges);
    for (int j0 = 0; j0 < size; j0 += RX_RASTER_TILE)
      for (int i0 = 0; i0 < size; i0 += RX_RASTER_TILE) {
        const int i1 = std::min(i0 + RX_RASTER_TILE, size) - 1, j1 = std::min(j0 + RX_RASTER_TILE, size) - 1;
        live.clear();
        for (int t = e0; t < e1; ++t) {
          int32_t v[RX_RASTER_EDGE_W];
          std::memcpy(v, edges + (size_t)t * RX_RASTER_EDGE_W, sizeof v);
          if (v[5] < 0) v[5] = 0;
          if (rx_rs_edge_hits_tile(v, i0, j0, i1, j1)) live.insert(live.end(), v, v + RX_RASTER_EDGE_W);
        }
        for (int j = j0; j <= j1; ++j)
          for (int i = i0; i <= i1; ++i) {
            uint32_t parity = 0;
            int32_t cls = RX_PX_BACKGROUND;
            for (size_t t = 0; t < live.size(); t += RX_RASTER_EDGE_W)
              rx_rs_edge_px(&live[t], 2 * i + 1, 2 * j + 1, &parity, &cls);
            layer[((size_t)slot * size + j) * size + i] = rx_rs_static_class(parity, cls);
          }
      }
  }
}

extern "C" void rx_host_raster_trail(const rx_raster_io* r) {
  const int S = r->size;
  for (int k = 0; k < r->K; ++k) {
    const int e = r->env_ids[k];
    if (e < 0 || e >= r->n_envs) continue;
    uint8_t* tr = r->trail + (size_t)k * S * S;
    for (int q = 0; q < r->A; ++q) {
      int32_t* last = r->last + ((size_t)k * r->A + q) * 3;
      const double x = r->x[(size_t)e * r->A + q], y = r->y[(size_t)e * r->A + q];
      int32_t X = 0, Y = 0;
      if (!((x - x) == 0.0 && (y - y) == 0.0 &&
            rx_rs_screen(x, y, r->view[3 * k], r->view[3 * k + 1], r->view[3 * k + 2], S, &X, &Y)))
        continue;
      int32_t i0, j0, i1, j1;
      if (last[2] && rx_rs_trail_box(last[0], last[1], X, Y, S, &i0, &j0, &i1, &j1)) {
        const uint8_t bit = q == 0 ? RX_PX_TRAIL0 : RX_PX_TRAIL1;
        for (int j = j0; j <= j1; ++j)
          for (int i = i0; i <= i1; ++i)
            if (rx_rs_capsule(2 * last[0], 2 * last[1], 2 * X, 2 * Y, 2 * i + 1, 2 * j + 1, RX_RASTER_TRAIL_W))
              tr[(size_t)j * S + i] |= bit;
      }
      last[0] = X;
      last[1] = Y;
      last[2] = 1;
    }
  }
}

extern "C" void rx_host_raster_frame(const rx_raster_io* r) {
  const int S = r->size;
  for (int k = 0; k < r->K; ++k) {
    const int e = r->env_ids[k], sl = r->layer_of[k];
    const int64_t off = r->out_off[k];
    if (sl < 0 || sl >= r->n_layers || off < 0 || off + (int64_t)(S - 1) * r->out_pitch + 3 * (int64_t)S > r->out_size)
      continue;
    rx_car_quad cars[2] = {};
    if (e >= 0 && e < r->n_envs)
      for (int q = 0; q < r->A; ++q) {
        const size_t c = (size_t)e * r->A + q;
        rx_rs_car(r->x[c], r->y[c], r->angle[c], r->view[3 * k], r->view[3 * k + 1], r->view[3 * k + 2], S, &cars[q]);
      }
    for (int j = 0; j < S; ++j) {
      const uint8_t* lp = r->layer + ((size_t)sl * S + j) * S;
      const uint8_t* tp = r->trail + ((size_t)k * S + j) * S;
      uint8_t* op = r->out + off + (int64_t)j * r->out_pitch;
      for (int i0 = 0; i0 < S; i0 += 4) {  // a lane of k_raster_frame
        const int n = std::min(4, S - i0);
        uint32_t cw = 0, tw = 0, o[3];
        for (int p = 0; p < n; ++p) {
          cw |= (uint32_t)lp[i0 + p] << (8 * p);
          tw |= (uint32_t)tp[i0 + p] << (8 * p);
        }
        rx_rs_group(cw, tw, cars, i0, j, o);
        for (int b = 0; b < 3 * n; ++b) op[3 * i0 + b] = o[b >> 2] >> (8 * (b & 3)) & 0xff;
      }
    }
  }
}
