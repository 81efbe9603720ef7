// rx_track_evolve.hip -- track evolution on the device (ABI v25 additive; rules in
// rx_track_evolve.h, DESIGN.md §4 "Track evolution"):
//   k_track_evolve_plan  once per resample, a lane per spawned slot: the kind, the
//                        parent and the point count of what will fill it;
//   k_track_evolve       once per resample, a lane per slot of the pool: a kept slot
//                        copies its points and width from the old buffer to its place
//                        in the new one, a spawned slot writes a fresh track or an
//                        edited child there.
// A lane per slot, not a wave: the work of a spawned slot is serial (the radius
// recurrence, edits that build on each other) and a few hundred flops, and a kept
// slot moves at most 64 points.  Every lane works in global memory on its own span of
// the new buffer: no private arrays, no LDS, no atomics.  Arguments are checked by
// rx_api.cpp.
#include <hip/hip_runtime.h>

#include "rx.h"
#include "rx_track_evolve.h"

namespace {

constexpr int kEvolveThreads = 64;  // one wave: the spawned lanes of a pool spread over as many CUs as it has waves

__global__ __launch_bounds__(kEvolveThreads) void k_track_evolve_plan(const rx_track_evolve_io ev, uint32_t generation,
                                                                      double edit_frac) {
  const int64_t j = (int64_t)blockIdx.x * kEvolveThreads + threadIdx.x;
  if (j >= ev.n_spawn) return;
  rx_te_plan_row(&ev, generation, edit_frac, (int32_t)j);
}

__global__ __launch_bounds__(kEvolveThreads) void k_track_evolve(const rx_track_evolve_io ev, uint32_t generation) {
  const int64_t k = (int64_t)blockIdx.x * kEvolveThreads + threadIdx.x;
  if (k >= ev.n_tracks) return;
  rx_te_slot(&ev, generation, (int32_t)k);
}

}  // namespace

extern "C" int rx_launch_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac,
                                           hipStream_t s) {
  hipLaunchKernelGGL(k_track_evolve_plan, dim3((unsigned)((ev->n_spawn + kEvolveThreads - 1) / kEvolveThreads)),
                     dim3(kEvolveThreads), 0, s, *ev, generation, edit_frac);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_evolve(const rx_track_evolve_io* ev, uint32_t generation, hipStream_t s) {
  hipLaunchKernelGGL(k_track_evolve, dim3((unsigned)((ev->n_tracks + kEvolveThreads - 1) / kEvolveThreads)),
                     dim3(kEvolveThreads), 0, s, *ev, generation);
  return (int)hipGetLastError();
}
