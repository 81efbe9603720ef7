// rx_track_evolve.hip -- track evolution on the device (ABI v25 additive; rules in
// rx_track_evolve.h, DESIGN.md §4 "Track evolution"):
//   k_track_evolve_plan  once per resample, a lane per spawned slot: the kind, the
//                        parent and the point count of what will fill it;
//   k_track_evolve       once per resample, a lane per slot of the pool: a kept slot
//                        copies its points and width from the old buffer to its place
//                        in the new one, a spawned slot writes a fresh track or an
//                        edited child there.
// and, for a pool whose slots keep their point counts (the in-place form):
//   k_track_evolve_classes  once per resample, ONE workgroup: the rank table regrouped
//                           by point count (a stable counting sort and a 64-bit scan);
//   k_track_evolve_inplace  a lane per spawned slot: the plan row and the track, into
//                           a compact staging buffer;
//   k_track_evolve_commit   a wave per spawned slot: the staging rows over the pool.
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

// ---- in place -------------------------------------------------------------------------------------------

constexpr int kClassThreads = 1024;  // slots per pass, a lane each
constexpr int kClassWaves = kClassThreads / 64;
constexpr int kBins = RX_TRACK_EVOLVE_BINS;  // bin P for a class, the last one for a slot of no class
static_assert(kBins <= kClassThreads && kClassWaves * kBins <= 2 * kClassThreads, "the bins are walked a lane each");

// ONE workgroup, three walks over the slots in passes of 1,024 (at 65,536 slots 64
// passes each; the table is a few hundred KB and the walks are bound by the barriers,
// not by memory):
//   1. the histogram of the point counts, LDS atomics on 66 bins (rx_te_bin keeps an
//      out-of-range P inside them), then its exclusive scan by one lane: where every
//      bin starts in `order`, and class_end;
//   2. the stable scatter.  Inside a wave the lanes of one bin find each other by
//      ballots (one round per distinct bin of the wave, five for a generated pool):
//      a lane's place among them is the count of lower lanes in the ballot.  The
//      waves' counts per bin meet in LDS; a lane adds the counts of the waves before
//      its own and the bin's cursor, which then moves on by the pass's total.  Lower
//      slots always land first: the sort is stable.  The slot goes to order[pos], its
//      weight to cdf_class[pos];
//   3. the inclusive scan of cdf_class in place, k_track_learn_tables' pattern: a wave
//      scan by shuffles, the wave totals through LDS, the carried total of the passes
//      before.
// Walk 3 reads what other lanes of this workgroup wrote to global memory in walk 2:
// the barrier between them orders it (one workgroup, one CU).
__global__ __launch_bounds__(kClassThreads) void k_track_evolve_classes(const rx_track_evolve_inplace_io ev) {
  __shared__ int32_t cursor[kBins];                     // walk 1: the histogram; walk 2: the next free place of a bin
  __shared__ int32_t wave_count[kClassWaves][kBins];    // walk 2: the slots of (wave, bin) in this pass
  __shared__ unsigned long long wave_total[kClassWaves];  // walk 3
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t n = ev.n_tracks;

  if (tid < kBins) cursor[tid] = 0;
  __syncthreads();
  for (int32_t base = 0; base < n; base += kClassThreads) {
    const int32_t k = base + tid;
    if (k < n) atomicAdd(&cursor[rx_te_bin(rx_te_points(ev.cp_off, k))], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int b = 0; b < kBins; ++b) {
      const int32_t c = cursor[b];
      cursor[b] = run;
      run += c;
      if (b <= RX_TRACK_MAX_P) ev.class_end[b] = run;  // bin 0 stays empty: class_end[0] = 0
    }
  }
  __syncthreads();

  for (int32_t base = 0; base < n; base += kClassThreads) {
    for (int i = tid; i < kClassWaves * kBins; i += kClassThreads) (&wave_count[0][0])[i] = 0;
    __syncthreads();
    const int32_t k = base + tid;
    const bool valid = k < n;
    const int32_t bin = valid ? rx_te_bin(rx_te_points(ev.cp_off, k)) : -1;
    int32_t place = 0;  // among the lanes of this wave with this bin
    unsigned long long todo = __ballot(valid);
    while (todo) {  // wave-uniform: every lane sees the same ballots
      const int leader = __ffsll((long long)todo) - 1;
      const int32_t b0 = __shfl(bin, leader, 64);
      const unsigned long long same = __ballot(valid && bin == b0);
      if (valid && bin == b0) place = (int32_t)__popcll(same & ((1ull << lane) - 1ull));
      if (lane == leader) wave_count[wave][b0] = (int32_t)__popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (valid) {
      int32_t pos = cursor[bin] + place;
      for (int w = 0; w < wave; ++w) pos += wave_count[w][bin];
      ev.order[pos] = k;
      ev.cdf_class[pos] = (int64_t)rx_te_class_weight(ev.cdf_score, k, bin);
    }
    __syncthreads();  // every lane has read the cursors
    if (tid < kBins) {
      int32_t total = 0;
      for (int w = 0; w < kClassWaves; ++w) total += wave_count[w][tid];
      cursor[tid] += total;
    }
    __syncthreads();  // the next pass clears wave_count and reads the cursors
  }
  __threadfence_block();
  __syncthreads();

  unsigned long long carry = 0;
  for (int32_t base = 0; base < n; base += kClassThreads) {
    const int32_t i = base + tid;
    unsigned long long w = i < n ? (unsigned long long)ev.cdf_class[i] : 0ull;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(w, o, 64);
      if (lane >= o) w += y;
    }
    if (lane == 63) wave_total[wave] = w;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int j = 0; j < kClassWaves; ++j) {
      const unsigned long long t = wave_total[j];
      if (j < wave) before += t;
      total += t;
    }
    if (i < n) ev.cdf_class[i] = (int64_t)(carry + before + w);
    carry += total;
    __syncthreads();  // the next pass overwrites wave_total
  }
}

// a lane per spawned slot, as k_track_evolve: the plan row and the track into the staging buffer
__global__ __launch_bounds__(kEvolveThreads) void k_track_evolve_inplace(const rx_track_evolve_inplace_io ev,
                                                                         uint32_t generation, double edit_frac) {
  const int64_t j = (int64_t)blockIdx.x * kEvolveThreads + threadIdx.x;
  if (j >= ev.n_spawn) return;
  rx_te_inplace_slot(&ev, generation, edit_frac, (int32_t)j);
}

// a wave per spawned slot, a lane per point (RX_TRACK_MAX_P = 64 of them at most); lane 0 the width
__global__ __launch_bounds__(kEvolveThreads) void k_track_evolve_commit(const rx_track_evolve_inplace_io ev) {
  static_assert(kEvolveThreads == RX_TRACK_MAX_P, "a lane per control point");
  const int32_t j = (int32_t)blockIdx.x, i = (int32_t)threadIdx.x;
  int32_t k, P;
  const int ok = rx_te_inplace_ok(&ev, j, &k, &P);
  if (k < 0 || k >= ev.n_tracks) return;
  if (ok && i < P) rx_te_commit_point(&ev, j, k, i);
  if (i == 0) ev.width[k] = ev.width_out[j];
}

}  // namespace

extern "C" int rx_launch_track_evolve_classes(const rx_track_evolve_inplace_io* ev, hipStream_t s) {
  hipLaunchKernelGGL(k_track_evolve_classes, dim3(1), dim3(kClassThreads), 0, s, *ev);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation,
                                              double edit_frac, hipStream_t s) {
  hipLaunchKernelGGL(k_track_evolve_inplace, dim3((unsigned)((ev->n_spawn + kEvolveThreads - 1) / kEvolveThreads)),
                     dim3(kEvolveThreads), 0, s, *ev, generation, edit_frac);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_evolve_commit(const rx_track_evolve_inplace_io* ev, hipStream_t s) {
  hipLaunchKernelGGL(k_track_evolve_commit, dim3((unsigned)ev->n_spawn), dim3(kEvolveThreads), 0, s, *ev);
  return (int)hipGetLastError();
}

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
