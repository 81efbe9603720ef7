// rx_league.hip -- league training's two small kernels (ABI v25 additive; rules
// in rx_league.h, DESIGN.md §4 "League training"):
//   k_league_weights  tallies -> sampling table, one wave, one lane per slot;
//   k_league_draw     tally the envs whose episode ended, then redraw their
//                     opponent ids; one lane per env.
// The per-step policy launch of rx_league_rollout_steps (k_league_act) lives in
// rx_ppo.hip beside k_selfplay_act.  Arguments are checked by rx_api.cpp.
#include <hip/hip_runtime.h>

#include "rx.h"
#include "rx_league.h"

namespace {

// Lane k computes f_k into LDS; every lane then runs rx_lg_cdf's two serial loops
// over the LDS row -- the order of the sums is the slot order whatever the launch.
__global__ __launch_bounds__(64) void k_league_weights(const int64_t* __restrict__ tally, double* __restrict__ cdf,
                                                       int n_slots, int n_live, int power, double mix, double prior) {
  __shared__ double f[RX_LEAGUE_MAX_SLOTS];
  const int k = (int)threadIdx.x;
  f[k] = k < n_live ? rx_lg_priority(tally + (size_t)k * RX_LEAGUE_TALLY_W, power, prior) : 0.0;
  __syncthreads();
  if (k < n_slots) cdf[k] = rx_lg_cdf(f, n_live, mix, k);
}

struct league_draw_args {
  int32_t* opp_id;
  int32_t* draw_count;
  int64_t* tally;
  const double* cdf;
  const float* done;   // [n], or nullptr = redraw every env, tally nothing
  const double* info;  // [n][2][RX_INFO_W] (with done)
  uint64_t seed;
  int64_t n;
  int32_t n_slots;
  int32_t agent;
};

__global__ __launch_bounds__(256) void k_league_draw(league_draw_args a) {
  __shared__ double cdf[RX_LEAGUE_MAX_SLOTS];
  if ((int)threadIdx.x < a.n_slots) cdf[threadIdx.x] = a.cdf[threadIdx.x];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  if (a.done) {
    if (a.done[e] == 0.0f) return;
    const int32_t k = a.opp_id[e];
    if (k >= 0 && k < a.n_slots) {  // an id outside the bank is not counted (and is replaced below)
      unsigned long long* row = reinterpret_cast<unsigned long long*>(a.tally + (size_t)k * RX_LEAGUE_TALLY_W);
      const int out = rx_lg_outcome(a.info + (size_t)e * 2 * RX_INFO_W, a.agent);
      atomicAdd(row, 1ull);
      if (out & 1) atomicAdd(row + 1, 1ull);
      if (out & 2) atomicAdd(row + 2, 1ull);
    }
  }
  const uint32_t count = (uint32_t)a.draw_count[e];
  a.opp_id[e] = rx_lg_pick(cdf, a.n_slots, rx_lg_uniform(a.seed, count, (uint32_t)e));
  a.draw_count[e] = (int32_t)(count + 1u);
}

}  // namespace

extern "C" int rx_launch_league_weights(const rx_league_io* lg, int n_live, int power, double mix, double prior,
                                        hipStream_t s) {
  hipLaunchKernelGGL(k_league_weights, dim3(1), dim3(64), 0, s, lg->tally, lg->cdf, lg->n_slots, n_live, power, mix,
                     prior);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info,
                                     hipStream_t s) {
  const league_draw_args a{lg->opp_id, lg->draw_count, lg->tally, lg->cdf, done, info, lg->seed, n, lg->n_slots,
                           lg->agent};
  hipLaunchKernelGGL(k_league_draw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
