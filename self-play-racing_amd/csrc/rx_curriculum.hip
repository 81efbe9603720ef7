// rx_curriculum.hip -- the track curriculum's kernels (ABI v25 additive;
// rules in rx_curriculum.h and rx_track_duel.h, DESIGN.md §4 "Track curriculum"):
//   k_track_tally   once per rollout step, a lane per env: the envs whose episode
//                   ended are summed per track slot INSIDE the wave and one lane
//                   per slot issues the int64 atomic adds;
//   k_track_tally2  k_track_tally for two-car envs: the learner's car in the single-agent
//                   columns, the win columns beside them (rx_track_duel.h);
//   k_track_episode k_track_tally plus the episodic draw: an env that ended takes its
//                   next slot at once (rx_track_episode);
//   k_track_scores  once per resample, ONE workgroup: per-slot weight and the
//                   inclusive integer scan into cdf, RX_TRACK_SCORES_CHUNK slots
//                   per pass with the running total carried along; with the win columns
//                   it is rx_track_duel_scores' kernel too;
//   k_track_draw    once per resample, a lane per env: two hashes and a binary
//                   search over cdf in global memory.
// Arguments are checked by rx_api.cpp.
#include <hip/hip_runtime.h>

#include "rx.h"
#include "rx_curriculum.h"
#include "rx_track_duel.h"

namespace {

struct track_tally_args {
  const int32_t* track;
  int64_t* tally;
  const float* done;
  const uint8_t* terminated;
  const double* info;  // [n][RX_INFO_W]
  int64_t n;
  int32_t n_tracks;
};

// In steady state almost no env ends in a step: the wave ballots `done` and leaves.
// Early in training thousands of envs can end in one step on a handful of slots, and
// every adder on one row serialises in the L2 atomic unit, so the wave first folds
// its lanes per slot (the wave-uniform loop of k_league_act): a leader
// slot is read from the lowest pending lane, its lanes are balloted, the counts are
// popcounts against the finished / crashed ballots, progress_q is a butterfly sum
// over the wave, and ONE lane adds the non-zero columns.  Integer adds: the result
// does not depend on the order in which waves arrive.
__global__ __launch_bounds__(256) void k_track_tally(track_tally_args a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ended = e < a.n && a.done[e] != 0.0f;
  if (__ballot(ended) == 0ull) return;
  int32_t slot = -1;
  int out = 0;
  long long pq = 0;
  if (ended) {
    const int32_t k = a.track[e];
    if (k >= 0 && k < a.n_tracks) {  // a slot outside the table is not counted
      const double progress = a.info[(size_t)e * RX_INFO_W + RX_INFO_PROGRESS];
      slot = k;
      out = rx_tc_outcome(progress, a.terminated[e]);
      pq = (long long)rx_tc_progress_q(progress);
    }
  }
  const bool live = slot >= 0;
  unsigned long long todo = __ballot(live);
  const unsigned long long fin = __ballot(live && (out & 1)), crash = __ballot(live && (out & 2));
  const int lane = (int)(threadIdx.x & 63);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int32_t s = __builtin_amdgcn_readlane(slot, leader);  // wave-uniform: in [0, n_tracks)
    const bool mine = live && slot == s;
    const unsigned long long same = __ballot(mine);
    long long sum = mine ? pq : 0;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == leader) {
      unsigned long long* row = reinterpret_cast<unsigned long long*>(a.tally + (size_t)s * RX_TRACK_TALLY_W);
      const unsigned long long nf = (unsigned long long)__popcll(same & fin);
      const unsigned long long nc = (unsigned long long)__popcll(same & crash);
      atomicAdd(row, (unsigned long long)__popcll(same));
      if (nf) atomicAdd(row + 1, nf);
      if (nc) atomicAdd(row + 2, nc);
      if (sum) atomicAdd(row + 3, (unsigned long long)sum);
    }
    todo &= ~same;
  }
}

struct track_tally2_args {
  const int32_t* track;
  int64_t* tally;
  int64_t* duel;
  const float* done;
  const uint8_t* terminated;
  const double* info;  // [n][2][RX_INFO_W]
  int64_t n;
  int32_t n_tracks;
  int32_t agent;  // the learner's car, 0 or 1
};

// k_track_tally for two-car envs (rules: rx_track_duel.h): the same ballot of `done` and the
// same fold per slot inside the wave, with six counts -- the slot's lanes, and its popcounts
// against the finished / crashed / won / opponent-finished / timed-out ballots -- and two
// butterfly sums (the progress_q of either car).  ONE lane adds the non-zero columns: at
// most 8 no-return 64-bit adds per distinct slot per wave.  An ended env reads its two info
// rows and one terminated byte.  Integer adds only; no LDS.
__global__ __launch_bounds__(256) void k_track_tally2(track_tally2_args a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ended = e < a.n && a.done[e] != 0.0f;
  if (__ballot(ended) == 0ull) return;
  int32_t slot = -1;
  int out = 0;
  long long pqa = 0, pqo = 0;
  if (ended) {
    const int32_t k = a.track[e];
    if (k >= 0 && k < a.n_tracks) {  // a slot outside the table is not counted
      const double* row = a.info + (size_t)e * 2 * RX_INFO_W;
      const double* ra = row + a.agent * RX_INFO_W;
      const double* ro = row + (1 - a.agent) * RX_INFO_W;
      const double pa = ra[RX_INFO_PROGRESS], po = ro[RX_INFO_PROGRESS];
      slot = k;
      out = rx_td_outcome(pa, po, ra[RX_INFO_PLACEMENT], a.terminated[e]);
      pqa = (long long)rx_tc_progress_q(pa);
      pqo = (long long)rx_tc_progress_q(po);
    }
  }
  const bool live = slot >= 0;
  unsigned long long todo = __ballot(live);
  const unsigned long long fin = __ballot(live && (out & RX_TD_FINISHED)), crash = __ballot(live && (out & RX_TD_CRASHED));
  const unsigned long long won = __ballot(live && (out & RX_TD_WON)), ofin = __ballot(live && (out & RX_TD_OPP_FINISHED));
  const unsigned long long tout = __ballot(live && (out & RX_TD_TIMEOUT));
  const int lane = (int)(threadIdx.x & 63);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int32_t s = __builtin_amdgcn_readlane(slot, leader);  // wave-uniform: in [0, n_tracks)
    const bool mine = live && slot == s;
    const unsigned long long same = __ballot(mine);
    long long sa = mine ? pqa : 0, so = mine ? pqo : 0;
    for (int o = 32; o > 0; o >>= 1) {
      sa += __shfl_xor(sa, o, 64);
      so += __shfl_xor(so, o, 64);
    }
    if (lane == leader) {
      unsigned long long* row = reinterpret_cast<unsigned long long*>(a.tally + (size_t)s * RX_TRACK_TALLY_W);
      unsigned long long* drow = reinterpret_cast<unsigned long long*>(a.duel + (size_t)s * RX_TRACK_DUEL_W);
      const unsigned long long nf = (unsigned long long)__popcll(same & fin);
      const unsigned long long nc = (unsigned long long)__popcll(same & crash);
      const unsigned long long nw = (unsigned long long)__popcll(same & won);
      const unsigned long long no = (unsigned long long)__popcll(same & ofin);
      const unsigned long long nt = (unsigned long long)__popcll(same & tout);
      atomicAdd(row, (unsigned long long)__popcll(same));
      if (nf) atomicAdd(row + 1, nf);
      if (nc) atomicAdd(row + 2, nc);
      if (sa) atomicAdd(row + 3, (unsigned long long)sa);
      if (nw) atomicAdd(drow, nw);
      if (no) atomicAdd(drow + 1, no);
      if (so) atomicAdd(drow + 2, (unsigned long long)so);
      if (nt) atomicAdd(drow + 3, nt);
    }
    todo &= ~same;
  }
}

struct track_episode_args {
  rx_track_io tc;
  rx_track_episode_io ep;
  const float* done;
  const uint8_t* terminated;
  const double* info;  // [n][RX_INFO_W]
  int64_t n;
};

// k_track_tally plus the episodic draw (rx_curriculum.h): an env that ended is tallied on
// the slot it ran and then draws its next one into track[e] and pos_slot[env_pos[e]], which
// the step after this launch resets it from (next-step autoreset).  The ballot, the fold
// per slot inside the wave and the adders are k_track_tally's (rx_tc_wave_episode_tally, shared
// with k_track_learn_episode); every lane touches only its
// own env's track / draws / pos_slot entries (env_pos is a permutation), so the draw needs
// no atomics.  slot_out[e] is the slot env e was on, ended or not, written before the draw.
__global__ __launch_bounds__(256) void k_track_episode(track_episode_args a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e < a.n;
  const bool ended = in && a.done[e] != 0.0f;
  const bool any = __ballot(ended) != 0ull;
  int32_t k = -1;
  if (in && (ended || a.ep.slot_out)) k = a.tc.track[e];
  if (in && a.ep.slot_out) a.ep.slot_out[e] = k;
  if (!any) return;
  const bool live = rx_tc_wave_episode_tally(a.tc.tally, a.tc.n_tracks, ended, k, a.terminated, a.info, e);
  if (live) rx_tc_episode_draw(&a.tc, &a.ep, a.n, e);
}

constexpr int kScoreThreads = RX_TRACK_SCORES_CHUNK;
constexpr int kScoreWaves = kScoreThreads / 64;

// One workgroup; per pass lane i takes slot base + i: W_k, an inclusive wave scan by
// shuffles, the wave totals through LDS, and the running total of the passes before
// (every lane keeps its own copy: the same integer).
// duel: the self-play table's win columns (rx_track_duel_scores; the weight is rx_td_weight), or null.
__global__ __launch_bounds__(kScoreThreads) void k_track_scores(const int64_t* __restrict__ tally,
                                                                const int64_t* __restrict__ duel,
                                                                int64_t* __restrict__ cdf, double* __restrict__ p,
                                                                int n_tracks, int score, int power, double prior) {
  __shared__ unsigned long long wave_total[kScoreWaves];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  unsigned long long carry = 0;
  for (int base = 0; base < n_tracks; base += kScoreThreads) {
    const int k = base + (int)threadIdx.x;
    unsigned long long x = 0;
    if (k < n_tracks) {
      double pk;
      const int64_t* row = tally + (size_t)k * RX_TRACK_TALLY_W;
      x = duel ? rx_td_weight(row, duel + (size_t)k * RX_TRACK_DUEL_W, score, power, prior, &pk)
               : rx_tc_weight(row, score, power, prior, &pk);
      p[k] = pk;
    }
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int j = 0; j < kScoreWaves; ++j) {
      const unsigned long long t = wave_total[j];
      if (j < wave) before += t;
      total += t;
    }
    if (k < n_tracks) cdf[k] = (int64_t)(carry + before + x);
    carry += total;
    __syncthreads();  // the next pass overwrites wave_total
  }
}

__global__ __launch_bounds__(256) void k_track_draw(const int64_t* __restrict__ cdf, int32_t* __restrict__ track_of_env,
                                                    int64_t n, int32_t n_tracks, uint64_t seed, uint32_t generation,
                                                    double mix) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  track_of_env[e] = rx_tc_draw(cdf, n_tracks, seed, generation, (uint32_t)e, mix);
}

}  // namespace

extern "C" int rx_launch_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                                     const double* info, hipStream_t s) {
  const track_tally_args a{tc->track, tc->tally, done, terminated, info, n, tc->n_tracks};
  hipLaunchKernelGGL(k_track_tally, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n,
                                       const float* done, const uint8_t* terminated, const double* info,
                                       hipStream_t s) {
  const track_episode_args a{*tc, *ep, done, terminated, info, n};
  hipLaunchKernelGGL(k_track_episode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_scores(const rx_track_io* tc, int power, double prior, hipStream_t s) {
  hipLaunchKernelGGL(k_track_scores, dim3(1), dim3(kScoreThreads), 0, s, tc->tally, (const int64_t*)nullptr, tc->cdf,
                     tc->p, tc->n_tracks, tc->score, power, prior);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int power, double prior,
                                           hipStream_t s) {
  hipLaunchKernelGGL(k_track_scores, dim3(1), dim3(kScoreThreads), 0, s, tc->tally, (const int64_t*)td->duel, tc->cdf,
                     tc->p, tc->n_tracks, tc->score, power, prior);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                                      const uint8_t* terminated, const double* info, hipStream_t s) {
  const track_tally2_args a{tc->track, tc->tally, td->duel, done, terminated, info, n, tc->n_tracks, td->agent};
  hipLaunchKernelGGL(k_track_tally2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, hipStream_t s) {
  hipLaunchKernelGGL(k_track_draw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tc->cdf, tc->track_of_env, n,
                     tc->n_tracks, tc->seed, generation, mix);
  return (int)hipGetLastError();
}
