// rx_curriculum.h -- the rules of the TRACK CURRICULUM (rx_track_tally /
// rx_track_scores / rx_track_draw / rx_track_rollout_steps, ABI v25 additive) as one
// set of inline functions compiled twice: by hipcc for gfx950 (rx_curriculum.hip)
// and as plain C++ for the host twins (rx_curriculum_host.cpp).  The scores are
// float64 with every step ONE separately rounded IEEE operation (both translation
// units are compiled with -ffp-contract=off; no pow, no exp); the sampling weights
// and every sum are INTEGERS, so any summation order gives the same bits: the
// kernel's parallel scan, the host twin's serial loop and a Python restatement
// (tests/test_curriculum_cpu.py) agree bit for bit.
//
// Rules (DESIGN.md §4 "Track curriculum"):
//  * tally[k] = (episodes, finishes, crashes, progress_q) of track slot k, int64.
//    An env whose episode ended on slot k counts one episode; finished = the
//    terminal step's info progress == 1.0 (the env reports exactly 1.0 only for a
//    finished lap, racing_env.py:158-159); crashed = terminated and not finished;
//    everything else is a timeout.  progress_q += (int64)(progress * 2^20).
//  * sampling weights:
//      p_k = (finishes + prior) / (episodes + 2 * prior)          (unseen: 0.5)
//      q_k = 1 - p_k                 score 0, "fail": the tracks still failed
//      q_k = 4 * p_k * (1 - p_k)     score 1, "potential": sometimes solved
//      f_k = q_k multiplied `power` times into 1.0
//      W_k = (uint64)(f_k * 2^32);   cdf_k = W_0 + ... + W_k (exact);  F = cdf_{n-1}
//  * the draw of env e at generation g:
//      h1 = splitmix64(seed ^ splitmix64(((uint64)g << 32) ^ e));  h2 = splitmix64(h1)
//      u  = (h1 >> 11) * 2^-53
//      F == 0 or u < mix:  slot = mulhi64(h2, n_tracks)            (uniform)
//      otherwise:          r = mulhi64(h2, F), slot = the smallest k with r < cdf_k
//    so a slot with W_k == 0 is reached through the uniform part only.
//  * the EPISODIC draw (rx_track_episode): an env whose episode ended on slot k is
//    tallied into row k and then takes the draw above at generation g = draws[e], its
//    own count of draws so far, under seed ^ RX_TRACK_EPISODE_SALT; draws[e] = g + 1.
//    The salt keeps the keys (draws[e], e) apart from rx_track_draw's (generation, e).
#pragma once

#include <stdint.h>

#include "rx.h"
#include "rx_league.h"  // rx_lg_splitmix64
#include "rx_math.h"

#define RX_TRACK_TALLY_W 4         // episodes, finishes, crashes, progress_q
#define RX_TRACK_MAX_POWER 4
#define RX_TRACK_SCORES_CHUNK 1024 // slots k_track_scores scans per pass (one lane each)
#define RX_TRACK_SCORE_FAIL 0
#define RX_TRACK_SCORE_POTENTIAL 1
#define RX_TRACK_EPISODE_SALT 0x9c3b5e2d7f1a8046ull  // the episodic draw's seed = seed ^ this

RX_FN uint64_t rx_tc_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIPCC__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// the outcome of an ended episode: bit 0 = finished, bit 1 = crashed, 0 = timeout
RX_FN int rx_tc_outcome(double progress, uint8_t terminated) {
  const int fin = progress == 1.0 ? 1 : 0;
  return fin | ((terminated != 0 && !fin) ? 2 : 0);
}

RX_FN int64_t rx_tc_progress_q(double progress) { return (int64_t)(progress * 1048576.0); }

// W_k of one slot from its tally row; *p_out = p_k
RX_FN uint64_t rx_tc_weight(const int64_t* t, int score, int power, double prior, double* p_out) {
  const double n = (double)t[0], fin = (double)t[1];
  const double p = (fin + prior) / (n + 2.0 * prior);
  *p_out = p;
  const double fail = 1.0 - p;
  const double q = score == RX_TRACK_SCORE_POTENTIAL ? (4.0 * p) * fail : fail;
  double f = 1.0;
  for (int i = 0; i < power; ++i) f = f * q;
  const double w = f * 4294967296.0;
  return w > 0.0 ? (uint64_t)w : 0ull;  // a tally with finishes > episodes (never written here) weighs nothing
}

// the smallest k with r < cdf_k, for r < cdf[n_tracks - 1]: the search ends inside the table
RX_FN int32_t rx_tc_search(const int64_t* cdf, int32_t n_tracks, uint64_t r) {
  int32_t lo = 0, hi = n_tracks - 1;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (r < (uint64_t)cdf[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the slot of env e at generation g from the inclusive integer table cdf[0 .. n_tracks - 1]
RX_FN int32_t rx_tc_draw(const int64_t* cdf, int32_t n_tracks, uint64_t seed, uint32_t g, uint32_t e, double mix) {
  const uint64_t h1 = rx_lg_splitmix64(seed ^ rx_lg_splitmix64(((uint64_t)g << 32) ^ (uint64_t)e));
  const uint64_t h2 = rx_lg_splitmix64(h1);
  const double u = (double)(h1 >> 11) * 0x1p-53;
  const uint64_t F = (uint64_t)cdf[n_tracks - 1];
  if (F == 0 || u < mix) return (int32_t)rx_tc_mulhi64(h2, (uint64_t)n_tracks);
  return rx_tc_search(cdf, n_tracks, rx_tc_mulhi64(h2, F));
}

// The episodic draw of env e, whose episode just ended on a slot inside the table: its
// next slot at generation draws[e], which advances; track[e] and, when the wave-order
// arrays are given, pos_slot[env_pos[e]] take it (a position outside [0, n) is not written).
// what every episodic draw writes: the counter past generation g, and the slot k drawn at g
RX_FN void rx_tc_episode_move(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, int64_t e, uint32_t g,
                              int32_t k) {
  ep->draws[e] = g + 1u;
  const_cast<int32_t*>(tc->track)[e] = k;
  if (ep->env_pos) {
    const int64_t pos = ep->env_pos[e];
    if (pos >= 0 && pos < n) ep->pos_slot[pos] = k;
  }
}

RX_FN int32_t rx_tc_episode_draw(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, int64_t e) {
  const uint32_t g = ep->draws[e];
  const int32_t k = rx_tc_draw(tc->cdf, tc->n_tracks, tc->seed ^ RX_TRACK_EPISODE_SALT, g, (uint32_t)e, ep->mix);
  rx_tc_episode_move(tc, ep, n, e, g, k);
  return k;
}

#if defined(__HIPCC__)
// The tally of one episodic launch, shared by k_track_episode and k_track_learn_episode
// (rx_track_replay.hip): the envs that ended (slot k inside the table) are folded per slot INSIDE
// the wave -- a leader slot read from the lowest pending lane, its lanes balloted, the counts
// popcounts against the finished / crashed ballots, progress_q a butterfly sum -- and ONE lane adds
// the non-zero columns.  EVERY lane of the wave must call it (ballots and shuffles); returns
// whether this lane's env was tallied, which is also whether it draws.
RX_FN bool rx_tc_wave_episode_tally(int64_t* tally, int32_t n_tracks, bool ended, int32_t k,
                                    const uint8_t* terminated, const double* info, int64_t e) {
  int32_t slot = -1;
  int out = 0;
  long long pq = 0;
  if (ended && k >= 0 && k < n_tracks) {  // a slot outside the table is neither counted nor redrawn
    const double progress = info[(size_t)e * RX_INFO_W + RX_INFO_PROGRESS];
    slot = k;
    out = rx_tc_outcome(progress, terminated[e]);
    pq = (long long)rx_tc_progress_q(progress);
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
      unsigned long long* row = reinterpret_cast<unsigned long long*>(tally + (size_t)s * RX_TRACK_TALLY_W);
      const unsigned long long nf = (unsigned long long)__popcll(same & fin);
      const unsigned long long nc = (unsigned long long)__popcll(same & crash);
      atomicAdd(row, (unsigned long long)__popcll(same));
      if (nf) atomicAdd(row + 1, nf);
      if (nc) atomicAdd(row + 2, nc);
      if (sum) atomicAdd(row + 3, (unsigned long long)sum);
    }
    todo &= ~same;
  }
  return live;
}
#endif
