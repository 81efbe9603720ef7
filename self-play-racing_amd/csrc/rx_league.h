// rx_league.h -- the rules of league TRAINING (rx_league_weights / rx_league_draw /
// rx_league_rollout_steps, ABI v25 additive) as one set of inline functions compiled
// twice: by hipcc for gfx950 (rx_league.hip) and as plain C++ for the host twins
// (rx_league_host.cpp).  Everything is float64 or integer; every step is ONE
// separately rounded IEEE add, multiply or divide (both translation units are
// compiled with -ffp-contract=off), there is no pow, no exp and no reduction whose
// order depends on the launch shape, so device, host and a NumPy restatement
// (tests/test_league_train_cpu.py) give the same bits.
//
// Rules (DESIGN.md §4 "League training"):
//  * tally[k] = (games, learner wins, opponent wins) of bank slot k, int64;
//  * sampling table of the live slots 0 .. n_live - 1 (prioritised fictitious
//    self-play: a slot the learner still loses to is drawn more often):
//      p_k    = (w + 0.5 * (g - w - l) + prior) / (g + 2 * prior)
//      f_k    = (1 - p_k) multiplied `power` times into 1.0
//      F      = f_0 + f_1 + ... in slot order
//      prob_k = (1 - mix) * (f_k / F) + mix / n_live       (F == 0: 1 / n_live)
//      cdf_k  = cdf_{k-1} + prob_k in slot order; 1.0 for every k >= n_live - 1;
//  * the draw of env e: h = splitmix64(seed ^ splitmix64((count << 32) ^ e)) -- the
//    form of the start-side draw in rx_kernels.hip --, u = (h >> 11) * 2^-53, id =
//    the smallest k with u < cdf_k.  cdf is 1.0 from n_live - 1 on and u < 1, so an
//    id is always a live slot and the draw itself needs no n_live.
#pragma once

#include <stdint.h>

#include "rx.h"
#include "rx_math.h"

#define RX_LEAGUE_MAX_SLOTS 64  // one lane per slot in k_league_weights
#define RX_LEAGUE_MAX_POWER 4
#define RX_LEAGUE_TALLY_W 3     // games, learner wins, opponent wins

RX_FN uint64_t rx_lg_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// f_k of one slot from its tally row
RX_FN double rx_lg_priority(const int64_t* t, int power, double prior) {
  const double g = (double)t[0], w = (double)t[1], l = (double)t[2];
  const double draws = (g - w) - l;
  const double num = (w + 0.5 * draws) + prior;
  const double den = g + 2.0 * prior;
  const double q = 1.0 - num / den;
  double f = 1.0;
  for (int i = 0; i < power; ++i) f = f * q;
  return f;
}

// cdf_k from the priorities f[0 .. n_live - 1] (host memory or LDS): two serial
// loops in slot order, the same for every caller
RX_FN double rx_lg_cdf(const double* f, int n_live, double mix, int k) {
  if (k >= n_live - 1) return 1.0;
  double F = 0.0;
  for (int j = 0; j < n_live; ++j) F = F + f[j];
  const double nl = (double)n_live;
  double c = 0.0;
  for (int j = 0; j <= k; ++j) {
    const double prob = F == 0.0 ? 1.0 / nl : (1.0 - mix) * (f[j] / F) + mix / nl;
    c = c + prob;
  }
  return c;
}

RX_FN double rx_lg_uniform(uint64_t seed, uint32_t count, uint32_t e) {
  const uint64_t h = rx_lg_splitmix64(seed ^ rx_lg_splitmix64(((uint64_t)count << 32) ^ (uint64_t)e));
  return (double)(h >> 11) * 0x1p-53;
}

// the smallest k with u < cdf_k; the last slot when there is none (a table that
// rx_league_weights wrote ends in 1.0, so that never happens with it)
RX_FN int32_t rx_lg_pick(const double* cdf, int n_slots, double u) {
  int32_t k = 0;
  while (k < n_slots - 1 && !(u < cdf[k])) ++k;
  return k;
}

// who won the episode of a two-car env from the terminal step's info rows:
// bit 0 = the learner's car placed first, bit 1 = the opponent's
RX_FN int rx_lg_outcome(const double* info_env, int agent) {
  const double pa = info_env[agent * RX_INFO_W + RX_INFO_PLACEMENT];
  const double po = info_env[(1 - agent) * RX_INFO_W + RX_INFO_PLACEMENT];
  return (pa == 1.0 ? 1 : 0) | (po == 1.0 ? 2 : 0);
}
