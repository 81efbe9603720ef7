// rx_track_replay.h -- the rules of the track curriculum's REPLAY SCORES
// (rx_track_learn_tally / _fold / _tables / _draw, ABI v25 additive): the value-loss
// score, rank prioritisation and staleness of prioritised level replay (Jiang et
// al. 2021) over the track slots.  As rx_curriculum.h, one set of inline functions
// compiled twice: by hipcc for gfx950 (rx_track_replay.hip) and as plain C++ for the
// host twins (rx_track_replay_host.cpp), both with -ffp-contract=off.  Floating
// point is float64 with every step ONE separately rounded IEEE operation (no pow,
// no exp); every sum is an INTEGER, so the kernels' atomics and parallel scans, the
// host twins' serial loops and a Python restatement (tests/test_track_replay_cpu.py)
// agree bit for bit.
//
// Rules (DESIGN.md §4 "Replay scores"):
//  * learn[k] = (samples, mag_q) of slot k, int64.  Every advantage a = adv[t][e]
//    of an env on slot k that is finite adds one sample and
//      mag_q += (int64)((double)m * 2^20),  m = min(kind 0: |a|, kind 1: max(a, 0); 2^20)
//    in float32 (|a| and max are exact).  Non-finite values and slots outside the
//    table add nothing.
//  * fold(update u, alpha), per slot with samples > 0:
//      mean  = ((double)mag_q / 2^20) / (double)samples
//      score = seen < 0 ? mean : score + alpha * (mean - score);  seen = u;  learn = 0
//    so a score is never negative.
//  * rank_k = 1 + #{ j : key_j > key_k or (key_j == key_k and j < k) } with
//    key = seen < 0 ? +inf : score: a total order, the never-scored slots first.
//    Keys are compared as their uint64 bit patterns (every key is >= +0.0).
//  * tables:  h = 1.0 / (double)rank;  f = h multiplied `power` times into 1.0;
//      W_k = (uint64)(f * 2^32);  S_k = seen < 0 ? 0 : max(now - seen, 0)
//    cdf_score / cdf_stale are their inclusive exact scans.
//  * the draw of env e at generation g: h1, h2, u of rx_tc_draw;
//      u < mix:                               slot = mulhi64(h2, n_tracks)
//      u < mix + stale_mix and F_stale > 0:   search cdf_stale with mulhi64(h2, F_stale)
//      otherwise:                             search cdf_score (uniform when its total is 0)
//    With stale_mix == 0 it is rx_tc_draw on cdf_score bit for bit.
//  * the tally by per-step slot (rx_track_learn_tally_slots): element (t, e) counts on row
//    slots[t][e] iff adv[t][e] is finite, the slot lies inside the table and dones is null or
//    dones[t][e] == 0.  A row entered with dones != 0 is the autoreset step: its observation is
//    the old track's terminal one, its successor the new track's first, and its advantage belongs
//    to neither slot.
//  * the episodic draw from the replay tables (rx_track_learn_episode): rx_track_episode with
//    the draw above in rx_tc_draw's place, at generation draws[e] under
//    seed ^ RX_TRACK_EPISODE_SALT (rx_curriculum.h).
#pragma once

#include <stdint.h>

#include "rx.h"
#include "rx_curriculum.h"  // rx_tc_mulhi64, rx_tc_search
#include "rx_league.h"      // rx_lg_splitmix64
#include "rx_math.h"

#define RX_TRACK_LEARN_W 2           // samples, mag_q
#define RX_TRACK_LEARN_MAX_POWER 10
#define RX_TRACK_LEARN_CHUNK 1024    // slots k_track_learn_tables scans per pass (one lane each)
#define RX_TRACK_RANK_TILE 1024      // keys k_track_rank stages in LDS per pass
#define RX_TRACK_LEARN_L1 0
#define RX_TRACK_LEARN_POS 1

RX_FN uint32_t rx_tl_f32_bits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b;
}

RX_FN uint64_t rx_tl_f64_bits(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b;
}

// the fixed-point magnitude of one advantage; returns 0 (and adds nothing) for a non-finite one
RX_FN int rx_tl_mag_q(float a, int kind, int64_t* q) {
  if ((rx_tl_f32_bits(a) & 0x7F800000u) == 0x7F800000u) return 0;  // inf or NaN
  float m = kind == RX_TRACK_LEARN_L1 ? (a < 0.0f ? -a : a) : (a > 0.0f ? a : 0.0f);
  if (m > 1048576.0f) m = 1048576.0f;
  *q = (int64_t)((double)m * 1048576.0);
  return 1;
}

// one slot's fold; row = its (samples, mag_q)
RX_FN void rx_tl_fold(int64_t* row, double* score, int32_t* seen, int32_t update, double alpha) {
  const int64_t samples = row[0];
  if (samples <= 0) return;
  const double mean = ((double)row[1] / 1048576.0) / (double)samples;
  const double d = mean - *score;
  *score = *seen < 0 ? mean : *score + alpha * d;
  *seen = update;
  row[0] = 0;
  row[1] = 0;
}

// the rank key as a bit pattern: +inf for a slot never scored
RX_FN uint64_t rx_tl_key(double score, int32_t seen) {
  return seen < 0 ? 0x7FF0000000000000ull : rx_tl_f64_bits(score);
}

// whether slot j stands before slot k in the rank order
RX_FN int rx_tl_before(uint64_t key_j, int32_t j, uint64_t key_k, int32_t k) {
  return key_j > key_k || (key_j == key_k && j < k);
}

RX_FN uint64_t rx_tl_weight(int32_t rank, int power) {
  const double h = 1.0 / (double)rank;
  double f = 1.0;
  for (int i = 0; i < power; ++i) f = f * h;
  return (uint64_t)(f * 4294967296.0);  // 0 < f <= 1
}

RX_FN uint64_t rx_tl_stale(int32_t seen, int32_t now) {
  const int64_t d = (int64_t)now - (int64_t)seen;
  return seen < 0 || d < 0 ? 0ull : (uint64_t)d;
}

RX_FN int32_t rx_tl_draw(const int64_t* cdf_score, const int64_t* cdf_stale, int32_t n_tracks, uint64_t seed,
                         uint32_t g, uint32_t e, double mix, double stale_mix) {
  const uint64_t h1 = rx_lg_splitmix64(seed ^ rx_lg_splitmix64(((uint64_t)g << 32) ^ (uint64_t)e));
  const uint64_t h2 = rx_lg_splitmix64(h1);
  const double u = (double)(h1 >> 11) * 0x1p-53;
  if (u < mix) return (int32_t)rx_tc_mulhi64(h2, (uint64_t)n_tracks);
  if (u < mix + stale_mix) {
    const uint64_t Fs = (uint64_t)cdf_stale[n_tracks - 1];
    if (Fs > 0) return rx_tc_search(cdf_stale, n_tracks, rx_tc_mulhi64(h2, Fs));
  }
  const uint64_t F = (uint64_t)cdf_score[n_tracks - 1];
  if (F == 0) return (int32_t)rx_tc_mulhi64(h2, (uint64_t)n_tracks);
  return rx_tc_search(cdf_score, n_tracks, rx_tc_mulhi64(h2, F));
}

// whether element (slot, done flag, advantage) of the per-step tally counts; *q = its magnitude
RX_FN int rx_tl_counts(int32_t slot, int32_t n_tracks, float done, float a, int kind, int64_t* q) {
  if (done != 0.0f || slot < 0 || slot >= n_tracks) return 0;
  return rx_tl_mag_q(a, kind, q);
}

// rx_tc_episode_draw from the replay tables: the next slot of env e, whose episode just ended on a
// slot inside the table, at generation draws[e], which advances
RX_FN int32_t rx_tl_episode_draw(const rx_track_io* tc, const rx_track_episode_io* ep, const int64_t* cdf_score,
                                 const int64_t* cdf_stale, uint64_t seed, double stale_mix, int64_t n, int64_t e) {
  const uint32_t g = ep->draws[e];
  const int32_t k = rx_tl_draw(cdf_score, cdf_stale, tc->n_tracks, seed ^ RX_TRACK_EPISODE_SALT, g, (uint32_t)e,
                               ep->mix, stale_mix);
  rx_tc_episode_move(tc, ep, n, e, g, k);
  return k;
}
