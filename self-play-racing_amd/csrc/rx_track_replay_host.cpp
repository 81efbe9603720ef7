// rx_track_replay_host.cpp -- the host twins of the replay-score kernels
// (rx_track_learn_tally_host / _tally_slots_host / _fold_host / _tables_host / _draw_host /
// rx_track_learn_episode_host, ABI v25 additive): the loops of rx_track_replay.hip one value / one slot / one env at a
// time over the same rx_track_replay.h functions.  Compiled as plain C++ (not as
// HIP); rx_api_curriculum.cpp checks the arguments before it calls in here.  No HIP call.
#include <algorithm>
#include <vector>

#include "rx.h"
#include "rx_curriculum.h"  // rx_tc_outcome, rx_tc_progress_q
#include "rx_track_replay.h"

extern "C" void rx_host_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv) {
  for (int32_t t = 0; t < T; ++t) {
    for (int64_t e = 0; e < n; ++e) {
      const int32_t k = lt->track[e];
      if (k < 0 || k >= lt->n_tracks) continue;
      int64_t q;
      if (!rx_tl_mag_q(adv[(int64_t)t * n + e], lt->kind, &q)) continue;
      int64_t* row = lt->learn + (size_t)k * RX_TRACK_LEARN_W;
      row[0] += 1;
      row[1] += q;
    }
  }
}

// the serial loop over [T][n]: the slot of every element from slots, the autoreset rows of dones left out
extern "C" void rx_host_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                                const int32_t* slots, const float* dones) {
  for (int32_t t = 0; t < T; ++t) {
    for (int64_t e = 0; e < n; ++e) {
      const int64_t i = (int64_t)t * n + e;
      int64_t q;
      if (!rx_tl_counts(slots[i], lt->n_tracks, dones ? dones[i] : 0.0f, adv[i], lt->kind, &q)) continue;
      int64_t* row = lt->learn + (size_t)slots[i] * RX_TRACK_LEARN_W;
      row[0] += 1;
      row[1] += q;
    }
  }
}

extern "C" void rx_host_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha) {
  for (int32_t k = 0; k < lt->n_tracks; ++k)
    rx_tl_fold(lt->learn + (size_t)k * RX_TRACK_LEARN_W, lt->score + k, lt->seen + k, update, alpha);
}

// the rank by a stable sort on the descending key: equal keys keep their slot order
extern "C" void rx_host_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now) {
  const int32_t n = lt->n_tracks;
  std::vector<uint64_t> key((size_t)n);
  std::vector<int32_t> order((size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    key[k] = rx_tl_key(lt->score[k], lt->seen[k]);
    order[k] = k;
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] > key[b]; });
  for (int32_t i = 0; i < n; ++i) lt->rank[order[i]] = i + 1;
  uint64_t cw = 0, cs = 0;
  for (int32_t k = 0; k < n; ++k) {
    cw += rx_tl_weight(lt->rank[k], power);
    cs += rx_tl_stale(lt->seen[k], now);
    lt->cdf_score[k] = (int64_t)cw;
    lt->cdf_stale[k] = (int64_t)cs;
  }
}

extern "C" void rx_host_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                                         double stale_mix) {
  for (int64_t e = 0; e < n; ++e)
    lt->track_of_env[e] = rx_tl_draw(lt->cdf_score, lt->cdf_stale, lt->n_tracks, lt->seed, generation, (uint32_t)e,
                                     mix, stale_mix);
}

// k_track_learn_episode one env at a time: rx_host_track_episode with the draw from the replay tables
extern "C" void rx_host_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt,
                                            const rx_track_episode_io* ep, double stale_mix, int64_t n,
                                            const float* done, const uint8_t* terminated, const double* info) {
  for (int64_t e = 0; e < n; ++e) {
    const int32_t k = tc->track[e];
    if (ep->slot_out) ep->slot_out[e] = k;
    if (done[e] == 0.0f || k < 0 || k >= tc->n_tracks) continue;
    const double progress = info[(size_t)e * RX_INFO_W + RX_INFO_PROGRESS];
    const int out = rx_tc_outcome(progress, terminated[e]);
    int64_t* row = tc->tally + (size_t)k * RX_TRACK_TALLY_W;
    row[0] += 1;
    if (out & 1) row[1] += 1;
    if (out & 2) row[2] += 1;
    row[3] += rx_tc_progress_q(progress);
    rx_tl_episode_draw(tc, ep, lt->cdf_score, lt->cdf_stale, lt->seed, stale_mix, n, e);
  }
}
