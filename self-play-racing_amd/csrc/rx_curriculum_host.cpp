// rx_curriculum_host.cpp -- the host twins of the track curriculum's kernels
// (rx_track_tally_host / rx_track_episode_host / rx_track_scores_host /
// rx_track_draw_host / rx_track_tally2_host / rx_track_duel_scores_host, ABI v25 additive): the loops of rx_curriculum.hip one env / one slot at a time over the
// same rx_curriculum.h functions.  Compiled as plain C++ (not as HIP), so
// rx_curriculum.h takes its host form; rx_api_curriculum.cpp checks the arguments before it
// calls in here.  No HIP call.
#include "rx.h"
#include "rx_curriculum.h"
#include "rx_track_duel.h"

extern "C" void rx_host_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                                    const double* info) {
  for (int64_t e = 0; e < n; ++e) {
    if (done[e] == 0.0f) continue;
    const int32_t k = tc->track[e];
    if (k < 0 || k >= tc->n_tracks) continue;
    const double progress = info[(size_t)e * RX_INFO_W + RX_INFO_PROGRESS];
    const int out = rx_tc_outcome(progress, terminated[e]);
    int64_t* row = tc->tally + (size_t)k * RX_TRACK_TALLY_W;
    row[0] += 1;
    if (out & 1) row[1] += 1;
    if (out & 2) row[2] += 1;
    row[3] += rx_tc_progress_q(progress);
  }
}

// k_track_episode one env at a time: slot_out, the tally on the slot the env ran, then its draw
extern "C" void rx_host_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n,
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
    rx_tc_episode_draw(tc, ep, n, e);
  }
}

extern "C" void rx_host_track_scores(const rx_track_io* tc, int power, double prior) {
  uint64_t c = 0;
  for (int32_t k = 0; k < tc->n_tracks; ++k) {
    double pk;
    c += rx_tc_weight(tc->tally + (size_t)k * RX_TRACK_TALLY_W, tc->score, power, prior, &pk);
    tc->p[k] = pk;
    tc->cdf[k] = (int64_t)c;
  }
}

extern "C" void rx_host_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix) {
  for (int64_t e = 0; e < n; ++e)
    tc->track_of_env[e] = rx_tc_draw(tc->cdf, tc->n_tracks, tc->seed, generation, (uint32_t)e, mix);
}

// k_track_tally2 one env at a time (rx_track_duel.h)
extern "C" void rx_host_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                                     const uint8_t* terminated, const double* info) {
  for (int64_t e = 0; e < n; ++e) {
    if (done[e] == 0.0f) continue;
    const int32_t k = tc->track[e];
    if (k < 0 || k >= tc->n_tracks) continue;
    const double* ra = info + ((size_t)e * 2 + td->agent) * RX_INFO_W;
    const double* ro = info + ((size_t)e * 2 + (1 - td->agent)) * RX_INFO_W;
    const double pa = ra[RX_INFO_PROGRESS], po = ro[RX_INFO_PROGRESS];
    const int out = rx_td_outcome(pa, po, ra[RX_INFO_PLACEMENT], terminated[e]);
    int64_t* row = tc->tally + (size_t)k * RX_TRACK_TALLY_W;
    int64_t* drow = td->duel + (size_t)k * RX_TRACK_DUEL_W;
    row[0] += 1;
    if (out & RX_TD_FINISHED) row[1] += 1;
    if (out & RX_TD_CRASHED) row[2] += 1;
    row[3] += rx_tc_progress_q(pa);
    if (out & RX_TD_WON) drow[0] += 1;
    if (out & RX_TD_OPP_FINISHED) drow[1] += 1;
    drow[2] += rx_tc_progress_q(po);
    if (out & RX_TD_TIMEOUT) drow[3] += 1;
  }
}

extern "C" void rx_host_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int power, double prior) {
  uint64_t c = 0;
  for (int32_t k = 0; k < tc->n_tracks; ++k) {
    double pk;
    c += rx_td_weight(tc->tally + (size_t)k * RX_TRACK_TALLY_W, td->duel + (size_t)k * RX_TRACK_DUEL_W, tc->score, power,
                      prior, &pk);
    tc->p[k] = pk;
    tc->cdf[k] = (int64_t)c;
  }
}
