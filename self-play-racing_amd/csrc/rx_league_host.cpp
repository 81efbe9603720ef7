// rx_league_host.cpp -- the host twins of league training's kernels
// (rx_league_weights_host / rx_league_draw_host, ABI v25 additive): the loops of
// rx_league.hip one slot / one env at a time over the same rx_league.h functions.
// Compiled as plain C++ (not as HIP), so rx_league.h takes its host form;
// rx_api_curriculum.cpp checks the arguments before it calls in here.  No HIP call.
#include "rx.h"
#include "rx_league.h"

extern "C" void rx_host_league_weights(const rx_league_io* lg, int n_live, int power, double mix, double prior) {
  double f[RX_LEAGUE_MAX_SLOTS];
  for (int k = 0; k < RX_LEAGUE_MAX_SLOTS; ++k)
    f[k] = k < n_live ? rx_lg_priority(lg->tally + (size_t)k * RX_LEAGUE_TALLY_W, power, prior) : 0.0;
  for (int k = 0; k < lg->n_slots; ++k) lg->cdf[k] = rx_lg_cdf(f, n_live, mix, k);
}

extern "C" void rx_host_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info) {
  double cdf[RX_LEAGUE_MAX_SLOTS];
  for (int k = 0; k < lg->n_slots; ++k) cdf[k] = lg->cdf[k];
  for (int64_t e = 0; e < n; ++e) {
    if (done) {
      if (done[e] == 0.0f) continue;
      const int32_t k = lg->opp_id[e];
      if (k >= 0 && k < lg->n_slots) {
        int64_t* row = lg->tally + (size_t)k * RX_LEAGUE_TALLY_W;
        const int out = rx_lg_outcome(info + (size_t)e * 2 * RX_INFO_W, lg->agent);
        row[0] += 1;
        if (out & 1) row[1] += 1;
        if (out & 2) row[2] += 1;
      }
    }
    const uint32_t count = (uint32_t)lg->draw_count[e];
    lg->opp_id[e] = rx_lg_pick(cdf, lg->n_slots, rx_lg_uniform(lg->seed, count, (uint32_t)e));
    lg->draw_count[e] = (int32_t)(count + 1u);
  }
}
