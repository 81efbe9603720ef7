// rx_api_curriculum.cpp -- C ABI (include/rx.h): the league and the track curriculum -- tally,
// duel, episode, replay ("learn") and evolve.  None of it reads a handle; the handle-bound forms
// (*_rollout_steps, *_episode_step) are in rx_api_loops.cpp and run the ios' checks from here.
//
// Every device / host pair is one static body taking (fn, host, the arguments, stream): the
// checks, all before any HIP call, then the kernel's launch or, with host, the twin's loop
// (rx_*_host.cpp).  The two exported functions pass their own name and nothing else, so a
// refusal cannot differ between an entry and its CPU-tested twin.
#include "rx_handle.h"

// ---- the scalar ranges, each spelled once
static int null_arg(const char* fn, const char* name) { return fail(RX_EINVAL, "%s: null %s", fn, name); }

static int count_arg(const char* fn, int64_t n) {
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  return RX_OK;
}

// a probability or fraction (NaN refused)
static int unit_arg(const char* fn, const char* name, double v) {
  if (!(v >= 0.0 && v <= 1.0)) return fail(RX_EINVAL, "%s: %s=%g outside [0, 1]", fn, name, v);
  return RX_OK;
}

static int power_arg(const char* fn, int32_t power, int32_t max) {
  if (power < 0 || power > max) return fail(RX_EINVAL, "%s: power=%d outside 0..%d", fn, power, max);
  return RX_OK;
}

static int prior_arg(const char* fn, double prior) {
  if (!(prior > 0.0)) return fail(RX_EINVAL, "%s: prior=%g must be > 0", fn, prior);
  return RX_OK;
}

// ---- ABI v25, additive: league training (csrc/rx_league.h).
// what: 0 = weights, 1 = draw, 2 = rollout.
int league_args(const char* fn, const rx_league_io* lg, int what) {
  if (!lg) return fail(RX_EINVAL, "%s: null league io", fn);
  if (lg->n_slots < 1 || lg->n_slots > 64) return fail(RX_EINVAL, "%s: n_slots=%d outside 1..64", fn, lg->n_slots);
  if (!lg->tally || !lg->cdf) return null_arg(fn, !lg->tally ? "tally" : "cdf");
  if (what == 0) return RX_OK;
  if (lg->agent != 0 && lg->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, lg->agent);
  if (!lg->opp_id || !lg->draw_count) return null_arg(fn, !lg->opp_id ? "opp_id" : "draw_count");
  if (what == 1) return RX_OK;
  if (!lg->params || !lg->log_std) return null_arg(fn, !lg->params ? "params" : "log_std");
  if (lg->params_stride < rx_ppo_n_params(19))
    return fail(RX_EINVAL, "%s: params_stride=%lld < the %d parameters of obs_dim 19", fn,
                (long long)lg->params_stride, rx_ppo_n_params(19));
  return precision_arg(fn, "opp_precision", lg->opp_precision);
}

static int league_weights(const char* fn, bool host, const rx_league_io* lg, int32_t n_live, int32_t power, double mix,
                          double prior, void* stream) {
  int rc = league_args(fn, lg, 0);
  if (rc) return rc;
  if (n_live < 1 || n_live > lg->n_slots)
    return fail(RX_EINVAL, "%s: n_live=%d outside 1..n_slots=%d", fn, n_live, lg->n_slots);
  if ((rc = power_arg(fn, power, 4)) || (rc = unit_arg(fn, "mix", mix)) || (rc = prior_arg(fn, prior))) return rc;
  if (!host) return launched(fn, rx_launch_league_weights(lg, n_live, power, mix, prior, (hipStream_t)stream));
  rx_host_league_weights(lg, n_live, power, mix, prior);
  return RX_OK;
}

static int league_draw(const char* fn, bool host, const rx_league_io* lg, int64_t n, const float* done,
                       const double* info, void* stream) {
  int rc = league_args(fn, lg, 1);
  if (rc || (rc = count_arg(fn, n))) return rc;
  if (done && !info) return fail(RX_EINVAL, "%s: null info (required with done)", fn);
  if (!host) return launched(fn, rx_launch_league_draw(lg, n, done, info, (hipStream_t)stream));
  rx_host_league_draw(lg, n, done, info);
  return RX_OK;
}

int rx_league_weights(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior, void* stream) {
  return league_weights("rx_league_weights", false, lg, n_live, power, mix, prior, stream);
}
int rx_league_weights_host(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior,
                           void* stream) {
  return league_weights("rx_league_weights_host", true, lg, n_live, power, mix, prior, stream);
}
int rx_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* stream) {
  return league_draw("rx_league_draw", false, lg, n, done, info, stream);
}
int rx_league_draw_host(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* stream) {
  return league_draw("rx_league_draw_host", true, lg, n, done, info, stream);
}

// ---- ABI v25, additive: the track curriculum (csrc/rx_curriculum.h).
// what: 0 = tally, 1 = scores (tc->score in 0 .. max_score), 2 = draw.
int track_args(const char* fn, const rx_track_io* tc, int what, int max_score) {
  if (!tc) return fail(RX_EINVAL, "%s: null track io", fn);
  if (tc->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, tc->n_tracks);
  if (what == 0 && (!tc->track || !tc->tally)) return null_arg(fn, !tc->track ? "track" : "tally");
  if (what == 1) {
    if (!tc->tally || !tc->cdf || !tc->p) return null_arg(fn, !tc->tally ? "tally" : !tc->cdf ? "cdf" : "p");
    if (tc->score < 0 || tc->score > max_score)  // (the two spellings predate the shared check)
      return max_score == 1 ? fail(RX_EINVAL, "%s: score=%d must be 0 or 1", fn, tc->score)
                            : fail(RX_EINVAL, "%s: score=%d outside 0..%d", fn, tc->score, max_score);
  }
  if (what == 2 && (!tc->cdf || !tc->track_of_env)) return null_arg(fn, !tc->cdf ? "cdf" : "track_of_env");
  return RX_OK;
}

// the env count and the step rows every tally reads
static int tally_inputs(const char* fn, int64_t n, const float* done, const uint8_t* terminated, const double* info) {
  const int rc = count_arg(fn, n);
  if (rc) return rc;
  if (!done || !terminated || !info) return null_arg(fn, !done ? "done" : !terminated ? "terminated" : "info");
  return RX_OK;
}

static int track_tally(const char* fn, bool host, const rx_track_io* tc, int64_t n, const float* done,
                       const uint8_t* terminated, const double* info, void* stream) {
  int rc = track_args(fn, tc, 0);
  if (rc || (rc = tally_inputs(fn, n, done, terminated, info))) return rc;
  if (!host) return launched(fn, rx_launch_track_tally(tc, n, done, terminated, info, (hipStream_t)stream));
  rx_host_track_tally(tc, n, done, terminated, info);
  return RX_OK;
}

static int track_scores(const char* fn, bool host, const rx_track_io* tc, int32_t power, double prior, void* stream) {
  int rc = track_args(fn, tc, 1);
  if (rc || (rc = power_arg(fn, power, 4)) || (rc = prior_arg(fn, prior))) return rc;
  if (!host) return launched(fn, rx_launch_track_scores(tc, power, prior, (hipStream_t)stream));
  rx_host_track_scores(tc, power, prior);
  return RX_OK;
}

static int track_draw(const char* fn, bool host, const rx_track_io* tc, int64_t n, uint32_t generation, double mix,
                      void* stream) {
  int rc = track_args(fn, tc, 2);
  if (rc || (rc = count_arg(fn, n)) || (rc = unit_arg(fn, "mix", mix))) return rc;
  if (!host) return launched(fn, rx_launch_track_draw(tc, n, generation, mix, (hipStream_t)stream));
  rx_host_track_draw(tc, n, generation, mix);
  return RX_OK;
}

int rx_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated, const double* info,
                   void* stream) {
  return track_tally("rx_track_tally", false, tc, n, done, terminated, info, stream);
}
int rx_track_tally_host(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                        const double* info, void* stream) {
  return track_tally("rx_track_tally_host", true, tc, n, done, terminated, info, stream);
}
int rx_track_scores(const rx_track_io* tc, int32_t power, double prior, void* stream) {
  return track_scores("rx_track_scores", false, tc, power, prior, stream);
}
int rx_track_scores_host(const rx_track_io* tc, int32_t power, double prior, void* stream) {
  return track_scores("rx_track_scores_host", true, tc, power, prior, stream);
}
int rx_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* stream) {
  return track_draw("rx_track_draw", false, tc, n, generation, mix, stream);
}
int rx_track_draw_host(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* stream) {
  return track_draw("rx_track_draw_host", true, tc, n, generation, mix, stream);
}

// ---- ABI v25, additive: the track curriculum for self-play (csrc/rx_track_duel.h).
int track_duel_io(const char* fn, const rx_track_duel_io* td) {
  if (!td) return fail(RX_EINVAL, "%s: null track duel io", fn);
  if (td->agent != 0 && td->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, td->agent);
  if (!td->duel) return null_arg(fn, "duel");
  return RX_OK;
}

static int track_tally2(const char* fn, bool host, const rx_track_io* tc, const rx_track_duel_io* td, int64_t n,
                        const float* done, const uint8_t* terminated, const double* info, void* stream) {
  int rc = track_args(fn, tc, 0);
  if (rc || (rc = track_duel_io(fn, td)) || (rc = tally_inputs(fn, n, done, terminated, info))) return rc;
  if (!host) return launched(fn, rx_launch_track_tally2(tc, td, n, done, terminated, info, (hipStream_t)stream));
  rx_host_track_tally2(tc, td, n, done, terminated, info);
  return RX_OK;
}

// rx_track_scores' checks with the duel scores' range (0 .. 3) and the duel io
static int track_duel_scores(const char* fn, bool host, const rx_track_io* tc, const rx_track_duel_io* td,
                             int32_t power, double prior, void* stream) {
  int rc = track_args(fn, tc, 1, 3);
  if (rc || (rc = track_duel_io(fn, td)) || (rc = power_arg(fn, power, 4)) || (rc = prior_arg(fn, prior))) return rc;
  if (!host) return launched(fn, rx_launch_track_duel_scores(tc, td, power, prior, (hipStream_t)stream));
  rx_host_track_duel_scores(tc, td, power, prior);
  return RX_OK;
}

int rx_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                    const uint8_t* terminated, const double* info, void* stream) {
  return track_tally2("rx_track_tally2", false, tc, td, n, done, terminated, info, stream);
}
int rx_track_tally2_host(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                         const uint8_t* terminated, const double* info, void* stream) {
  return track_tally2("rx_track_tally2_host", true, tc, td, n, done, terminated, info, stream);
}
int rx_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                         void* stream) {
  return track_duel_scores("rx_track_duel_scores", false, tc, td, power, prior, stream);
}
int rx_track_duel_scores_host(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                              void* stream) {
  return track_duel_scores("rx_track_duel_scores_host", true, tc, td, power, prior, stream);
}

// ---- ABI v25, additive: episodic track draws (rx_track_episode, csrc/rx_curriculum.h).  The checks that
// need no handle: rx_track_tally's, rx_track_draw's table and mix, and the episode io.
// table: whether the draw reads tc->cdf (the replay forms read rx_track_learn_io's tables instead).
int track_episode_args(const char* fn, const rx_track_io* tc, const rx_track_episode_io* ep, bool table) {
  int rc = track_args(fn, tc, 0);
  if (rc) return rc;
  if (table && !tc->cdf) return null_arg(fn, "cdf");
  if (!ep) return fail(RX_EINVAL, "%s: null episode io", fn);
  if (!ep->draws) return null_arg(fn, "draws");
  if (!ep->env_pos != !ep->pos_slot)
    return fail(RX_EINVAL, "%s: null %s (env_pos and pos_slot: both or neither)", fn,
                !ep->env_pos ? "env_pos" : "pos_slot");
  return unit_arg(fn, "mix", ep->mix);
}

static int track_episode(const char* fn, bool host, const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n,
                         const float* done, const uint8_t* terminated, const double* info, void* stream) {
  int rc = track_episode_args(fn, tc, ep);
  if (rc || (rc = tally_inputs(fn, n, done, terminated, info))) return rc;
  if (!host) return launched(fn, rx_launch_track_episode(tc, ep, n, done, terminated, info, (hipStream_t)stream));
  rx_host_track_episode(tc, ep, n, done, terminated, info);
  return RX_OK;
}

int rx_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                     const uint8_t* terminated, const double* info, void* stream) {
  return track_episode("rx_track_episode", false, tc, ep, n, done, terminated, info, stream);
}
int rx_track_episode_host(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                          const uint8_t* terminated, const double* info, void* stream) {
  return track_episode("rx_track_episode_host", true, tc, ep, n, done, terminated, info, stream);
}

// ---- ABI v25, additive: the curriculum's replay scores (csrc/rx_track_replay.h).
static int learn_io(const char* fn, const rx_track_learn_io* lt) {
  if (!lt) return fail(RX_EINVAL, "%s: null track learn io", fn);
  if (lt->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, lt->n_tracks);
  return RX_OK;
}

// rx_track_learn_tally's checks; by_slot: rx_track_learn_tally_slots', which reads no lt->track
static int learn_tally_args(const char* fn, const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                            bool by_slot) {
  int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (lt->kind != 0 && lt->kind != 1) return fail(RX_EINVAL, "%s: kind=%d must be 0 or 1", fn, lt->kind);
  if (!by_slot && !lt->track) return null_arg(fn, "track");
  if (!lt->learn) return null_arg(fn, "learn");
  if (T <= 0) return fail(RX_EINVAL, "%s: T=%d must be > 0", fn, T);
  if ((rc = count_arg(fn, n))) return rc;
  if (!adv) return null_arg(fn, "adv");
  return RX_OK;
}

// the stale share of a replay draw beside the uniform share `mix` (rx_track_learn_draw's rules)
static int stale_args(const char* fn, const rx_track_learn_io* lt, double mix, double stale_mix) {
  const int rc = unit_arg(fn, "stale_mix", stale_mix);
  if (rc) return rc;
  if (!(mix + stale_mix <= 1.0))
    return fail(RX_EINVAL, "%s: mix + stale_mix = %g + %g above 1", fn, mix, stale_mix);
  if (stale_mix > 0.0 && !lt->cdf_stale) return null_arg(fn, "cdf_stale");
  return RX_OK;
}

static int learn_tally(const char* fn, bool host, const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                       void* stream) {
  const int rc = learn_tally_args(fn, lt, T, n, adv, false);
  if (rc) return rc;
  if (!host) return launched(fn, rx_launch_track_learn_tally(lt, T, n, adv, (hipStream_t)stream));
  rx_host_track_learn_tally(lt, T, n, adv);
  return RX_OK;
}

static int learn_fold(const char* fn, bool host, const rx_track_learn_io* lt, int32_t update, double alpha,
                      void* stream) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->learn) return null_arg(fn, "learn");
  if (!lt->score) return null_arg(fn, "score");
  if (!lt->seen) return null_arg(fn, "seen");
  if (!(alpha > 0.0 && alpha <= 1.0)) return fail(RX_EINVAL, "%s: alpha=%g outside (0, 1]", fn, alpha);
  if (!host) return launched(fn, rx_launch_track_learn_fold(lt, update, alpha, (hipStream_t)stream));
  rx_host_track_learn_fold(lt, update, alpha);
  return RX_OK;
}

static int learn_tables(const char* fn, bool host, const rx_track_learn_io* lt, int32_t power, int32_t now,
                        void* stream) {
  int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->score) return null_arg(fn, "score");
  if (!lt->seen) return null_arg(fn, "seen");
  if (!lt->rank) return null_arg(fn, "rank");
  if (!lt->cdf_score) return null_arg(fn, "cdf_score");
  if (!lt->cdf_stale) return null_arg(fn, "cdf_stale");
  if ((rc = power_arg(fn, power, 10))) return rc;  // the rank exponent: a wider range than the tallies' 0..4
  if (now < 0) return fail(RX_EINVAL, "%s: now=%d must be >= 0", fn, now);
  if (!host) return launched(fn, rx_launch_track_learn_tables(lt, power, now, (hipStream_t)stream));
  rx_host_track_learn_tables(lt, power, now);
  return RX_OK;
}

static int learn_draw(const char* fn, bool host, const rx_track_learn_io* lt, int64_t n, uint32_t generation,
                      double mix, double stale_mix, void* stream) {
  int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->cdf_score) return null_arg(fn, "cdf_score");
  if (!lt->track_of_env) return null_arg(fn, "track_of_env");
  if ((rc = count_arg(fn, n)) || (rc = unit_arg(fn, "mix", mix)) || (rc = stale_args(fn, lt, mix, stale_mix)))
    return rc;
  if (!host) return launched(fn, rx_launch_track_learn_draw(lt, n, generation, mix, stale_mix, (hipStream_t)stream));
  rx_host_track_learn_draw(lt, n, generation, mix, stale_mix);
  return RX_OK;
}

int rx_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* stream) {
  return learn_tally("rx_track_learn_tally", false, lt, T, n, adv, stream);
}
int rx_track_learn_tally_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* stream) {
  return learn_tally("rx_track_learn_tally_host", true, lt, T, n, adv, stream);
}
int rx_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha, void* stream) {
  return learn_fold("rx_track_learn_fold", false, lt, update, alpha, stream);
}
int rx_track_learn_fold_host(const rx_track_learn_io* lt, int32_t update, double alpha, void* stream) {
  return learn_fold("rx_track_learn_fold_host", true, lt, update, alpha, stream);
}
int rx_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now, void* stream) {
  return learn_tables("rx_track_learn_tables", false, lt, power, now, stream);
}
int rx_track_learn_tables_host(const rx_track_learn_io* lt, int32_t power, int32_t now, void* stream) {
  return learn_tables("rx_track_learn_tables_host", true, lt, power, now, stream);
}
int rx_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix, double stale_mix,
                        void* stream) {
  return learn_draw("rx_track_learn_draw", false, lt, n, generation, mix, stale_mix, stream);
}
int rx_track_learn_draw_host(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                             double stale_mix, void* stream) {
  return learn_draw("rx_track_learn_draw_host", true, lt, n, generation, mix, stale_mix, stream);
}

// ---- ABI v25, additive: the replay scores on episodic draws -- the tally by per-step slot and the
// episode-end draw from the replay tables (csrc/rx_track_replay.h).
static int learn_tally_slots(const char* fn, bool host, const rx_track_learn_io* lt, int32_t T, int64_t n,
                             const float* adv, const int32_t* slots, const float* dones, void* stream) {
  const int rc = learn_tally_args(fn, lt, T, n, adv, true);
  if (rc) return rc;
  if (!slots) return null_arg(fn, "slots");
  if (!host) return launched(fn, rx_launch_track_learn_tally_slots(lt, T, n, adv, slots, dones, (hipStream_t)stream));
  rx_host_track_learn_tally_slots(lt, T, n, adv, slots, dones);
  return RX_OK;
}

// the checks of the replay episodic forms that need no handle: rx_track_episode's but for tc->cdf,
// then the learn io's tables and the two mixes
int learn_episode_args(const char* fn, const rx_track_io* tc, const rx_track_learn_io* lt,
                       const rx_track_episode_io* ep, double stale_mix) {
  int rc = track_episode_args(fn, tc, ep, false);
  if (rc || (rc = learn_io(fn, lt))) return rc;
  if (lt->n_tracks != tc->n_tracks)
    return fail(RX_EINVAL, "%s: n_tracks=%d of the track learn io != n_tracks=%d of the track io", fn, lt->n_tracks,
                tc->n_tracks);
  if (!lt->cdf_score) return null_arg(fn, "cdf_score");
  return stale_args(fn, lt, ep->mix, stale_mix);
}

static int learn_episode(const char* fn, bool host, const rx_track_io* tc, const rx_track_learn_io* lt,
                         const rx_track_episode_io* ep, double stale_mix, int64_t n, const float* done,
                         const uint8_t* terminated, const double* info, void* stream) {
  int rc = learn_episode_args(fn, tc, lt, ep, stale_mix);
  if (rc || (rc = tally_inputs(fn, n, done, terminated, info))) return rc;
  if (!host)
    return launched(fn, rx_launch_track_learn_episode(tc, lt, ep, stale_mix, n, done, terminated, info,
                                                      (hipStream_t)stream));
  rx_host_track_learn_episode(tc, lt, ep, stale_mix, n, done, terminated, info);
  return RX_OK;
}

int rx_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                               const int32_t* slots, const float* dones, void* stream) {
  return learn_tally_slots("rx_track_learn_tally_slots", false, lt, T, n, adv, slots, dones, stream);
}
int rx_track_learn_tally_slots_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                    const int32_t* slots, const float* dones, void* stream) {
  return learn_tally_slots("rx_track_learn_tally_slots_host", true, lt, T, n, adv, slots, dones, stream);
}
int rx_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                           double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                           const double* info, void* stream) {
  return learn_episode("rx_track_learn_episode", false, tc, lt, ep, stale_mix, n, done, terminated, info, stream);
}
int rx_track_learn_episode_host(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                                double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                                const double* info, void* stream) {
  return learn_episode("rx_track_learn_episode_host", true, tc, lt, ep, stale_mix, n, done, terminated, info, stream);
}

// ---- ABI v25, additive: track evolution (csrc/rx_track_evolve.h).
static int evolve_io(const char* fn, const rx_track_evolve_io* ev) {
  if (!ev) return fail(RX_EINVAL, "%s: null track evolve io", fn);
  if (ev->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, ev->n_tracks);
  if (ev->n_spawn < 0 || ev->n_spawn > ev->n_tracks)
    return fail(RX_EINVAL, "%s: n_spawn=%d outside 0..n_tracks=%d", fn, ev->n_spawn, ev->n_tracks);
  if (ev->n_spawn > 0) {
    if (!ev->slots) return null_arg(fn, "slots");
    if (!ev->plan) return null_arg(fn, "plan");
  }
  if (!ev->cp_off) return null_arg(fn, "cp_off");
  return RX_OK;
}

static int evolve_plan(const char* fn, bool host, const rx_track_evolve_io* ev, uint32_t generation, double edit_frac,
                       void* stream) {
  int rc = evolve_io(fn, ev);
  if (rc) return rc;
  if (!ev->cdf_score) return null_arg(fn, "cdf_score");
  if ((rc = unit_arg(fn, "edit_frac", edit_frac))) return rc;
  // The twins differ here: with nothing to spawn the device form returns (a zero-size grid is
  // never launched); the host twin goes on into its loop, which then runs no iteration.
  if (!host && ev->n_spawn == 0) return RX_OK;
  if (!host) return launched(fn, rx_launch_track_evolve_plan(ev, generation, edit_frac, (hipStream_t)stream));
  rx_host_track_evolve_plan(ev, generation, edit_frac);
  return RX_OK;
}

static int evolve(const char* fn, bool host, const rx_track_evolve_io* ev, uint32_t generation, void* stream) {
  const int rc = evolve_io(fn, ev);
  if (rc) return rc;
  if (!ev->cp) return null_arg(fn, "cp");
  if (!ev->width) return null_arg(fn, "width");
  if (!ev->cp_off_new) return null_arg(fn, "cp_off_new");
  if (!ev->cp_new) return null_arg(fn, "cp_new");
  if (!ev->width_new) return null_arg(fn, "width_new");
  if (!host) return launched(fn, rx_launch_track_evolve(ev, generation, (hipStream_t)stream));
  rx_host_track_evolve(ev, generation);
  return RX_OK;
}

int rx_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* stream) {
  return evolve_plan("rx_track_evolve_plan", false, ev, generation, edit_frac, stream);
}
int rx_track_evolve_plan_host(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* stream) {
  return evolve_plan("rx_track_evolve_plan_host", true, ev, generation, edit_frac, stream);
}
int rx_track_evolve(const rx_track_evolve_io* ev, uint32_t generation, void* stream) {
  return evolve("rx_track_evolve", false, ev, generation, stream);
}
int rx_track_evolve_host(const rx_track_evolve_io* ev, uint32_t generation, void* stream) {
  return evolve("rx_track_evolve_host", true, ev, generation, stream);
}

// ---- ABI v25, additive: track evolution in place.  One body for the three stages and their
// twins; which: 0 classes, 1 inplace, 2 commit.  With nothing to spawn, stages 1 and 2 return
// before anything is read, in both twins.
static int evolve_inplace(const char* fn, bool host, const rx_track_evolve_inplace_io* ev, int which,
                          uint32_t generation, double edit_frac, void* stream) {
  if (!ev) return fail(RX_EINVAL, "%s: null track evolve inplace io", fn);
  if (ev->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, ev->n_tracks);
  if (ev->n_spawn < 0 || ev->n_spawn > ev->n_tracks)
    return fail(RX_EINVAL, "%s: n_spawn=%d outside 0..n_tracks=%d", fn, ev->n_spawn, ev->n_tracks);
  if (which == 1) {
    const int rc = unit_arg(fn, "edit_frac", edit_frac);
    if (rc) return rc;
  }
  if (which != 0 && ev->n_spawn == 0) return RX_OK;
  if (which != 0 && !ev->slots) return null_arg(fn, "slots");
  if (!ev->cp_off) return null_arg(fn, "cp_off");
  if (which != 0) {
    if (!ev->cp) return null_arg(fn, "cp");
    if (!ev->width) return null_arg(fn, "width");
  }
  if (which == 0 && !ev->cdf_score) return null_arg(fn, "cdf_score");
  if (which != 2) {
    if (!ev->order) return null_arg(fn, "order");
    if (!ev->cdf_class) return null_arg(fn, "cdf_class");
    if (!ev->class_end) return null_arg(fn, "class_end");
  }
  if (which == 1 && !ev->plan) return null_arg(fn, "plan");
  if (which != 0) {
    if (!ev->out_off) return null_arg(fn, "out_off");
    if (!ev->cp_out) return null_arg(fn, "cp_out");
    if (!ev->width_out) return null_arg(fn, "width_out");
  }
  const hipStream_t s = (hipStream_t)stream;
  if (!host)
    return launched(fn, which == 0   ? rx_launch_track_evolve_classes(ev, s)
                        : which == 1 ? rx_launch_track_evolve_inplace(ev, generation, edit_frac, s)
                                     : rx_launch_track_evolve_commit(ev, s));
  if (which == 0) rx_host_track_evolve_classes(ev);
  if (which == 1) rx_host_track_evolve_inplace(ev, generation, edit_frac);
  if (which == 2) rx_host_track_evolve_commit(ev);
  return RX_OK;
}

int rx_track_evolve_classes(const rx_track_evolve_inplace_io* ev, void* stream) {
  return evolve_inplace("rx_track_evolve_classes", false, ev, 0, 0, 0.0, stream);
}
int rx_track_evolve_classes_host(const rx_track_evolve_inplace_io* ev, void* stream) {
  return evolve_inplace("rx_track_evolve_classes_host", true, ev, 0, 0, 0.0, stream);
}
int rx_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac, void* stream) {
  return evolve_inplace("rx_track_evolve_inplace", false, ev, 1, generation, edit_frac, stream);
}
int rx_track_evolve_inplace_host(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac,
                                 void* stream) {
  return evolve_inplace("rx_track_evolve_inplace_host", true, ev, 1, generation, edit_frac, stream);
}
int rx_track_evolve_commit(const rx_track_evolve_inplace_io* ev, void* stream) {
  return evolve_inplace("rx_track_evolve_commit", false, ev, 2, 0, 0.0, stream);
}
int rx_track_evolve_commit_host(const rx_track_evolve_inplace_io* ev, void* stream) {
  return evolve_inplace("rx_track_evolve_commit_host", true, ev, 2, 0, 0.0, stream);
}
