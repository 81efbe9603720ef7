// rx_api_loops.cpp -- C ABI (include/rx.h): the handle-bound callers of launch().  rx_rollout, the
// three step loops (rollout, two-car rollout, evaluation record) and every *_rollout_steps,
// rx_eval_steps, rx_match_steps and *_episode_step entry point in front of them.
#include "rx_handle.h"

// rx_rollout: the persistent small-N rollout (k_rollout) on a handle in the
// one-env-per-wave configuration; the per-step io pointers are set in-kernel.
static int max_waypoints(const rx_env* h) {
  int m = 0;
  for (int k = 0; k < h->n_tracks; ++k) m = std::max(m, h->wp_off_h[k + 1] - h->wp_off_h[k]);
  return m;
}

int rx_rollout_supported(const rx_env* h) {
  return h && h->assigned && h->bound && h->cfg.n_agents == 1 && h->sched.dyn_lpe == 64 && (h->D == 15 || h->D == 19) &&
         max_waypoints(h) <= RX_ROLLOUT_MAX_W;
}

// ---- the step loops: the argument checks of their entry points, each written once.
// fn is the entry point's name; every check returns before any HIP call.
int precision_arg(const char* fn, const char* field, int32_t precision) {
  if (precision != RX_PREC_FP32 && precision != RX_PREC_BF16)
    return fail(RX_EINVAL, "%s: %s=%d (RX_PREC_FP32 or RX_PREC_BF16)", fn, field, precision);
  return RX_OK;
}

static int rollout_dims(const char* fn, const rx_env* h, const rx_rollout_io* r) {
  if (r->T <= 0) return fail(RX_EINVAL, "%s: T=%d must be > 0", fn, r->T);
  if (r->obs_dim != h->D) return fail(RX_EINVAL, "%s: obs_dim %d != the handle's %d", fn, r->obs_dim, h->D);
  return RX_OK;
}

static int rollout_bufs(const char* fn, const rx_rollout_io* r) {
  const char* null = !r->params ? "params" : !r->log_std ? "log_std" : !r->eps ? "eps" : !r->obs ? "obs"
                     : !r->actions ? "actions" : !r->logprobs ? "logprobs" : !r->values ? "values"
                     : !r->rewards ? "rewards" : !r->dones ? "dones" : !r->next_obs ? "next_obs"
                     : !r->next_done ? "next_done" : nullptr;
  return null ? fail(RX_EINVAL, "%s: null rollout buffer %s", fn, null) : RX_OK;
}

// bank: the opponents' parameters come from a league io, so opp_params / opp_log_std are not read
static int selfplay_bufs(const char* fn, const rx_selfplay_io* sp, bool bank) {
  const char* null = !bank && !sp->opp_params ? "opp_params" : !bank && !sp->opp_log_std ? "opp_log_std"
                     : !sp->opp_eps ? "opp_eps" : !sp->env_actions ? "env_actions" : !sp->env_obs ? "env_obs"
                     : !sp->env_reward ? "env_reward" : !sp->sink ? "sink" : nullptr;
  return null ? fail(RX_EINVAL, "%s: null self-play buffer %s", fn, null) : RX_OK;
}

// the evaluation record, and the io rows k_eval_acc reads
static int record_args(const char* fn, const rx_io* io, const double* acc, const uint8_t* active,
                       const int32_t* n_active) {
  if (!acc || !active || !n_active)
    return fail(RX_EINVAL, "%s: null %s", fn, !acc ? "acc" : !active ? "active" : "n_active");
  if (!io->obs || !io->reward64 || !io->info || !io->done_f32)
    return fail(RX_EINVAL, "%s: null io->%s", fn,
                !io->obs ? "obs" : !io->reward64 ? "reward64" : !io->info ? "info" : "done_f32");
  return RX_OK;
}

// bf16 with parameters that are fixed for the whole call: their operand fragments are built once
// (k_policy_frag) and every step's policy launch reads them -- the same bf16 values rx_policy_act
// converts per use.  *frag stays null for fp32.
static int policy_fragments(const char* fn, rx_env* h, int32_t obs_dim, const float* params, int32_t precision,
                            hipStream_t s, const void** frag) {
  *frag = nullptr;
  if (precision != RX_PREC_BF16) return RX_OK;
  if (rx_launch_policy_frag(obs_dim, params, h->policy_frag.p, s))
    return fail(RX_EHIP, "%s: fragment launch failed", fn);
  *frag = h->policy_frag.p;
  return RX_OK;
}

int rx_rollout(rx_env* h, const rx_io* io, const rx_rollout_io* r, void* stream) {
  if (!h || !io || !r) return fail(RX_EINVAL, "rx_rollout: null argument");
  if (!rx_rollout_supported(h))
    return fail(RX_ESTATE, "rx_rollout: needs an assigned, bound single-agent handle in the small-N (one env per "
                           "wave) configuration with 15 or 19 observation columns and <= %d waypoints per slot",
                RX_ROLLOUT_MAX_W);
  int rc;
  if ((rc = rollout_dims("rx_rollout", h, r)) != 0 || (rc = rollout_bufs("rx_rollout", r)) != 0) return rc;
  if (h->sched.n_dyn_waves != h->cfg.n_envs) return fail(RX_ESTATE, "rx_rollout: expected one env per dynamics wave");
  rx_kargs a{};
  make_kargs(h, io, RX_MODE_STEP, nullptr, a);
  a.sort_keys = nullptr;
  a.tasks_out = nullptr;
  a.prof_ts = nullptr;
  if ((rc = rx_launch_rollout(&a, r, max_waypoints(h), (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "k_rollout launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// The single-agent rollout loop: per step rx_policy_act on obs[t], then rx_step of actions[t] writing
// obs[t + 1], rewards[t] and dones[t + 1] (next_obs / next_done after the last).  tc == null is
// rx_rollout_steps; with tc, rx_track_rollout_steps: one k_track_tally after every step, which reads
// the done row the step just wrote and the env's terminated / info rows before the next step
// overwrites them (one stream).  The policy and env launches are the same either way.
// With ep as well, rx_track_episodic_rollout_steps: k_track_episode in the tally's place, so an env
// that ended in step t is reset by step t + 1 from the slot it just drew; slots: [T][N] or null.
// With lt too, rx_track_learn_episodic_rollout_steps: k_track_learn_episode in that launch's place.
static int rollout_loop(const char* fn, rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                        int32_t precision, void* stream, const rx_track_episode_io* ep = nullptr,
                        int32_t* slots = nullptr, const rx_track_learn_io* lt = nullptr, double stale_mix = 0.0) {
  const int64_t N = h->cfg.n_envs, D = h->D;
  hipStream_t hs = (hipStream_t)stream;
  const void* frag;
  int rc = policy_fragments(fn, h, r->obs_dim, r->params, precision, hs, &frag);
  if (rc) return rc;
  for (int32_t t = 0; t < r->T; ++t) {
    const bool last = t + 1 == r->T;
    const rx_policy_io pio{r->obs_dim, N, r->obs + t * N * D, r->eps + t * N * 2, r->params, r->log_std,
                           r->actions + t * N * 2, r->logprobs + t * N, r->values + t * N, 0, 0, precision,
                           nullptr, 0};
    if ((rc = rx_launch_policy_act(&pio, hs, frag)) != 0)
      return fail(RX_EHIP, "%s: policy launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
    rx_io s = *io;
    s.actions = r->actions + t * N * 2;
    s.obs = last ? r->next_obs : r->obs + (t + 1) * N * D;
    s.reward = r->rewards + t * N;
    s.done_f32 = last ? r->next_done : r->dones + (t + 1) * N;
    if ((rc = launch(h, &s, RX_MODE_STEP, nullptr, stream)) != 0) return rc;
    if (ep) {
      rx_track_episode_io e = *ep;
      e.slot_out = slots ? slots + t * N : nullptr;
      rc = lt ? rx_launch_track_learn_episode(tc, lt, &e, stale_mix, N, s.done_f32, io->terminated, io->info, hs)
              : rx_launch_track_episode(tc, &e, N, s.done_f32, io->terminated, io->info, hs);
      if (rc != 0) return fail(RX_EHIP, "%s: episode launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
    } else if (tc && (rc = rx_launch_track_tally(tc, N, s.done_f32, io->terminated, io->info, hs)) != 0)
      return fail(RX_EHIP, "%s: tally launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  }
  return RX_OK;
}

// The two-car rollout loop: per step ONE launch for both policies, then rx_step on the env's own
// buffers; one agent-row copy after the last step.  The opponent's actor runs on its rows of the
// env's observation buffer (wrappers.py:36-39), actions into its slot of the env's action buffer;
// the learning agent on obs[t] -- the caller's rows at t = 0 (they may predate an env rebuild),
// afterwards its rows of the env's buffer, which the launch also copies into obs[t] together with
// the agent's reward of step t - 1 -- actions into the rollout row and its env slot.
// lg == null is rx_selfplay_rollout_steps (k_selfplay_act, one frozen opponent).  With lg,
// rx_league_rollout_steps (k_league_act): env e's opponent is bank member lg->opp_id[e], the
// opponent's params / log_std are the bank bases, and the tally and redraw of step t's done flags
// is folded into step t + 1's launch (its opponent waves are the only readers of the ids), so one
// k_league_draw per rollout remains, for the last step.  RX_LEAGUE_FOLD=0 (an A/B build,
// tools/bench_league_train.py) launches k_league_draw after every step instead: the same bits,
// one more launch per step.
#ifndef RX_LEAGUE_FOLD
#define RX_LEAGUE_FOLD 1
#endif
// With tc and td, rx_track_duel_rollout_steps: one k_track_tally2 after every step, which reads the
// done row the step just wrote and the env's terminated / info rows before the next step overwrites
// them (one stream); with lg the next step's folded draw reads the same info rows, and neither
// writes them.  The policy and env launches are the same either way.
static int two_car_rollout_loop(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                                const rx_league_io* lg, int32_t precision, void* stream,
                                const rx_track_io* tc = nullptr, const rx_track_duel_io* td = nullptr) {
  const int64_t N = h->cfg.n_envs, D = h->D;
  const int q = sp->agent, o = 1 - q;
  hipStream_t hs = (hipStream_t)stream;
  int rc;
  for (int32_t t = 0; t < r->T; ++t) {
    const bool last = t + 1 == r->T;
    const rx_policy_io opp{(int32_t)D, N, sp->env_obs + o * D, sp->opp_eps + t * N * 2,
                           lg ? lg->params : sp->opp_params, lg ? lg->log_std : sp->opp_log_std,
                           sp->env_actions + 2 * o, nullptr, sp->sink, 2 * D, 4,
                           lg ? lg->opp_precision : sp->opp_precision, nullptr, 0};
    const rx_policy_io pio{(int32_t)D, N, t == 0 ? r->obs : sp->env_obs + q * D, r->eps + t * N * 2, r->params,
                           r->log_std, r->actions + t * N * 2, r->logprobs + t * N, r->values + t * N,
                           t == 0 ? 0 : 2 * D, 0, precision, sp->env_actions + 2 * q, 4};
    float* obs_out = t == 0 ? nullptr : r->obs + t * N * D;
    float* rew_out = t == 0 ? nullptr : r->rewards + (t - 1) * N;
    if (lg) {
      // io->info still holds step t - 1's rows here: rx_step writes it after this launch
      const bool fold = RX_LEAGUE_FOLD && t > 0;
      rc = rx_launch_league_act(&pio, &opp, lg, fold ? r->dones + t * N : nullptr, fold ? io->info : nullptr,
                                obs_out, sp->env_reward, rew_out, hs);
    } else {
      rc = rx_launch_selfplay_act(&pio, &opp, obs_out, sp->env_reward, rew_out, q, hs);
    }
    if (rc)
      return fail(RX_EHIP, "%s policy launch failed: %s", lg ? "league" : "self-play",
                  hipGetErrorString((hipError_t)rc));
    rx_io s = *io;
    s.actions = sp->env_actions;
    s.obs = sp->env_obs;
    s.reward = sp->env_reward;
    s.done_f32 = last ? r->next_done : r->dones + (t + 1) * N;  // dones['__all__'] (wrappers.py:51)
    if ((rc = launch(h, &s, RX_MODE_STEP, nullptr, stream)) != 0) return rc;
    // the envs that ended: count the episode against their track slot
    if (tc && (rc = rx_launch_track_tally2(tc, td, N, s.done_f32, io->terminated, io->info, hs)) != 0)
      return fail(RX_EHIP, "track tally launch failed: %s", hipGetErrorString((hipError_t)rc));
    // the envs that ended: count the result against their opponent, draw the next one
    if (lg && (last || !RX_LEAGUE_FOLD) && (rc = rx_launch_league_draw(lg, N, s.done_f32, io->info, hs)) != 0)
      return fail(RX_EHIP, "league draw launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  // the last step's agent rows: next_obs and rewards[T - 1]
  rc = rx_launch_agent_rows((int)N, (int)D, q, sp->env_obs, sp->env_reward, r->next_obs, r->rewards + (r->T - 1) * N,
                            hs);
  if (rc) return fail(RX_EHIP, "agent-row copy launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// The accumulating loop of an evaluation: per step the policy launch (if any), rx_step of actions[t]
// in place, k_eval_acc.  ev.params == null is open loop (the caller's actions); with m the policy
// launch is the bank's (car q of env e on policy m->seat[e][q]), else rx_policy_act over all N * A
// rows -- both cars of a two-car env are rows of the same launch: one policy drives them
// (utils/metrics.py:94-101).  ev holds the fields rx_eval_io and rx_match_io share.
static int record_loop(const char* fn, rx_env* h, const rx_io* io, const rx_eval_io& ev, const rx_match_io* m,
                       int32_t n_steps, void* stream) {
  const int64_t N = h->cfg.n_envs, A = h->cfg.n_agents, NA = N * A;
  hipStream_t hs = (hipStream_t)stream;
  const void* frag = nullptr;
  int rc;
  if (ev.params && !m && (rc = policy_fragments(fn, h, ev.obs_dim, ev.params, ev.precision, hs, &frag)) != 0)
    return rc;
  for (int32_t t = 0; t < n_steps; ++t) {
    float* act = ev.actions + (int64_t)t * NA * 2;
    if (ev.params) {
      const rx_policy_io pio{ev.obs_dim, NA, io->obs, ev.eps + (int64_t)t * NA * 2, ev.params, ev.log_std, act,
                             ev.logp_sink, ev.value_sink, 0, 0, ev.precision, nullptr, 0};
      if (m) {
        const rx_policy_bank_io b{pio, m->n_policies, (int32_t)A, m->params_stride, m->seat};
        rc = rx_launch_policy_act_bank(&b, hs);
      } else {
        rc = rx_launch_policy_act(&pio, hs, frag);
      }
      if (rc) return fail(RX_EHIP, "%s: policy launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
    }
    rx_io s = *io;
    s.actions = act;
    if ((rc = launch(h, &s, RX_MODE_STEP, nullptr, stream)) != 0) return rc;
    // after launch(): its re-sort (if any) has been enqueued, so perm and the working rows agree
    if ((rc = rx_launch_eval_acc((int)N, (int)A, h->perm[0].p, &h->work, io, ev.acc, ev.active, ev.n_active,
                                 hs)) != 0)
      return fail(RX_EHIP, "k_eval_acc launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  return RX_OK;
}

int rx_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, int32_t precision, void* stream) {
  const char* fn = "rx_rollout_steps";
  if (!h || !io || !r) return fail(RX_EINVAL, "%s: null argument", fn);
  if (!h->assigned || !h->bound) return fail(RX_ESTATE, "%s: needs an assigned, bound handle", fn);
  if (h->cfg.n_agents != 1) return fail(RX_EINVAL, "%s: single-agent handles only", fn);
  int rc;
  if ((rc = rollout_dims(fn, h, r)) != 0 || (rc = rollout_bufs(fn, r)) != 0 ||
      (rc = precision_arg(fn, "precision", precision)) != 0)
    return rc;
  return rollout_loop(fn, h, io, r, nullptr, precision, stream);
}

int rx_selfplay_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                              int32_t precision, void* stream) {
  const char* fn = "rx_selfplay_rollout_steps";
  if (!h || !io || !r || !sp) return fail(RX_EINVAL, "%s: null argument", fn);
  if (!h->assigned || !h->bound) return fail(RX_ESTATE, "%s: needs an assigned, bound handle", fn);
  if (h->cfg.n_agents != 2) return fail(RX_EINVAL, "%s: two-car handles only", fn);
  int rc = rollout_dims(fn, h, r);
  if (rc) return rc;
  if (sp->agent != 0 && sp->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, sp->agent);
  if ((rc = rollout_bufs(fn, r)) != 0 || (rc = selfplay_bufs(fn, sp, false)) != 0) return rc;
  if (h->D != 19) return fail(RX_EINVAL, "%s: obs_dim %d (19)", fn, h->D);
  if ((rc = precision_arg(fn, "precision", precision)) != 0 ||
      (rc = precision_arg(fn, "opp_precision", sp->opp_precision)) != 0)
    return rc;
  return two_car_rollout_loop(h, io, r, sp, nullptr, precision, stream);
}

// ABI v25: an evaluation's step loop (policy or open-loop actions, rx_step, k_eval_acc
// per step) enqueued by one call; every argument is checked before the first HIP call.
int rx_eval_steps(rx_env* h, const rx_io* io, const rx_eval_io* ev, int32_t n_steps, void* stream) {
  if (!h) return fail(RX_EINVAL, "rx_eval_steps: null handle");
  if (!io) return fail(RX_EINVAL, "rx_eval_steps: null io");
  if (!ev) return fail(RX_EINVAL, "rx_eval_steps: null ev");
  if (n_steps <= 0) return fail(RX_EINVAL, "rx_eval_steps: n_steps=%d must be > 0", n_steps);
  if (!ev->actions) return fail(RX_EINVAL, "rx_eval_steps: null actions");
  int rc = record_args("rx_eval_steps", io, ev->acc, ev->active, ev->n_active);
  if (rc) return rc;
  if (ev->params) {  // policy mode
    if (ev->obs_dim != 15 && ev->obs_dim != 19)
      return fail(RX_EINVAL, "rx_eval_steps: obs_dim=%d has no policy kernel (15 or 19)", ev->obs_dim);
    if ((rc = precision_arg("rx_eval_steps", "precision", ev->precision)) != 0) return rc;
    if (!ev->log_std || !ev->eps || !ev->logp_sink || !ev->value_sink)
      return fail(RX_EINVAL, "rx_eval_steps: null %s (policy mode)",
                  !ev->log_std ? "log_std" : !ev->eps ? "eps" : !ev->logp_sink ? "logp_sink" : "value_sink");
  }
  // from here on the handle is read
  if (ev->obs_dim != h->D) return fail(RX_EINVAL, "rx_eval_steps: obs_dim %d != the handle's %d", ev->obs_dim, h->D);
  if (h->n_tracks <= 0 || !h->assigned || !h->bound)
    return fail(RX_ESTATE, "rx_eval_steps: needs an assigned, bound handle");
  return record_loop("rx_eval_steps", h, io, *ev, nullptr, n_steps, stream);
}

// ABI v25, additive: rx_eval_steps' policy mode with a seating -- per step one bank launch
// (car q of env e on policy seat[e][q]), rx_step, k_eval_acc.
int rx_match_steps(rx_env* h, const rx_io* io, const rx_match_io* m, int32_t n_steps, void* stream) {
  if (!h) return fail(RX_EINVAL, "rx_match_steps: null handle");
  if (!io) return fail(RX_EINVAL, "rx_match_steps: null io");
  if (!m) return fail(RX_EINVAL, "rx_match_steps: null match io");
  if (n_steps <= 0) return fail(RX_EINVAL, "rx_match_steps: n_steps=%d must be > 0", n_steps);
  if (m->obs_dim != 15 && m->obs_dim != 19)
    return fail(RX_EINVAL, "rx_match_steps: obs_dim=%d has no policy kernel (15 or 19)", m->obs_dim);
  int rc = precision_arg("rx_match_steps", "precision", m->precision);
  if (rc) return rc;
  if (m->n_policies <= 0) return fail(RX_EINVAL, "rx_match_steps: n_policies=%d must be > 0", m->n_policies);
  if (m->params_stride < rx_ppo_n_params(m->obs_dim))
    return fail(RX_EINVAL, "rx_match_steps: params_stride=%lld < the %d parameters of obs_dim %d",
                (long long)m->params_stride, rx_ppo_n_params(m->obs_dim), m->obs_dim);
  if (!m->params || !m->log_std || !m->eps || !m->seat || !m->actions || !m->logp_sink || !m->value_sink)
    return fail(RX_EINVAL, "rx_match_steps: null %s",
                !m->params ? "params" : !m->log_std ? "log_std" : !m->eps ? "eps" : !m->seat ? "seat"
                : !m->actions ? "actions" : !m->logp_sink ? "logp_sink" : "value_sink");
  if ((rc = record_args("rx_match_steps", io, m->acc, m->active, m->n_active)) != 0) return rc;
  // from here on the handle is read
  if (m->obs_dim != h->D) return fail(RX_EINVAL, "rx_match_steps: obs_dim %d != the handle's %d", m->obs_dim, h->D);
  if (h->n_tracks <= 0 || !h->assigned || !h->bound)
    return fail(RX_ESTATE, "rx_match_steps: needs an assigned, bound handle");
  if (h->cfg.n_agents != 1 && h->cfg.n_agents != 2)
    return fail(RX_EINVAL, "rx_match_steps: n_agents=%d (1 or 2)", h->cfg.n_agents);
  const rx_eval_io ev{m->obs_dim, m->precision, m->params, m->log_std, m->eps, m->actions, m->logp_sink,
                      m->value_sink, m->acc, m->active, m->n_active};
  return record_loop("rx_match_steps", h, io, ev, m, n_steps, stream);
}

// the two-car rollout loop with a per-env opponent from the bank (two_car_rollout_loop)
int rx_league_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                            const rx_league_io* lg, int32_t precision, void* stream) {
  const char* fn = "rx_league_rollout_steps";
  // the league io first: its refusals need no handle (tests/test_league_train_cpu.py)
  int rc = league_args(fn, lg, 2);
  if (rc) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (!io || !r || !sp) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : !r ? "rollout io" : "self-play io");
  if (!h->assigned || !h->bound || h->cfg.n_agents != 2 || h->D != 19)
    return fail(RX_EINVAL, "%s: the handle must be an assigned, bound two-car handle with obs_dim 19", fn);
  if ((rc = rollout_dims(fn, h, r)) != 0) return rc;
  if (sp->agent != lg->agent)
    return fail(RX_EINVAL, "%s: agent %d of the self-play io != agent %d of the league io", fn, sp->agent, lg->agent);
  if ((rc = rollout_bufs(fn, r)) != 0 || (rc = selfplay_bufs(fn, sp, true)) != 0) return rc;
  if (!io->info) return fail(RX_EINVAL, "%s: null io->info (the tally reads the terminal step's placement)", fn);
  return two_car_rollout_loop(h, io, r, sp, lg, precision, stream);
}

// the io rows every track tally reads after the step
static int tally_rows(const char* fn, const rx_io* io) {
  if (!io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null io->%s (the tally reads the terminal step's rows)", fn,
                !io->terminated ? "terminated" : "info");
  return RX_OK;
}

// the single-agent rollout loop with the tally (rollout_loop)
int rx_track_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                           int32_t precision, void* stream) {
  const char* fn = "rx_track_rollout_steps";
  // the track io first: its refusals need no handle (tests/test_curriculum_cpu.py)
  int rc = track_args(fn, tc, 0);
  if (rc) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (!io || !r) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : "rollout io");
  if (!h->assigned || !h->bound || h->cfg.n_agents != 1)
    return fail(RX_EINVAL, "%s: the handle must be an assigned, bound single-agent handle", fn);
  if ((rc = rollout_dims(fn, h, r)) != 0 || (rc = rollout_bufs(fn, r)) != 0) return rc;
  if ((rc = tally_rows(fn, io)) != 0) return rc;
  return rollout_loop(fn, h, io, r, tc, precision, stream);
}

// the two-car rollout loop with the tally (two_car_rollout_loop); lg: the league's opponents, or null
int rx_track_duel_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                                const rx_league_io* lg, const rx_track_io* tc, const rx_track_duel_io* td,
                                int32_t precision, void* stream) {
  const char* fn = "rx_track_duel_rollout_steps";
  // the track and league ios first: their refusals need no handle (tests/test_track_selfplay_cpu.py)
  int rc = track_args(fn, tc, 0);
  if (rc || (rc = track_duel_io(fn, td)) != 0) return rc;
  if (lg && (rc = league_args(fn, lg, 2)) != 0) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (!io || !r || !sp) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : !r ? "rollout io" : "self-play io");
  if (!h->assigned || !h->bound || h->cfg.n_agents != 2 || h->D != 19)
    return fail(RX_EINVAL, "%s: the handle must be an assigned, bound two-car handle with obs_dim 19", fn);
  if ((rc = rollout_dims(fn, h, r)) != 0) return rc;
  if (sp->agent != 0 && sp->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, sp->agent);
  if (td->agent != sp->agent)
    return fail(RX_EINVAL, "%s: agent %d of the track duel io != agent %d of the self-play io", fn, td->agent,
                sp->agent);
  if (lg && lg->agent != td->agent)
    return fail(RX_EINVAL, "%s: agent %d of the league io != agent %d of the track duel io", fn, lg->agent, td->agent);
  if ((rc = rollout_bufs(fn, r)) != 0 || (rc = selfplay_bufs(fn, sp, lg != nullptr)) != 0) return rc;
  if (!lg && (rc = precision_arg(fn, "opp_precision", sp->opp_precision)) != 0) return rc;
  if ((rc = tally_rows(fn, io)) != 0) return rc;
  return two_car_rollout_loop(h, io, r, sp, lg, precision, stream, tc, td);
}

// the handle of the two handle-bound forms: lane-varying slots and next-step autoreset
static int track_episode_handle(const char* fn, const rx_env* h, const rx_track_io* tc) {
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (!h->assigned || !h->bound || h->cfg.n_agents != 1)
    return fail(RX_EINVAL, "%s: the handle must be an assigned, bound single-agent handle", fn);
  if (!h->sched.lane_tracks)
    return fail(RX_EINVAL, "%s: the handle's schedule is not lane-varying: set rx_config.lane_tracks = 1 (it needs "
                           "one lane per env: with at most %d envs set dyn_lpe = 1 as well)", fn, RX_WIDE_N);
  if (h->cfg.autoreset != RX_AUTORESET_NEXT_STEP)
    return fail(RX_EINVAL, "%s: autoreset=%d must be RX_AUTORESET_NEXT_STEP: the step after a terminal one resets "
                           "the env from the slot just drawn", fn, h->cfg.autoreset);
  if (tc->track != h->st.track)
    return fail(RX_EINVAL, "%s: track must be the handle's bound rx_state.track", fn);
  return RX_OK;
}

// the episode io of a handle-bound form: the wave-order arrays are the handle's
static rx_track_episode_io episode_on_handle(const rx_env* h, const rx_track_episode_io* ep) {
  rx_track_episode_io e = *ep;
  e.env_pos = h->env_pos.p;
  e.pos_slot = h->pos_slot.p;
  return e;
}

// rx_track_episode on a handle, after a step; with lt, rx_track_learn_episode (the draw from the
// replay tables: lt is read only with learn).  done == null: the io's done row.
static int episode_step(const char* fn, bool learn, rx_env* h, const rx_track_io* tc, const rx_track_learn_io* lt,
                        const rx_track_episode_io* ep, double stale_mix, const rx_io* io, const float* done,
                        void* stream) {
  int rc = learn ? learn_episode_args(fn, tc, lt, ep, stale_mix) : track_episode_args(fn, tc, ep);
  if (rc || (rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io) return fail(RX_EINVAL, "%s: null io", fn);
  if (!done) done = io->done_f32;
  if (!done || !io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null %s", fn, !done ? "done" : !io->terminated ? "io->terminated" : "io->info");
  const rx_track_episode_io e = episode_on_handle(h, ep);
  const int64_t N = h->cfg.n_envs;
  const hipStream_t s = (hipStream_t)stream;
  return launched(fn, learn ? rx_launch_track_learn_episode(tc, lt, &e, stale_mix, N, done, io->terminated, io->info, s)
                            : rx_launch_track_episode(tc, &e, N, done, io->terminated, io->info, s));
}

int rx_track_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_episode_io* ep, const rx_io* io,
                          const float* done, void* stream) {
  return episode_step("rx_track_episode_step", false, h, tc, nullptr, ep, 0.0, io, done, stream);
}
int rx_track_learn_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_learn_io* lt,
                                const rx_track_episode_io* ep, double stale_mix, const rx_io* io, const float* done,
                                void* stream) {
  return episode_step("rx_track_learn_episode_step", true, h, tc, lt, ep, stale_mix, io, done, stream);
}

// The single-agent rollout loop with the tally and the episodic draw (rollout_loop); with learn,
// the draw from lt's replay tables.  The track, learn and episode ios first: their refusals need no handle.
static int episodic_rollout(const char* fn, bool learn, rx_env* h, const rx_io* io, const rx_rollout_io* r,
                            const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                            double stale_mix, int32_t* slots, int32_t precision, void* stream) {
  int rc = learn ? learn_episode_args(fn, tc, lt, ep, stale_mix) : track_episode_args(fn, tc, ep);
  if (rc) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if ((rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io || !r) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : "rollout io");
  if ((rc = rollout_dims(fn, h, r)) != 0 || (rc = rollout_bufs(fn, r)) != 0) return rc;
  if ((rc = tally_rows(fn, io)) != 0) return rc;
  const rx_track_episode_io e = episode_on_handle(h, ep);
  return rollout_loop(fn, h, io, r, tc, precision, stream, &e, slots, lt, stale_mix);
}

int rx_track_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                    const rx_track_episode_io* ep, int32_t* slots, int32_t precision, void* stream) {
  return episodic_rollout("rx_track_episodic_rollout_steps", false, h, io, r, tc, nullptr, ep, 0.0, slots, precision,
                          stream);
}
int rx_track_learn_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                          const rx_track_learn_io* lt, const rx_track_episode_io* ep, double stale_mix,
                                          int32_t* slots, int32_t precision, void* stream) {
  return episodic_rollout("rx_track_learn_episodic_rollout_steps", true, h, io, r, tc, lt, ep, stale_mix, slots,
                          precision, stream);
}
