// rx_api_train.cpp -- C ABI (include/rx.h): the training side.  GAE, Adam, the PPO update's
// launches, the permutation, the KL check and the policy forward; none of it reads a handle.
#include "rx_handle.h"

static int gae(int32_t T, int32_t N, const float* r, const float* v, const float* d, const float* nv, const float* nd,
               double gamma, double lam, float* adv, float* ret, int scan, void* stream) {
  if (T <= 0 || N <= 0) return fail(RX_EINVAL, "rx_gae: T=%d N=%d must be > 0", T, N);
  if (!r || !v || !d || !nv || !nd || !adv || !ret) return fail(RX_EINVAL, "rx_gae: null buffer");
  if ((long long)T * N > 0x7fffffffffffLL) return fail(RX_EINVAL, "rx_gae: T*N too large");
  // agent/ppo.py:149,151: c["gamma"] * nnt is float32(gamma) * nnt; the Python
  // double product gamma*lambda is rounded to float32 once.
  const float g = (float)gamma;
  const float gl = (float)(gamma * lam);
  const int rc = rx_launch_gae(T, N, r, v, d, nv, nd, g, gl, adv, ret, scan, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "gae launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_gae(int32_t T, int32_t N, const float* r, const float* v, const float* d, const float* nv, const float* nd,
           double gamma, double lam, float* adv, float* ret, void* stream) {
  return gae(T, N, r, v, d, nv, nd, gamma, lam, adv, ret, 0, stream);
}

int rx_gae_scan(int32_t T, int32_t N, const float* r, const float* v, const float* d, const float* nv,
                const float* nd, double gamma, double lam, float* adv, float* ret, void* stream) {
  return gae(T, N, r, v, d, nv, nd, gamma, lam, adv, ret, 1, stream);
}

static int adam_cfg_error(const rx_adam_config* cfg) {
  if (!cfg) return fail(RX_EINVAL, "rx_adam: cfg is null");
  if (cfg->n_tensors <= 0 || cfg->n_tensors > RX_ADAM_MAX_TENSORS)
    return fail(RX_EINVAL, "rx_adam: n_tensors=%d not in [1, %d]", cfg->n_tensors, RX_ADAM_MAX_TENSORS);
  if (cfg->offsets[0] != 0) return fail(RX_EINVAL, "rx_adam: offsets[0] must be 0");
  for (int k = 0; k < cfg->n_tensors; ++k)
    if (cfg->offsets[k + 1] < cfg->offsets[k]) return fail(RX_EINVAL, "rx_adam: offsets not ascending");
  if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0 && cfg->beta2 >= 0.0 && cfg->beta2 < 1.0 && cfg->eps >= 0.0))
    return fail(RX_EINVAL, "rx_adam: bad betas/eps");
  return RX_OK;
}

size_t rx_adam_workspace_floats(const rx_adam_config* cfg) {
  if (adam_cfg_error(cfg) != RX_OK) return 0;
  const int64_t n = cfg->offsets[cfg->n_tensors];
  const int64_t nb = n > 0 ? (n + RX_ADAM_NORM_ELEMS - 1) / RX_ADAM_NORM_ELEMS : 1;
  return (size_t)(nb * cfg->n_tensors) + 2;  // + Adam's two step scalars
}

int rx_adam_clip_step(const rx_adam_config* cfg, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                      float* step, const double* lr, const uint8_t* stop, float* ws, void* stream) {
  if (const int rc = adam_cfg_error(cfg)) return rc;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !lr || !ws)
    return fail(RX_EINVAL, "rx_adam_clip_step: null buffer");
  const int rc = rx_launch_adam(cfg, params, grads, exp_avg, exp_avg_sq, step, lr, stop, ws, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "adam launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

size_t rx_ppo_workspace_floats(int32_t obs_dim, int32_t mb) {
  return (obs_dim == 15 || obs_dim == 19) && mb > 0 ? rx_ppo_partial_floats(obs_dim, mb) : 0;
}

size_t rx_ppo_workspace_doubles(int32_t mb) { return mb > 0 ? (size_t)rx_ppo_n_wg(mb) : 0; }

static int check_ppo_batch(const rx_ppo_batch* b) {
  if (!b) return fail(RX_EINVAL, "rx_ppo: batch is null");
  if (b->obs_dim != 15 && b->obs_dim != 19) return fail(RX_EINVAL, "rx_ppo: obs_dim=%d (15 or 19)", b->obs_dim);
  if (b->mb <= 0 || b->n_rows <= 0) return fail(RX_EINVAL, "rx_ppo: mb=%d n_rows=%lld", b->mb, (long long)b->n_rows);
  if (precision_arg("rx_ppo", "precision", b->precision)) return RX_EINVAL;
  if (!b->obs || !b->actions || !b->logprobs || !b->advantages || !b->returns || !b->values || !b->perm ||
      !b->params || !b->log_std)
    return fail(RX_EINVAL, "rx_ppo: null buffer");
  return RX_OK;
}

int rx_ppo_adv_stats(const rx_ppo_batch* b, int32_t n_mb, float* stats, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if (n_mb <= 0 || !stats) return fail(RX_EINVAL, "rx_ppo_adv_stats: n_mb=%d stats=%p", n_mb, (void*)stats);
  if ((int64_t)n_mb * b->mb > b->n_rows) return fail(RX_EINVAL, "rx_ppo_adv_stats: n_mb*mb > n_rows");
  if ((rc = rx_launch_adv_stats(b, n_mb, stats, nullptr, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "adv stats launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_ppo_adv_moments(const rx_ppo_batch* b, int32_t n_mb, double* moments, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if (n_mb <= 0 || !moments) return fail(RX_EINVAL, "rx_ppo_adv_moments: n_mb=%d moments=%p", n_mb, (void*)moments);
  if ((int64_t)n_mb * b->mb > b->n_rows) return fail(RX_EINVAL, "rx_ppo_adv_moments: n_mb*mb > n_rows");
  if ((rc = rx_launch_adv_stats(b, n_mb, nullptr, moments, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "adv moments launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

size_t rx_ppo_adv_workspace_doubles(int32_t mb, int32_t n_mb) {
  return mb > 0 && n_mb > 0 ? 2 * (size_t)n_mb * (size_t)rx_adv_chunks(mb) : 0;
}

int rx_ppo_adv_stats_ws(const rx_ppo_batch* b, int32_t n_mb, double* ws, float* stats, double* moments, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if (n_mb <= 0 || !ws || (!stats && !moments))
    return fail(RX_EINVAL, "rx_ppo_adv_stats_ws: n_mb=%d ws=%p stats=%p moments=%p", n_mb, (void*)ws, (void*)stats,
                (void*)moments);
  if ((int64_t)n_mb * b->mb > b->n_rows) return fail(RX_EINVAL, "rx_ppo_adv_stats_ws: n_mb*mb > n_rows");
  if ((rc = rx_launch_adv_stats_ws(b, n_mb, ws, moments ? nullptr : stats, moments, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "adv stats launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_ppo_adv_finalize(const double* moments, int32_t n_mb, int64_t count, float* stats, void* stream) {
  if (n_mb <= 0 || count <= 0 || !moments || !stats)
    return fail(RX_EINVAL, "rx_ppo_adv_finalize: n_mb=%d count=%lld moments=%p stats=%p", n_mb, (long long)count,
                (const void*)moments, (void*)stats);
  const int rc = rx_launch_adv_finalize(moments, n_mb, count, stats, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "adv finalize launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_ppo_minibatch_grad(const rx_ppo_batch* b, int32_t m, float* ws_f32, double* ws_f64, float* grad,
                          uint8_t* stop, float* kl_at_stop, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if (!b->adv_stats) return fail(RX_EINVAL, "rx_ppo_minibatch_grad: adv_stats is null");
  if (m < 0 || (int64_t)(m + 1) * b->mb > b->n_rows) return fail(RX_EINVAL, "rx_ppo_minibatch_grad: m=%d out of range", m);
  if (!ws_f32 || !ws_f64 || !grad || !stop || !kl_at_stop) return fail(RX_EINVAL, "rx_ppo_minibatch_grad: null buffer");
  if ((rc = rx_launch_ppo_grad(b, m, 1.0f, stop, kl_at_stop, nullptr, ws_f32, ws_f64, grad, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "ppo grad launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

size_t rx_ppo_update_workspace_floats(int32_t obs_dim, const rx_adam_config* cfg) {
  if ((obs_dim != 15 && obs_dim != 19) || adam_cfg_error(cfg) != RX_OK) return 0;
  // the per-tensor sums of squares of every reduce block + Adam's two step scalars
  return (size_t)rx_ppo_reduce_blocks(obs_dim) * cfg->n_tensors + 2;
}

int rx_ppo_minibatch_update(const rx_ppo_batch* b, int32_t m, const rx_adam_config* cfg, float* params,
                            float* ws_f32, double* ws_f64, float* grad, float* exp_avg, float* exp_avg_sq, float* step,
                            const double* lr, uint8_t* stop, float* kl_at_stop, float* adam_ws, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if ((rc = adam_cfg_error(cfg))) return rc;
  if (!b->adv_stats) return fail(RX_EINVAL, "rx_ppo_minibatch_update: adv_stats is null");
  if (m < 0 || (int64_t)(m + 1) * b->mb > b->n_rows)
    return fail(RX_EINVAL, "rx_ppo_minibatch_update: m=%d out of range", m);
  if (!params || params != b->params) return fail(RX_EINVAL, "rx_ppo_minibatch_update: params must be b->params");
  if (cfg->offsets[cfg->n_tensors] != rx_ppo_n_params(b->obs_dim))
    return fail(RX_EINVAL, "rx_ppo_minibatch_update: cfg covers %lld parameters, the policy has %d",
                (long long)cfg->offsets[cfg->n_tensors], rx_ppo_n_params(b->obs_dim));
  if (!ws_f32 || !ws_f64 || !grad || !exp_avg || !exp_avg_sq || !step || !lr || !stop || !kl_at_stop || !adam_ws)
    return fail(RX_EINVAL, "rx_ppo_minibatch_update: null buffer");
  const hipStream_t s = (hipStream_t)stream;
  if ((rc = rx_launch_ppo_grad(b, m, 1.0f, stop, kl_at_stop, nullptr, ws_f32, ws_f64, grad, s, cfg, adam_ws, step, lr)))
    return fail(RX_EHIP, "ppo grad launch failed: %s", hipGetErrorString((hipError_t)rc));
  if ((rc = rx_launch_adam_apply(cfg, params, grad, exp_avg, exp_avg_sq, step, lr, stop, adam_ws,
                                 rx_ppo_reduce_blocks(b->obs_dim), s)))
    return fail(RX_EHIP, "adam launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_ppo_minibatch_grad_shard(const rx_ppo_batch* b, int32_t m, float scale, float* ws_f32, double* ws_f64,
                                float* grad, float* kl_out, const uint8_t* stop, void* stream) {
  int rc = check_ppo_batch(b);
  if (rc) return rc;
  if (!b->adv_stats) return fail(RX_EINVAL, "rx_ppo_minibatch_grad_shard: adv_stats is null");
  if (m < 0 || (int64_t)(m + 1) * b->mb > b->n_rows)
    return fail(RX_EINVAL, "rx_ppo_minibatch_grad_shard: m=%d out of range", m);
  if (!(scale > 0.0f)) return fail(RX_EINVAL, "rx_ppo_minibatch_grad_shard: scale=%g", (double)scale);
  if (!ws_f32 || !ws_f64 || !grad || !kl_out || !stop)
    return fail(RX_EINVAL, "rx_ppo_minibatch_grad_shard: null buffer");
  // the kernels only read *stop in shard mode (the decision is rx_ppo_kl_check's)
  if ((rc = rx_launch_ppo_grad(b, m, scale, const_cast<uint8_t*>(stop), nullptr, kl_out, ws_f32, ws_f64, grad,
                               (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "ppo grad launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_random_permutation(int64_t n, uint64_t seed, int64_t* out, void* stream) {
  if (n < 0 || n > (1ll << 62)) return fail(RX_EINVAL, "rx_random_permutation: n = %lld out of range", (long long)n);
  if (n > 0 && !out) return fail(RX_EINVAL, "rx_random_permutation: null output");
  const int rc = rx_launch_permutation(n, seed, out, (hipStream_t)stream);
  if (rc) return fail(RX_EHIP, "rx_random_permutation launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_ppo_kl_check(const float* kl, float kl_target, uint8_t* stop, float* kl_at_stop, void* stream) {
  if (!kl || !stop || !kl_at_stop) return fail(RX_EINVAL, "rx_ppo_kl_check: null buffer");
  const int rc = rx_launch_kl_check(kl, kl_target, stop, kl_at_stop, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "kl check launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_policy_act(const rx_policy_io* io, void* stream) {
  if (!io) return fail(RX_EINVAL, "rx_policy_act: io is null");
  if (io->obs_dim != 15 && io->obs_dim != 19) return fail(RX_EINVAL, "rx_policy_act: obs_dim=%d (15 or 19)", io->obs_dim);
  if (io->n <= 0) return fail(RX_EINVAL, "rx_policy_act: n=%lld", (long long)io->n);
  if (precision_arg("rx_policy_act", "precision", io->precision)) return RX_EINVAL;
  if ((io->obs_stride != 0 && io->obs_stride < io->obs_dim) || (io->act_stride != 0 && io->act_stride < 2) ||
      (io->act2_stride != 0 && io->act2_stride < 2))
    return fail(RX_EINVAL, "rx_policy_act: row strides overlap (obs %lld, act %lld)", (long long)io->obs_stride,
                (long long)io->act_stride);
  if (!io->obs || !io->eps || !io->params || !io->log_std || !io->actions || !io->logprobs || !io->values)
    return fail(RX_EINVAL, "rx_policy_act: null buffer");
  const int rc = rx_launch_policy_act(io, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "policy launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// ABI v25, additive: rx_policy_act with per-row parameters from a bank (k_policy_act_bank)
int rx_policy_act_bank(const rx_policy_bank_io* b, void* stream) {
  if (!b) return fail(RX_EINVAL, "rx_policy_act_bank: io is null");
  const rx_policy_io* io = &b->io;
  if (io->obs_dim != 15 && io->obs_dim != 19)
    return fail(RX_EINVAL, "rx_policy_act_bank: obs_dim=%d (15 or 19)", io->obs_dim);
  if (io->n <= 0) return fail(RX_EINVAL, "rx_policy_act_bank: n=%lld must be > 0", (long long)io->n);
  if (b->n_policies <= 0) return fail(RX_EINVAL, "rx_policy_act_bank: n_policies=%d must be > 0", b->n_policies);
  if (b->params_stride < rx_ppo_n_params(io->obs_dim))
    return fail(RX_EINVAL, "rx_policy_act_bank: params_stride=%lld < the %d parameters of obs_dim %d",
                (long long)b->params_stride, rx_ppo_n_params(io->obs_dim), io->obs_dim);
  if (precision_arg("rx_policy_act_bank", "precision", io->precision)) return RX_EINVAL;
  if ((b->tile_cars != 1 && b->tile_cars != 2) || (b->tile_cars == 2 && (io->n & 1)))
    return fail(RX_EINVAL, "rx_policy_act_bank: tile_cars=%d (1, or 2 with an even n; n=%lld)", b->tile_cars,
                (long long)io->n);
  if ((io->obs_stride != 0 && io->obs_stride < io->obs_dim) || (io->act_stride != 0 && io->act_stride < 2) ||
      (io->act2_stride != 0 && io->act2_stride < 2))
    return fail(RX_EINVAL, "rx_policy_act_bank: row strides overlap (obs_stride %lld, act_stride %lld, act2_stride %lld)",
                (long long)io->obs_stride, (long long)io->act_stride, (long long)io->act2_stride);
  if (!io->obs || !io->eps || !io->params || !io->log_std || !io->actions || !io->logprobs || !io->values ||
      !b->policy_of_row)
    return fail(RX_EINVAL, "rx_policy_act_bank: null %s",
                !io->obs ? "obs" : !io->eps ? "eps" : !io->params ? "params" : !io->log_std ? "log_std"
                : !io->actions ? "actions" : !io->logprobs ? "logprobs" : !io->values ? "values" : "policy_of_row");
  const int rc = rx_launch_policy_act_bank(b, (hipStream_t)stream);
  if (rc != 0) return fail(RX_EHIP, "bank policy launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}
