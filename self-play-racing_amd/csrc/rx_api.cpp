// rx_api.cpp -- C ABI (include/rx.h): what owns or mutates the handle.  The error state, handle
// lifetime, track-table upload, env->wavefront grouping, state binding, the step's launches
// and rx_steps.  The other entry points: rx_api_loops.cpp (rollout, eval and match loops),
// rx_api_train.cpp (GAE, Adam, PPO, policies), rx_api_tracks.cpp (track and culling tables,
// rasteriser), rx_api_curriculum.cpp (league and track curriculum); rx_handle.h joins them.
//
// Everything that allocates or copies synchronously (rx_upload_tracks,
// rx_assign) happens outside the step path; rx_reset / rx_step / rx_gae only
// enqueue kernels on the caller's stream, so they can be graph-captured.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "rx_handle.h"

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int launched(const char* fn, int rc) {
  return rc ? fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc)) : RX_OK;
}

// Culling tables for every slot (rx_cull.h through the host twin): chunks of G
// consecutive boundary segments per side, their end-point boxes, per slot the
// bounding circle of all boundary points and the longest segment (kernel margins,
// DESIGN.md §3), the float32 copies and the per-slot headers.
static int build_chunks(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* seg,
                 const double* meta) {
  const int G = h->cfg.cull_chunk, SG = h->cfg.cull_super;  // SG: leaves per super-chunk (0 = one level)
  int64_t tot[4];
  int rc;
  if ((rc = rx_cull_table_sizes(n_tracks, wp_off, G, SG, tot))) return rc;
  const size_t n1 = (size_t)n_tracks + 1, Wt = (size_t)wp_off[n_tracks];
  std::vector<int32_t> off(n1), soff(n1), woff(n1), wsoff(n1);
  std::vector<double> boxes(4 * tot[0]), sboxes(4 * tot[1]), wboxes(4 * tot[2]), wsboxes(4 * tot[3]);
  std::vector<double> geo(4 * (size_t)n_tracks);
  std::vector<float> boxes_f(20 * tot[0]), sboxes_f(20 * tot[1]), sf(8 * Wt);
  std::vector<rx_slot_hdr> hd((size_t)n_tracks);
  const rx_cull_tables t = {off.data(),    soff.data(),    woff.data(), wsoff.data(),   boxes.data(),
                            sboxes.data(), wboxes.data(),  wsboxes.data(), geo.data(), boxes_f.data(),
                            sboxes_f.data(), sf.data(), hd.data()};
  if ((rc = rx_build_cull_tables_host(n_tracks, wp_off, wp, seg, meta, G, SG, &t, nullptr))) return rc;
  if ((rc = upload(h->seg_f, sf.data(), sf.size()))) return rc;
  if (G > 0) {
    h->n_chunk_boxes = (int32_t)tot[0];
    h->n_super_boxes = (int32_t)tot[1];
    if ((rc = upload(h->chunk_box_f, boxes_f.data(), boxes_f.size()))) return rc;
    if (SG > 0 && (rc = upload(h->super_box_f, sboxes_f.data(), sboxes_f.size()))) return rc;
    if ((rc = upload(h->chunk_off, off.data(), off.size()))) return rc;
    if ((rc = upload(h->chunk_box, boxes.data(), boxes.size()))) return rc;
    if ((rc = upload(h->slot_geo, geo.data(), geo.size()))) return rc;
    if ((rc = upload(h->wchunk_off, woff.data(), woff.size()))) return rc;
    if ((rc = upload(h->wchunk_box, wboxes.data(), wboxes.size()))) return rc;
    if ((rc = upload(h->wsuper_off, wsoff.data(), wsoff.size()))) return rc;
    if ((rc = upload(h->wsuper_box, wsboxes.data(), wsboxes.size()))) return rc;
    if (SG > 0) {
      if ((rc = upload(h->super_off, soff.data(), soff.size()))) return rc;
      if ((rc = upload(h->super_box, sboxes.data(), sboxes.size()))) return rc;
    }
  }
  return upload(h->slot_hdr, hd.data(), hd.size());
}

const char* rx_last_error(void) { return g_err.c_str(); }
int rx_abi_version(void) { return RX_ABI_VERSION; }

int rx_create(const rx_config* cfg, rx_env** out) {
  if (!cfg || !out) return fail(RX_EINVAL, "rx_create: null argument");
  *out = nullptr;
  std::string err;
  int rc = rx_config_check(cfg, &err);  // the ranges (rx_assign_plan_host.cpp), before any device call
  if (rc) return fail(rc, "%s", err.c_str());
  int ndev = 0;
  RX_HIP(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(RX_EINVAL, "device %d not present (%d devices)", cfg->device, ndev);
  RX_HIP(hipSetDevice(cfg->device));
  rx_env* h = new rx_env();
  h->cfg = *cfg;
  if (!(h->cfg.speed_weight == h->cfg.speed_weight)) h->cfg.speed_weight = 8.0;
  h->D = cfg->n_sensors + 4 + 4 * (cfg->n_agents - 1);
  // sensor angles = np.linspace(-c, c, n) (racing_env.py:45, multi_racing_env.py:50):
  // numpy computes start + i*step with step = (stop-start)/(n-1), and sets the
  // last element to stop exactly.
  {
    const int n = cfg->n_sensors;
    std::vector<double> rel(n);
    const double start = -cfg->sensor_half_cone, stop = cfg->sensor_half_cone;
    if (n == 1) {
      rel[0] = start;
    } else {
      const double div = (double)(n - 1);
      const double delta = stop - start;
      const double step = delta / div;
      for (int i = 0; i < n; ++i) rel[i] = (double)i * step + start;
      rel[n - 1] = stop;
    }
    h->rel_angles_h = rel;
    rc = upload(h->rel_angles, rel.data(), rel.size());
    if (rc) {
      delete h;
      return rc;
    }
  }
  *out = h;
  return RX_OK;
}

int rx_sensor_angles(const rx_env* h, double* out) {
  if (!h || !out) return fail(RX_EINVAL, "rx_sensor_angles: null argument");
  std::copy(h->rel_angles_h.begin(), h->rel_angles_h.end(), out);
  return RX_OK;
}

int rx_env_order(rx_env* h, int32_t* perm_out, int32_t* sort_bins, int32_t* sort_shift) {
  if (!h || !perm_out) return fail(RX_EINVAL, "rx_env_order: null argument");
  if (!h->assigned) return fail(RX_ESTATE, "rx_env_order before rx_assign");
  RX_HIP(hipSetDevice(h->cfg.device));
  RX_HIP(hipDeviceSynchronize());
  RX_HIP(hipMemcpy(perm_out, h->perm[0].p, (size_t)h->cfg.n_envs * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (sort_bins) *sort_bins = h->sched.sort_on ? h->sched.sort_bins : 0;
  if (sort_shift) *sort_shift = h->sched.sort_shift;
  return RX_OK;
}

// the split step applies (k_kin + k_step2): STEP mode, next-step or no autoreset,
// single-agent envs at one lane per env
static bool split_step(const rx_env* h, int mode) {
  return h->sched.split && mode == RX_MODE_STEP && (h->cfg.n_agents == 2 || h->sched.dyn_lpe == 1) &&
         h->cfg.autoreset != RX_AUTORESET_SAME_STEP && h->cs_scratch.p;
}

int rx_schedule(const rx_env* h, int32_t* out) {
  if (!h || !out) return fail(RX_EINVAL, "rx_schedule: null argument");
  if (!h->assigned) return fail(RX_ESTATE, "rx_schedule before rx_assign");
  rx_sched_row(h->cfg, h->sched, (int32_t)h->dyn_calls, out);
  return RX_OK;
}

int rx_destroy(rx_env* h) {
  if (!h) return RX_OK;
  (void)hipSetDevice(h->cfg.device);
  delete h;  // every buffer is a DevBuf member: it frees itself
  return RX_OK;
}

int rx_upload_tracks(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* nrm,
                     const double* seg, const double* meta) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (n_tracks <= 0 || !wp_off || !wp || !nrm || !seg || !meta) return fail(RX_EINVAL, "rx_upload_tracks: bad arguments");
  if (wp_off[0] != 0) return fail(RX_EINVAL, "wp_off[0] must be 0");
  for (int k = 0; k < n_tracks; ++k) {
    const int W = wp_off[k + 1] - wp_off[k];
    if (W < 2) return fail(RX_EINVAL, "track %d has %d waypoints (need >= 2)", k, W);
    if (W > 64 * RX_WP_CHUNK * RX_WP_SUPER)  // closest-waypoint super-chunk mask is 64 bits
      return fail(RX_EINVAL, "track %d has %d waypoints (at most %d)", k, W, 64 * RX_WP_CHUNK * RX_WP_SUPER);
    if (!(meta[8 * k + 3] >= 0)) return fail(RX_EINVAL, "track %d width invalid", k);
    if (!(meta[8 * k + 4] > 0)) return fail(RX_EINVAL, "track %d max_track_distance must be > 0", k);
  }
  const size_t Wt = (size_t)wp_off[n_tracks];
  RX_HIP(hipSetDevice(h->cfg.device));
  int rc;
  if ((rc = upload(h->wp_off, wp_off, (size_t)n_tracks + 1))) return rc;
  if ((rc = upload(h->wp, wp, 2 * Wt))) return rc;
  if ((rc = upload(h->nrm, nrm, 2 * Wt))) return rc;
  if ((rc = upload(h->seg, seg, 8 * Wt))) return rc;
  if ((rc = upload(h->meta, meta, 8 * (size_t)n_tracks))) return rc;
  // the culling tables, the per-slot headers and the float32 copy of the segments (nearest
  // rounding; the kernel's error bound covers it)
  if ((rc = build_chunks(h, n_tracks, wp_off, wp, seg, meta))) return rc;
  h->wp_off_h.assign(wp_off, wp_off + n_tracks + 1);
  h->n_tracks = n_tracks;
  h->assigned = false;  // slots may have changed meaning: require rx_assign again
  return RX_OK;
}

static int sync_state(rx_env* h, int to_user, void* stream = nullptr, bool blocking = true);

// check -> plan -> upload -> commit.  The plan (rx_plan_assignment, host only) is computed into
// locals; a refusal returns with the handle as it was.  `assigned` is cleared before the first
// upload and the schedule is written only after the last, so a failed upload leaves a handle that
// refuses to step, not one with new lane counts beside old wave tables.  upload keeps a large
// enough buffer at its address (captured graphs and rx_replace_tracks_device rely on it).
int rx_assign(rx_env* h, const int32_t* track_of_env) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (h->n_tracks <= 0) return fail(RX_ESTATE, "rx_assign before rx_upload_tracks");
  if (!track_of_env) return fail(RX_EINVAL, "track_of_env is null");
  const int N = h->cfg.n_envs, A = h->cfg.n_agents, R = h->cfg.n_sensors;
  rx_assignment plan;
  std::string err;
  int rc = rx_plan_assignment(h->cfg, h->n_tracks, h->wp_off_h.data(), track_of_env, &plan, &err, h->lane_cars);
  if (rc) return fail(rc, "%s", err.c_str());
  const rx_sched& sc = plan.sched;
  RX_HIP(hipSetDevice(h->cfg.device));
  h->assigned = false;
  if ((rc = upload(h->slot_n, plan.slot_n.data(), plan.slot_n.size()))) return rc;
  if ((rc = upload(h->perm[0], plan.perm.data(), plan.perm.size()))) return rc;
  if ((rc = upload(h->perm[1], plan.perm.data(), plan.perm.size()))) return rc;
  if (A == 2) {
    std::vector<uint32_t> z(N, 0u);
    if ((rc = upload(h->resets, z.data(), z.size()))) return rc;
  }
  if (sc.lane_tracks) {  // the kernels read each position's slot: the order stays fixed
    if ((rc = upload(h->pos_slot, plan.pos_slot.data(), plan.pos_slot.size()))) return rc;
    if ((rc = upload(h->env_pos, plan.env_pos.data(), plan.env_pos.size()))) return rc;
    if (A == 1) {  // rx_regroup_slots' buffers: here, so the call itself may run under capture
      if ((rc = reserve(h->regroup_scratch, rx_regroup_scratch_size(N)))) return rc;
      if ((rc = reserve(h->regroup_src, (size_t)N)) || (rc = reserve(h->regroup_slot, (size_t)N))) return rc;
    }
  } else if (sc.sort_on) {  // the spatial re-sort's bins, keys and counters
    const size_t total = (size_t)sc.sort_bins;
    std::vector<uint32_t> zk(std::max<size_t>((size_t)N, total), 0u);
    if ((rc = upload(h->sort_base, plan.sort_base.data(), plan.sort_base.size()))) return rc;
    if ((rc = upload(h->keys_in, zk.data(), (size_t)N))) return rc;
    if ((rc = upload(h->keys_off, zk.data(), (size_t)N))) return rc;
    if ((rc = upload(h->sort_hist, zk.data(), total))) return rc;
    if ((rc = upload(h->sort_cursor, zk.data(), total))) return rc;
  }
  if (h->cfg.ray_order == 2) {  // task ids before the first sort: position-major, (agent, ray) minor -- a valid order
    const size_t nt = (size_t)N * A * R;
    std::vector<int32_t> t0(nt);
    for (size_t o = 0; o < nt; ++o) t0[o] = (int32_t)o;  // task id (A*p + q)*R + r at slot p*A*R + q*R + r
    if ((rc = upload(h->tasks, t0.data(), nt))) return rc;
  }
  {
    std::vector<double> z(2 * (size_t)N * A, 0.0);
    if ((rc = upload(h->cs_scratch, z.data(), z.size()))) return rc;
  }
  // the carrying schedule's snapshots (single-agent; here, not in rx_steps: it may run under capture)
  if (RX_STEPS_CARRY && A == 1) {
    const std::vector<double> zd(3 * (size_t)N, 0.0);
    const std::vector<int32_t> zi((size_t)N * R, 0);
    const std::vector<float> zf((size_t)N * h->D, 0.0f);
    for (int b = 0; b < RX_PAIR_RING; ++b)
      if ((rc = upload(h->snap_pose[b], zd.data(), zd.size()))) return rc;
    for (int b = 0; b < RX_TASK_RING && h->cfg.ray_order == 2; ++b)
      if ((rc = upload(h->snap_tasks[b], zi.data(), zi.size()))) return rc;
    for (int b = 0; b < RX_SHADOW_ROWS; ++b)
      if ((rc = upload(h->obs_shadow[b], zf.data(), zf.size()))) return rc;
    for (int b = 0; b < RX_CROSS_RING && RX_STEPS_CROSS && sc.sort_on; ++b) {  // the crossing step's
      if ((rc = upload(h->snap_rows[b], zi.data(), (size_t)N))) return rc;
      if ((rc = upload(h->snap_hint[b], zd.data(), (size_t)N))) return rc;
    }
  }
  if ((rc = upload(h->dyn_waves, plan.dyn.data(), plan.dyn.size()))) return rc;
  if ((rc = upload(h->ray_waves, plan.ray.data(), plan.ray.size()))) return rc;
  if (!h->policy_frag.p) {  // allocated here, not in rx_rollout_steps: it may run inside a graph capture
    RX_HIP(hipSetDevice(h->cfg.device));
    if (hipMalloc(&h->policy_frag.p, rx_policy_frag_bytes()) != hipSuccess)
      return fail(RX_ENOMEM, "rx_assign: policy fragment image");
    h->policy_frag.n = rx_policy_frag_bytes();
  }
  h->ray_waves_h.swap(plan.ray);
  h->sched = sc;
  h->assigned = true;
  h->tasks_stale = true;
  h->sort_pending = false;
  h->sort_hist_done = false;  // the histogram was re-uploaded as zeros above (or sorting is off)
  if (h->bound && h->st.track) RX_HIP(hipMemcpy(h->st.track, track_of_env, N * sizeof(int32_t), hipMemcpyHostToDevice));
  if (h->bound) return sync_state(h, 0);  // the new wave order: re-read the caller's arrays
  return RX_OK;
}

int rx_set_lane_cars(rx_env* h, int32_t mode) {
  if (!h) return fail(RX_EINVAL, "rx_set_lane_cars: null handle");
  if (mode < -1 || mode > 1) return fail(RX_EINVAL, "rx_set_lane_cars: lane_cars must be 0 (auto), 1 or -1 (got %d)", mode);
  if (h->cfg.n_agents != 2)
    return fail(RX_EINVAL, "rx_set_lane_cars: a single-agent handle: rx_config.lane_tracks governs its schedule");
  h->lane_cars = mode;  // resolved by the next rx_assign
  return RX_OK;
}

// rx_assign_plan / rx_assign_plan_cars (fn names the entry in the texts)
static int assign_plan(const char* fn, const rx_config* cfg, int32_t lane_cars, int32_t n_tracks, const int32_t* wp_off,
                       const int32_t* track_of_env, rx_assign_plan_io* io) {
  if (n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n_tracks);
  for (int k = 0; k < n_tracks; ++k)
    if (wp_off[k + 1] - wp_off[k] < 2)
      return fail(RX_EINVAL, "track %d has %d waypoints (need >= 2)", k, wp_off[k + 1] - wp_off[k]);
  rx_assignment plan;
  std::string err;
  const int rc = rx_plan_assignment(*cfg, n_tracks, wp_off, track_of_env, &plan, &err, lane_cars);
  if (rc) return fail(rc, "%s", err.c_str());
  const rx_sched& sc = plan.sched;
  const bool room = io->schedule && io->perm && io->dyn_waves && io->ray_waves && io->dyn_cap >= sc.n_dyn_waves &&
                    io->ray_cap >= sc.n_ray_waves;
  io->n_dyn_waves = sc.n_dyn_waves;
  io->n_ray_waves = sc.n_ray_waves;
  if (!room) return RX_OK;  // the sizes only
  rx_sched_row(*cfg, sc, 0, io->schedule);
  std::copy(plan.perm.begin(), plan.perm.end(), io->perm);
  io->sort_bins = sc.sort_bins;
  io->sort_shift = sc.sort_shift;
  static_assert(sizeof(rx_wave) == 4 * sizeof(int32_t), "wave records are int32 [4]");
  if (!plan.dyn.empty()) memcpy(io->dyn_waves, plan.dyn.data(), plan.dyn.size() * sizeof(rx_wave));
  if (!plan.ray.empty()) memcpy(io->ray_waves, plan.ray.data(), plan.ray.size() * sizeof(rx_wave));
  if (io->slot_n) std::copy(plan.slot_n.begin(), plan.slot_n.end(), io->slot_n);
  if (io->pos_slot) std::copy(plan.pos_slot.begin(), plan.pos_slot.end(), io->pos_slot);
  if (io->env_pos) std::copy(plan.env_pos.begin(), plan.env_pos.end(), io->env_pos);
  if (io->sort_base) std::copy(plan.sort_base.begin(), plan.sort_base.end(), io->sort_base);
  return RX_OK;
}

int rx_assign_plan(const rx_config* cfg, int32_t n_tracks, const int32_t* wp_off, const int32_t* track_of_env,
                   rx_assign_plan_io* io) {
  if (!cfg || !wp_off || !track_of_env || !io) return fail(RX_EINVAL, "rx_assign_plan: null argument");
  return assign_plan("rx_assign_plan", cfg, -1, n_tracks, wp_off, track_of_env, io);
}

int rx_assign_plan_cars(const rx_config* cfg, int32_t lane_cars, int32_t n_tracks, const int32_t* wp_off,
                        const int32_t* track_of_env, rx_assign_plan_io* io) {
  if (!cfg || !wp_off || !track_of_env || !io) return fail(RX_EINVAL, "rx_assign_plan_cars: null argument");
  if (cfg->n_agents == 1)
    return fail(RX_EINVAL, "rx_assign_plan_cars: n_agents = 1: rx_config.lane_tracks governs a single-agent schedule "
                           "(rx_assign_plan)");
  return assign_plan("rx_assign_plan_cars", cfg, lane_cars, n_tracks, wp_off, track_of_env, io);
}

// working copy <-> the caller's arrays (env order); blocking = finish before
// returning (bind / assign), else enqueued on the caller's stream
static int sync_state(rx_env* h, int to_user, void* stream, bool blocking) {
  if (!h->bound || !h->assigned) return fail(RX_ESTATE, "state sync needs rx_bind_state and rx_assign");
  RX_HIP(hipSetDevice(h->cfg.device));
  rx_state user = h->st, work = h->work;
  if (!user.finished_step) work.finished_step = nullptr;  // A == 1 without the array: nothing to move
  int rc = rx_state_sync(&work, &user, h->perm[0].p, h->cfg.n_envs, h->cfg.n_agents, to_user, (hipStream_t)stream);
  if (rc) return fail(RX_EHIP, "state sync failed: %s", hipGetErrorString((hipError_t)rc));
  if (blocking) RX_HIP(hipDeviceSynchronize());
  return RX_OK;
}

int rx_bind_state(rx_env* h, const rx_state* st) {
  if (!h || !st) return fail(RX_EINVAL, "rx_bind_state: null argument");
  if (!st->x || !st->y || !st->angle || !st->vx || !st->vy || !st->progress || !st->last_progress ||
      !st->last_steering || !st->flags || !st->steps || !st->track || !st->env_flags || !st->ep_return ||
      !st->ep_length)
    return fail(RX_EINVAL, "rx_bind_state: every state array except finished_step is required");
  if (h->cfg.n_agents == 2 && !st->finished_step) return fail(RX_EINVAL, "rx_bind_state: finished_step required for 2 agents");
  h->st = *st;
  if (!h->work.x) {  // working copy + shadow, same shapes as the caller's arrays
    const size_t N = (size_t)h->cfg.n_envs, NA = N * (size_t)h->cfg.n_agents;
    int used = 0;  // RX_WORK_ARRAYS arrays per state
    for (rx_state* w : {&h->work, &h->work_tmp}) {
      auto alloc = [&](auto** ptr, size_t bytes) -> int {
        DevBuf<uint8_t>& m = h->work_mem[used++];
        if (hipMalloc(&m.p, std::max<size_t>(bytes, 16)) != hipSuccess) {
          m.p = nullptr;
          return fail(RX_ENOMEM, "working state alloc");
        }
        m.n = std::max<size_t>(bytes, 16);
        RX_HIP(hipMemset(m.p, 0, m.n));
        *ptr = reinterpret_cast<std::remove_reference_t<decltype(*ptr)>>(m.p);
        return RX_OK;
      };
      int rc;
      for (double** f : {&w->x, &w->y, &w->angle, &w->vx, &w->vy, &w->progress, &w->last_progress, &w->last_steering})
        if ((rc = alloc(f, NA * sizeof(double)))) return rc;
      if ((rc = alloc(&w->flags, NA))) return rc;
      if ((rc = alloc(&w->finished_step, NA * sizeof(int32_t)))) return rc;
      if ((rc = alloc(&w->steps, N * sizeof(int32_t)))) return rc;
      if ((rc = alloc(&w->env_flags, N))) return rc;
      if ((rc = alloc(&w->ep_return, N * sizeof(double)))) return rc;
      if ((rc = alloc(&w->ep_length, N * sizeof(int32_t)))) return rc;
    }
  }
  h->bound = true;
  if (h->assigned) return sync_state(h, 0);
  return RX_OK;
}

int rx_state_import(rx_env* h, void* stream) {
  if (!h) return fail(RX_EINVAL, "null handle");
  return sync_state(h, 0, stream, false);
}

int rx_state_export(rx_env* h, void* stream) {
  if (!h) return fail(RX_EINVAL, "null handle");
  return sync_state(h, 1, stream, false);
}

int rx_set_speed_weight(rx_env* h, double w) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (!(w == w)) return fail(RX_EINVAL, "speed_weight is NaN");
  h->cfg.speed_weight = w;
  return RX_OK;
}

// rx_profile: give the next launch its stamp record (nullptr when not
// profiling or the record is full).
static constexpr int kProfMax = 512;  // launches per record
static int prof_stride(const rx_env* h) {
  const int wide = h->cfg.n_envs * h->cfg.n_agents * h->cfg.n_sensors;  // k_rays_wide: one wave per ray
  return std::max(h->sched.reward_lpe * ((h->sched.n_dyn_waves + 7) / 8 * 8) + h->sched.n_ray_waves, wide) + 8;
}
static void prof_arm(rx_env* h, rx_kargs& a, int kind) {
  a.prof_ts = nullptr;
  if (!h->prof || !h->prof_buf.p || (int)h->prof_kinds.size() >= kProfMax) return;
  a.prof_stride = prof_stride(h);
  a.prof_ts = h->prof_buf.p + (size_t)h->prof_kinds.size() * 2 * a.prof_stride;
  h->prof_kinds.push_back(kind);
}

void make_kargs(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, rx_kargs& a) {
  a.tr = rx_track_view{h->wp_off.p,    h->wp.p,        h->nrm.p,      h->seg.p,        h->meta.p,
                       h->chunk_off.p, h->chunk_box.p, h->slot_geo.p, h->wchunk_off.p, h->wchunk_box.p,
                       h->super_off.p, h->super_box.p, h->wsuper_off.p, h->wsuper_box.p,
                       h->chunk_box_f.p, h->super_box_f.p, h->n_chunk_boxes, h->n_super_boxes, h->seg_f.p,
                       h->slot_hdr.p};
  a.st = h->work;
  a.st.track = h->st.track;                // read-only, env order
  a.st.speed_weight = h->st.speed_weight;  // read-only, env order (or nullptr)
  a.io = *io;
  a.dyn_waves = h->dyn_waves.p;
  a.ray_waves = h->ray_waves.p;
  a.perm = h->perm[0].p;
  a.rel_angles = h->rel_angles.p;
  a.reset_mask = mask;
  a.n_dyn_waves = h->sched.n_dyn_waves;
  a.n_ray_waves = h->sched.n_ray_waves;
  a.n_sensors = h->cfg.n_sensors;
  a.D = h->D;
  a.max_steps = h->cfg.max_steps;
  a.autoreset = h->cfg.autoreset;
  a.mode = mode;
  a.cull_chunk = h->chunk_box.p ? h->cfg.cull_chunk : 0;
  a.cull_super = h->super_box.p ? h->cfg.cull_super : 0;
  a.speed_weight = h->cfg.speed_weight;
  a.seed = h->cfg.seed;
  a.reset_count = h->resets.p;
  a.ray_order = h->cfg.ray_order;
  a.dyn_lpe = h->sched.dyn_lpe;
  a.ray_lpr = h->sched.ray_lpr;
  a.ray_tail_from = h->sched.ray_tail_from;
  a.ray_tail_lpr = h->sched.ray_tail_lpr;
  a.reward_lpe = h->sched.reward_lpe;
  a.argmin_window = h->sched.argmin_window;
  a.slot_nenv = h->slot_n.p;
  a.wide = h->sched.dyn_lpe == 64;
  a.n_wide_tasks = h->cfg.n_envs * h->cfg.n_agents * h->cfg.n_sensors;
  a.tasks = h->tasks.p;
  a.tasks_out = (h->cfg.ray_order == 2 && !a.wide && !h->sched.lane_tracks) ? h->tasks.p : nullptr;
  a.lane_tracks = h->sched.lane_tracks;
  a.pos_slot = h->sched.lane_tracks ? h->pos_slot.p : nullptr;
  a.cs_scratch = h->cs_scratch.p;
  a.ray_x = a.st.x;  // the ray inputs: the working state (rx_steps' carrying launches: a snapshot)
  a.ray_y = a.st.y;
  a.ray_angle = a.st.angle;
  a.ray_hint = a.st.progress;  // (a crossing step of rx_steps: the hint snapshot)
  a.sort_base = h->sort_base.p;
  a.sort_shift = h->sched.sort_shift;
  a.box_quadrants = h->cfg.box_quadrants >= 0;
  a.seg_filter = h->cfg.seg_filter >= 0;
#ifdef RX_AB_NO_EPSTATS  // A/B build only (tools/build_rev.py): drop the episode-statistics atomics
  a.io.ep_stats = nullptr;
#endif
}

// The bookkeeping of a dynamics launch, shared by launch() and rx_steps' carrying schedule
// (steps_pair), which advances it as K x rx_step would.
// The ray-task order only steers which rays share a wave (results never depend on it): a KIN
// part may reuse the previous one's while the blocks hold the same envs.  Does the next KIN
// part sort its ray tasks?  (Asked only where tasks_out is non-null.)
static bool task_sort_due(const rx_env* h) {
  return h->tasks_stale || (h->task_calls % (uint64_t)h->sched.task_sort) == 0;
}
// ... and the same for the KIN part being armed now, which takes its turn
static bool take_task_sort_turn(rx_env* h) {
  const bool due = task_sort_due(h);
  if (due) h->tasks_stale = false;
  ++h->task_calls;
  return due;
}
// Spatial re-sort, every sort_interval dynamics launches (dyn_calls counts them only while
// the re-sort is on): is it due `ahead` dynamics launches from now?
static bool resort_on(const rx_env* h) { return h->cfg.sort_interval > 0 && h->sched.sort_on; }
static bool resort_due(const rx_env* h, int32_t ahead) {
  return resort_on(h) && ((h->dyn_calls + ahead) % h->cfg.sort_interval) == 0;
}
// The REWARD half (or k_dyn) of the re-sort step writes the sort keys; with `hist` (single
// agent, split step) it also builds the re-sort's histogram and each env's rank in its bin,
// one launch fewer per re-sort: rx_sort_envs skips k_sort_hist.  The histogram is zero
// unless sort_hist_done, when it holds the counts of the keys this launch is about to
// overwrite (keys requested again before their sort ran: rx_step_phases(1) twice, or a reset
// in between): clear it, so the fused count, or k_sort_hist, starts from zero.
static int arm_sort_keys(rx_env* h, rx_kargs& a, bool hist, hipStream_t s) {
  if (h->sort_hist_done) {
    RX_HIP(hipMemsetAsync(h->sort_hist.p, 0, (size_t)h->sched.sort_bins * sizeof(uint32_t), s));
    h->sort_hist_done = false;
  }
  a.sort_keys = h->keys_in.p;
  if (hist) {
    a.sort_hist = h->sort_hist.p;
    a.sort_off = h->keys_off.p;
    h->sort_hist_done = true;
  }
  return RX_OK;
}
// The sort itself, which moves the working-state rows: after the raycast of the step whose
// keys it reads (the ray tasks name positions), so the new order applies from the next step.
static int sort_envs_now(rx_env* h, hipStream_t s) {
  const int hist_done = h->sort_hist_done ? 1 : 0;
  h->sort_hist_done = false;
  h->tasks_stale = true;  // the re-sort moves envs between blocks
  rx_state work = h->work, tmp = h->work_tmp;
  const int rc = rx_sort_envs(h->keys_in.p, h->keys_off.p, h->cfg.n_envs, h->cfg.n_agents, h->sort_hist.p,
                              h->sort_cursor.p, h->sched.sort_bins, h->perm[0].p, h->perm[1].p, &work, &tmp, s, hist_done);
  if (rc != 0) return fail(RX_EHIP, "spatial sort failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// ---- positions regrouped by slot (ABI v25, additive; DESIGN.md §3 "Positions regrouped by slot")
int32_t rx_regroup_plan_host(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot,
                             int32_t* src_out, int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out) {
  std::string err;
  const int rc = rx_plan_regroup(n, n_tracks, perm, pos_slot, src_out, perm_out, pos_slot_out, env_pos_out, &err);
  return rc ? fail(rc, "%s", err.c_str()) : RX_OK;
}

int64_t rx_regroup_scratch_bytes(int32_t n, int32_t n_tracks) {
  if (n < 0 || n_tracks <= 0) return -1;
  return (int64_t)rx_regroup_scratch_size(n);
}

int rx_regroup_plan(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot, int32_t* src_out,
                    int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out, void* scratch,
                    int64_t scratch_bytes, void* stream) {
  const char* fn = "rx_regroup_plan";
  if (n < 0) return fail(RX_EINVAL, "%s: n must be >= 0 (got %d)", fn, n);
  if (n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n_tracks);
  const void* ptrs[] = {perm, pos_slot, src_out, perm_out, pos_slot_out, env_pos_out, scratch};
  const char* names[] = {"perm", "pos_slot", "src_out", "perm_out", "pos_slot_out", "env_pos_out", "scratch"};
  for (int i = 0; i < 7; ++i)
    if (!ptrs[i]) return fail(RX_EINVAL, "%s: null %s", fn, names[i]);
  if (scratch_bytes < (int64_t)rx_regroup_scratch_size(n))
    return fail(RX_EINVAL, "%s: scratch of %lld bytes, rx_regroup_scratch_bytes(%d, %d) = %lld", fn,
                (long long)scratch_bytes, n, n_tracks, (long long)rx_regroup_scratch_size(n));
  if ((uintptr_t)scratch % sizeof(uint32_t)) return fail(RX_EINVAL, "%s: scratch must be 4-byte aligned", fn);
  return launched(fn, rx_launch_regroup_plan(n, n_tracks, perm, pos_slot, src_out, perm_out, pos_slot_out,
                                             env_pos_out, scratch, (hipStream_t)stream));
}

// the handles the two entries below take: single-agent on the lane-varying schedule
static int regroup_handle(const char* fn, const rx_env* h) {
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (h->n_tracks <= 0) return fail(RX_ESTATE, "%s: no track table (rx_upload_tracks)", fn);
  if (!h->assigned) return fail(RX_ESTATE, "%s: no env assignment (rx_assign)", fn);
  if (!h->bound) return fail(RX_ESTATE, "%s: no state bound (rx_bind_state)", fn);
  if (h->cfg.n_agents != 1)
    return fail(RX_EINVAL, "%s: a two-car handle: its schedule binds every wave to one slot (no plan resolves "
                           "two-car envs to the lane-varying schedule), and rx_assign is its regroup", fn);
  if (!h->sched.lane_tracks)
    return fail(RX_EINVAL, "%s: the handle's schedule is not lane-varying: the grouped and wide schedules bind "
                           "waves to slots and rx_assign is their regroup (rx_config.lane_tracks = 1)", fn);
  return RX_OK;
}

// Plan from the live perm and pos_slot (the new perm into the shadow perm[1], env_pos rewritten in
// place: the plan does not read it), gather the working rows into work_tmp by src, copy back.  Launches
// only, on the caller's stream, into buffers rx_assign reserved: capturable, and every buffer the step,
// rollout and episodic kernels read keeps its address.  Between calls that step the env nothing else is
// indexed by position on this schedule (the pose snapshots and task rows of rx_steps live for one call;
// the ray tasks are position-major and never re-ranked).
int rx_regroup_slots(rx_env* h, void* stream) {
  const char* fn = "rx_regroup_slots";
  int rc = regroup_handle(fn, h);
  if (rc) return rc;
  const int N = h->cfg.n_envs;
  if (!h->regroup_scratch.p || h->regroup_src.n < (size_t)N || h->regroup_slot.n < (size_t)N)
    return fail(RX_ESTATE, "%s: no scratch (rx_assign reserves it)", fn);
  const hipStream_t s = (hipStream_t)stream;
  if ((rc = rx_launch_regroup_plan(N, h->n_tracks, h->perm[0].p, h->pos_slot.p, h->regroup_src.p, h->perm[1].p,
                                   h->regroup_slot.p, h->env_pos.p, h->regroup_scratch.p, s)) != 0)
    return launched(fn, rc);
  rx_state work = h->work, tmp = h->work_tmp;
  return launched(fn, rx_launch_regroup_move(N, h->regroup_src.p, h->perm[1].p, h->perm[0].p, h->regroup_slot.p,
                                             h->pos_slot.p, &work, &tmp, s));
}

int rx_lane_layout(rx_env* h, int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out) {
  const char* fn = "rx_lane_layout";
  if (!perm_out || !pos_slot_out || !env_pos_out)
    return fail(RX_EINVAL, "%s: null %s", fn, !perm_out ? "perm_out" : !pos_slot_out ? "pos_slot_out" : "env_pos_out");
  const int rc = regroup_handle(fn, h);
  if (rc) return rc;
  const size_t bytes = (size_t)h->cfg.n_envs * sizeof(int32_t);
  RX_HIP(hipSetDevice(h->cfg.device));
  RX_HIP(hipDeviceSynchronize());
  RX_HIP(hipMemcpy(perm_out, h->perm[0].p, bytes, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(pos_slot_out, h->pos_slot.p, bytes, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(env_pos_out, h->env_pos.p, bytes, hipMemcpyDeviceToHost));
  return RX_OK;
}

int launch(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, void* stream, int phases) {
  if (phases < 1 || phases > 3) return fail(RX_EINVAL, "phases must be 1, 2 or 3 (got %d)", phases);
  if (!h) return fail(RX_EINVAL, "null handle");
  if (!io) return fail(RX_EINVAL, "io is null");
  if (h->n_tracks <= 0) return fail(RX_ESTATE, "no track table (rx_upload_tracks)");
  if (!h->assigned) return fail(RX_ESTATE, "no env assignment (rx_assign)");
  if (!h->bound) return fail(RX_ESTATE, "no state bound (rx_bind_state)");
  if (!io->obs) return fail(RX_EINVAL, "io->obs is required");
  if (mode == RX_MODE_STEP && !io->actions) return fail(RX_EINVAL, "io->actions is required");
  rx_kargs a{};
  make_kargs(h, io, mode, mask, a);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  // Split step: k_kin1 / k_kin2 (resets, kinematics, [car-car contact,]
  // non-ray obs, ray-task sort), then k_step2<A> = the REWARD part (argmins,
  // collision, reward, done) side by side with the raycast in ONE launch.  STEP
  // with next-step or no autoreset; single-agent envs at one lane per env
  // (same-step autoreset needs done before the observation; explicit resets
  // and small single-agent N use the one-kernel path).
  const int A = h->cfg.n_agents;
  // rx_set_start_draws: rank the envs this launch's dynamics kernel resets (env order)
  if (h->draws && A == 2 && (phases & RX_PHASE_DYNAMICS) &&
      (mode == RX_MODE_RESET || h->cfg.autoreset == RX_AUTORESET_NEXT_STEP)) {
    if ((rc = rx_launch_reset_rank(h->cfg.n_envs, mode, mask, a.st.env_flags, a.perm, h->draw_tmp.p, h->draw_rank.p,
                                   h->draw_cursor, h->draw_base.p, h->n_draws, s)) != 0)
      return fail(RX_EHIP, "k_reset_rank launch failed: %s", hipGetErrorString((hipError_t)rc));
    a.draws = h->draws;
    a.n_draws = h->n_draws;
    a.draw_base = h->draw_base.p;
    a.reset_rank = h->draw_rank.p;
  }
  const bool split = split_step(h, mode);
  const bool dyn = (phases & RX_PHASE_DYNAMICS) != 0;
  if (dyn && a.tasks_out && !take_task_sort_turn(h)) a.tasks_out = nullptr;
  // the re-sort step: its keys are armed below, for the launch that writes them (the two-car
  // REWARD half and k_dyn count no bins); the sort runs after the step's raycast, which
  // rx_step_phases may ask for in a later call (sort_pending)
  const bool resort = dyn && resort_due(h, 0);
  if (dyn && resort_on(h)) ++h->dyn_calls;
  if (resort) h->sort_pending = true;
  if (split) {
    if (dyn) {
      prof_arm(h, a, RX_KERNEL_KIN);
      if ((rc = rx_launch_split(&a, A, RX_SPLIT_KIN, s)) != 0)
        return fail(RX_EHIP, "k_kin1 launch failed: %s", hipGetErrorString((hipError_t)rc));
      a.tasks_out = nullptr;
      if (resort && (rc = arm_sort_keys(h, a, A == 1, s)) != 0) return rc;
      prof_arm(h, a, phases == 3 ? RX_KERNEL_STEP2 : RX_KERNEL_REWARD);
      if ((rc = rx_launch_split(&a, A, phases == 3 ? RX_SPLIT_REWARD_RAYS : RX_SPLIT_REWARD, s)) != 0)
        return fail(RX_EHIP, "k_step2 launch failed: %s", hipGetErrorString((hipError_t)rc));
    } else {
      a.tasks_out = nullptr;
      prof_arm(h, a, RX_KERNEL_RAYS);
      if ((rc = rx_launch_step(&a, A, RX_PHASE_RAYS, s)) != 0)
        return fail(RX_EHIP, "k_rays launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
  } else {
    if (dyn) {
      if (resort && (rc = arm_sort_keys(h, a, false, s)) != 0) return rc;
      prof_arm(h, a, RX_KERNEL_DYN);
      if ((rc = rx_launch_step(&a, h->cfg.n_agents, RX_PHASE_DYNAMICS, s)) != 0)
        return fail(RX_EHIP, "k_dyn launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (phases & RX_PHASE_RAYS) {
      a.sort_keys = nullptr;
      a.tasks_out = nullptr;
      prof_arm(h, a, RX_KERNEL_RAYS);
      if ((rc = rx_launch_step(&a, h->cfg.n_agents, RX_PHASE_RAYS, s)) != 0)
        return fail(RX_EHIP, "k_rays launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
  }
  if (h->sort_pending && (phases & RX_PHASE_RAYS)) {
    h->sort_pending = false;
    if ((rc = sort_envs_now(h, s)) != 0) return rc;
  }
  return RX_OK;
}

int rx_profile(rx_env* h, int32_t enable) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (enable == 1) {  // a fresh record, all stamps 0 (= no wave)
    if (!h->assigned) return fail(RX_ESTATE, "rx_profile before rx_assign");
    RX_HIP(hipSetDevice(h->cfg.device));
    RX_HIP(hipDeviceSynchronize());  // no launch of the previous record may still write
    const size_t n = (size_t)kProfMax * 2 * prof_stride(h);
    if (h->prof_buf.n < n) {
      h->prof_buf.release();
      if (hipMalloc(&h->prof_buf.p, n * sizeof(unsigned long long)) != hipSuccess)
        return fail(RX_ENOMEM, "rx_profile: stamp buffer alloc");
      h->prof_buf.n = n;
    }
    RX_HIP(hipMemset(h->prof_buf.p, 0, n * sizeof(unsigned long long)));
    h->prof_kinds.clear();
  }
  h->prof = enable != 0;  // 2 = resume the current record
  return RX_OK;
}

int rx_profile_read(rx_env* h, double* mean_ms, int32_t* count) {
  if (!h || !mean_ms || !count) return fail(RX_EINVAL, "rx_profile_read: null argument");
  double sum[RX_KERNEL_KINDS] = {0};
  int32_t n[RX_KERNEL_KINDS] = {0};
  const size_t nl = h->prof_kinds.size();
  if (nl) {
    RX_HIP(hipSetDevice(h->cfg.device));
    int khz = 0;
    RX_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device));
    if (khz <= 0) return fail(RX_EHIP, "rx_profile_read: no wall-clock rate");
    RX_HIP(hipDeviceSynchronize());
    const int stride = prof_stride(h);
    std::vector<unsigned long long> st(nl * 2 * stride);
    RX_HIP(hipMemcpy(st.data(), h->prof_buf.p, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < nl; ++l) {
      const unsigned long long* r = st.data() + l * 2 * stride;
      unsigned long long t0 = ~0ull, t1 = 0;
      for (int i = 0; i < stride; ++i) {
        if (r[i]) t0 = std::min(t0, r[i]);
        t1 = std::max(t1, r[stride + i]);
      }
      if (t1 == 0 || t0 == ~0ull || t1 < t0) continue;  // launch with no waves
      sum[h->prof_kinds[l]] += (double)(t1 - t0) / (double)khz;  // ticks / kHz = ms
      ++n[h->prof_kinds[l]];
    }
  }
  for (int k = 0; k < RX_KERNEL_KINDS; ++k) {
    mean_ms[k] = n[k] ? sum[k] / n[k] : 0.0;
    count[k] = n[k];
  }
  return RX_OK;
}

int rx_profile_waves(rx_env* h, int32_t launch, uint64_t* start, uint64_t* end, int32_t cap, int32_t* n_waves,
                     int32_t* kind, int32_t* khz) {
  if (!h || !start || !end || !n_waves || !kind || !khz) return fail(RX_EINVAL, "rx_profile_waves: null argument");
  if (launch < 0 || (size_t)launch >= h->prof_kinds.size())
    return fail(RX_EINVAL, "rx_profile_waves: launch %d not recorded (%d in the record)", launch,
                (int)h->prof_kinds.size());
  if (cap < 0) return fail(RX_EINVAL, "rx_profile_waves: cap %d < 0", cap);
  RX_HIP(hipSetDevice(h->cfg.device));
  RX_HIP(hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, h->cfg.device));
  RX_HIP(hipDeviceSynchronize());
  const int stride = prof_stride(h);
  const int n = std::min(stride, cap);
  const unsigned long long* r = h->prof_buf.p + (size_t)launch * 2 * stride;
  if (n > 0) {
    RX_HIP(hipMemcpy(start, r, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(end, r + stride, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  *n_waves = stride;
  *kind = h->prof_kinds[launch];
  return RX_OK;
}

int rx_ray_waves(const rx_env* h, int32_t* out, int32_t cap, int32_t* n_waves) {
  if (!h || !n_waves || (cap > 0 && !out)) return fail(RX_EINVAL, "rx_ray_waves: null argument");
  if (!h->assigned) return fail(RX_ESTATE, "rx_ray_waves before rx_assign");
  const size_t n = h->ray_waves_h.size();
  for (size_t i = 0; i < n && (int64_t)i < (int64_t)cap; ++i) {
    const rx_wave& w = h->ray_waves_h[i];
    out[4 * i + 0] = w.track;
    out[4 * i + 1] = w.perm_start;
    out[4 * i + 2] = w.task_start;
    out[4 * i + 3] = w.count;
  }
  *n_waves = (int32_t)n;
  return RX_OK;
}

int rx_ray_tasks(rx_env* h, int32_t* out, int64_t cap, int64_t* n, void* stream) {
  if (!h || !n || (cap > 0 && !out)) return fail(RX_EINVAL, "rx_ray_tasks: null argument");
  if (!h->assigned) return fail(RX_ESTATE, "rx_ray_tasks before rx_assign");
  const int64_t len = std::min<int64_t>((int64_t)h->tasks.n,
                                        (int64_t)h->cfg.n_envs * h->cfg.n_agents * h->cfg.n_sensors);
  *n = len;
  if (cap <= 0) return RX_OK;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(out, h->tasks.p, (size_t)std::min(cap, len) * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(RX_EHIP, "rx_ray_tasks: copy failed");
  return RX_OK;
}

int rx_set_start_draws(rx_env* h, const uint32_t* draws, int64_t n_draws, int64_t* cursor) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (!draws) {
    h->draws = nullptr, h->n_draws = 0, h->draw_cursor = nullptr;
    return RX_OK;
  }
  if (h->cfg.n_agents != 2) return fail(RX_EINVAL, "rx_set_start_draws: single-agent resets draw nothing");
  if (h->cfg.autoreset == RX_AUTORESET_SAME_STEP)
    return fail(RX_EINVAL, "rx_set_start_draws: same-step autoreset draws inside the step (unsupported)");
  if (n_draws < 0 || !cursor) return fail(RX_EINVAL, "rx_set_start_draws: need n_draws >= 0 and a cursor");
  RX_HIP(hipSetDevice(h->cfg.device));
  const size_t N = (size_t)h->cfg.n_envs;
  if (h->draw_rank.n < N) {
    h->draw_rank.release();
    h->draw_tmp.release();
    if (hipMalloc(&h->draw_rank.p, N * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&h->draw_tmp.p, N * sizeof(int32_t)) != hipSuccess)
      return fail(RX_ENOMEM, "rx_set_start_draws: rank buffers");
    h->draw_rank.n = h->draw_tmp.n = N;
  }
  if (!h->draw_base.p) {
    if (hipMalloc(&h->draw_base.p, sizeof(int64_t)) != hipSuccess) return fail(RX_ENOMEM, "rx_set_start_draws");
    h->draw_base.n = 1;
  }
  h->draws = draws, h->n_draws = n_draws, h->draw_cursor = cursor;
  return RX_OK;
}

int rx_reset(rx_env* h, const uint8_t* mask, const rx_io* io, void* stream) {
  return launch(h, io, RX_MODE_RESET, mask, stream);
}

int rx_step(rx_env* h, const rx_io* io, void* stream) { return launch(h, io, RX_MODE_STEP, nullptr, stream); }

int rx_step_phases(rx_env* h, const rx_io* io, int32_t phases, void* stream) {
  return launch(h, io, RX_MODE_STEP, nullptr, stream, phases);
}

// ABI v21: n_steps steps from one call, each the launches of rx_step on its io rows.
static rx_io io_at(const rx_io* io, const rx_io_strides& st, int64_t s) {
  rx_io o = *io;
  o.actions = io->actions + s * st.actions;
  o.obs = io->obs + s * st.obs;
  if (io->reward) o.reward = io->reward + s * st.reward;
  if (io->reward64) o.reward64 = io->reward64 + s * st.reward64;
  if (io->terminated) o.terminated = io->terminated + s * st.terminated;
  if (io->truncated) o.truncated = io->truncated + s * st.truncated;
  if (io->done_f32) o.done_f32 = io->done_f32 + s * st.done_f32;
  if (io->info) o.info = io->info + s * st.info;
  if (io->ep_done) o.ep_done = io->ep_done + s * st.ep_done;
  return o;
}

// The schedule of K steps as launch records (include/rx.h; DESIGN.md §3 "The carried step",
// "The paired launch", "The crossing step", "The deep launch").  Block b's KIN part of step
// k + 1 needs only block b's REWARD results of step k, so REWARD workgroup b of a k_step2_pair
// launch runs it and k_kin1 leaves the step; a launch's REWARD workgroups advance up to
// `depth` steps D_k = (REWARD k, KIN k + 1).  KIN k + 1 overwrites what the ray waves of step
// k read, so every KIN part also stores its pose to a snapshot and the ray waves read that.
// They read nothing else that a later step writes and nothing of a later step reads what they
// write, so once KIN k's launch has completed they can be cast in ANY later launch.
//
// A step goes through two queues.  `to_rank`: KIN done in an earlier launch, ray tasks not
// ranked yet; `to_cast`: ranked (or passed over by the task_sort cadence) in an earlier
// launch, rays not cast.  Every launch casts all of to_cast, ranks all of to_rank in RANK
// workgroups and refills to_rank with the steps its KIN parts (and the k_kin1 behind it)
// stepped -- so a step's KIN, ranking and rays are three launches in a row, and neither
// queue ever holds more than `depth` steps:
//   k_kin1(0) [D0 D1 | rank 0] [D2 D3 | rank 1 2 | rays 0] [D4 D5 | rank 3 4 | rays 1 2] ...
// A handle that ranks nothing (task_sort 0) and the lag-1 schedule (rank_in_kin: the KIN
// parts rank, as before the deep launch) skip to_rank, and so does a step passed over by the
// cadence while to_rank is empty.  A step passed over by the cadence
// reads the row of the last ranked step before it, or the handle's task buffer when the call
// has ranked none; the call writes ring rows only and leaves the handle's buffer marked stale
// once it has ranked anything (a valid, older order; the next dynamics launch sorts).
//
// A re-sort step, and the call's last step, has no KIN behind its REWARD and ends its
// launch's chain; the re-sort step's REWARD writes the keys, the sort follows the launch and
// a k_kin1 of the next step follows the sort.  With `cross` every step still queued at the
// sort is cast (and ranked) after it from its ring slots, which the sort leaves alone, and
// from the snapshots of perm and progress that the key-writing REWARD stored; without it the
// key-writing REWARD waits for a launch that leaves the queues empty.  At the end of the call
// launches without sub-steps drain the queues.  Rings: see include/rx.h.
int32_t rx_steps_plan(rx_plan_args* in, rx_plan_launch* out, int32_t cap) {
  static_assert(RX_PLAN_CROSS_RING == RX_CROSS_RING && RX_STEPS_DEPTH <= RX_PLAN_MAX_DEPTH, "include/rx.h");
  if (in && in->n_steps >= 1 && in->rank_in_kin < 0)  // the library's own choice for a call of this length
    in->rank_in_kin = RX_STEPS_RANK_IN_KIN || in->n_steps < RX_STEPS_DEEP_MIN_K;
  if (in && in->n_steps >= 1 && in->depth == 0)
    in->depth = in->rank_in_kin ? 2 : in->n_steps < RX_STEPS_FULL_MIN_K ? std::min(4, RX_STEPS_DEPTH) : RX_STEPS_DEPTH;
  if (!in || in->n_steps < 1 || in->depth < 2 || in->depth > RX_PLAN_MAX_DEPTH || in->sort_interval < 0 ||
      in->task_sort < 0 || in->dyn_calls < 0 || in->task_calls < 0 || cap < 0 || (cap > 0 && !out))
    return -1;
  const int32_t K = in->n_steps, D = in->depth, P = 3 * D, T = 2 * D + 1, C = RX_PLAN_CROSS_RING;
  const bool lag1 = in->rank_in_kin != 0, ranking = in->task_sort > 0;
  struct qstep {
    int32_t k, pose, row, snap;  // row: what its rays read; snap: -1 while its window is the live one
    bool ranked;                 // ... and it is ranked into `row` itself
  };
  std::vector<qstep> to_rank, to_cast, stepped;
  bool stale = in->tasks_stale != 0;
  int64_t tcalls = in->task_calls;
  int32_t cur_row = -1, tb = 0, cb = 0, ranked = 0, n_out = 0, k = 0;
  auto resort_step = [&](int32_t s) {
    return in->sort_interval > 0 && ((int64_t)in->dyn_calls + s) % in->sort_interval == 0;
  };
  // step s's KIN part is being scheduled now (in step order: the cadence is K x rx_step's)
  auto kin = [&](int32_t s) {
    bool r = false;
    if (ranking) {
      r = stale || tcalls % in->task_sort == 0;
      if (r) stale = false, cur_row = tb, tb = (tb + 1) % T, ++ranked;
      ++tcalls;
    }
    return qstep{s, s % P, cur_row, -1, r};
  };
  auto blank = [] {
    rx_plan_launch L{};
    L.first_step = -1, L.keys_snap = -1, L.kin1_after = -1, L.kin1_pose = -1, L.kin1_row = -1;
    for (int i = 0; i < RX_PLAN_MAX_DEPTH; ++i) {
      L.kin_pose[i] = L.kin_row[i] = L.rank_step[i] = L.rank_pose[i] = L.rank_row[i] = -1;
      L.ray_step[i] = L.ray_pose[i] = L.ray_row[i] = L.ray_snap[i] = L.ray_shadow[i] = -1;
    }
    return L;
  };
  auto emit = [&](const rx_plan_launch& L) {
    if (n_out < cap) out[n_out] = L;
    ++n_out;
  };
  // A stepped step joins to_rank, or to_cast at once when nothing ranks it and no step before
  // it is still to be ranked (the row it reads was then written by an earlier launch)
  bool ranks_empty = true;  // the launch being planned ranks nothing and passes nothing on
  auto enqueue = [&](const qstep& q) {
    const bool direct = lag1 || !ranking || (!q.ranked && ranks_empty && to_rank.empty());
    (direct ? to_cast : to_rank).push_back(q);
  };
  auto kin1_behind = [&](rx_plan_launch& L, int32_t s) {
    const qstep q = kin(s);
    L.kin1_after = s, L.kin1_pose = q.pose, L.kin1_row = lag1 && q.ranked ? q.row : -1;
    enqueue(q);
  };
  {
    rx_plan_launch L = blank();
    kin1_behind(L, 0);
    emit(L);
  }
  while (k < K || !to_rank.empty() || !to_cast.empty()) {
    if ((int32_t)to_cast.size() > D || (int32_t)to_rank.size() > D) return -2;  // (never: see above)
    rx_plan_launch L = blank();
    L.n_rays = (int32_t)to_cast.size();
    for (int32_t r = 0; r < L.n_rays; ++r) {
      const qstep& q = to_cast[r];
      L.ray_step[r] = q.k, L.ray_pose[r] = q.pose, L.ray_row[r] = q.row, L.ray_snap[r] = q.snap;
      L.ray_shadow[r] = r + 1 < L.n_rays ? r : -1;  // the newest writes the caller's rows
    }
    to_cast.clear();
    for (const qstep& q : to_rank) {
      if (q.ranked) {
        L.rank_step[L.n_rank] = q.k, L.rank_pose[L.n_rank] = q.pose, L.rank_row[L.n_rank] = q.row;
        ++L.n_rank;
      }
      to_cast.push_back(q);
    }
    ranks_empty = to_rank.empty();
    to_rank.clear();
    stepped.clear();
    int32_t n = 0;
    while (n < D && k < K) {
      const bool keyed = resort_step(k), last = k + 1 == K;
      if (keyed) {
        // may steps stay queued across this sort?  lag 1: the crossing step is the second
        // sub-step, a step follows it in the call, and its task row is a ring row
        bool crosses = in->cross != 0;
        if (lag1) crosses = crosses && n == 1 && !last && (!ranking || stepped.back().row >= 0);
        if (!crosses && !(n == 0 && ranks_empty)) break;  // else: the launch that empties the queues
      } else if (lag1 && last && n > 0) {
        break;  // lag 1: the call's last step keeps its own launch (REWARD beside its own rays)
      }
      if (n == 0) L.first_step = k;
      const bool kin_behind = !keyed && !last;
      L.kin[n] = kin_behind;
      if (kin_behind) {
        const qstep q = kin(k + 1);
        L.kin_pose[n] = q.pose, L.kin_row[n] = lag1 && q.ranked ? q.row : -1;
        stepped.push_back(q);
      }
      L.keys = keyed;
      ++k, ++n;
      if (!kin_behind) break;
    }
    L.n_sub = n;
    for (const qstep& q : stepped) enqueue(q);
    if (L.keys) {
      L.sort_after = 1;
      if (!to_rank.empty() || !to_cast.empty()) {
        L.keys_snap = cb;
        for (qstep& q : to_rank)
          if (q.snap < 0) q.snap = cb;
        for (qstep& q : to_cast)
          if (q.snap < 0) q.snap = cb;
        cb = (cb + 1) % C;
      }
      stale = true;  // the re-sort moves envs between blocks
    }
    if (n > 0 && !L.kin[n - 1] && k < K) kin1_behind(L, k);
    if (L.n_sub + L.n_rank + L.n_rays == 0) return -3;  // (never: a launch always makes progress)
    emit(L);
  }
  in->ranked = ranked;
  in->tasks_stale_out = stale || ranked > 0;
  return n_out;
}

// rx_steps' carrying schedule (steps_pair) applies to the split step of single-agent envs at
// one lane per env -- what k_step2_pair is built for -- while nothing records (rx_profile's
// stamps and the counters are per launch of rx_step's kernels), with no re-sort left pending
// by rx_step_phases (its keys belong to a step whose rays are not cast yet), and needs
// rx_assign's snapshot rings and shadow obs rows.  Otherwise rx_steps is K x rx_step.
static bool steps_carried(const rx_env* h, const rx_io* io) {
  if (!RX_STEPS_CARRY || !split_step(h, RX_MODE_STEP) || h->cfg.n_agents != 1 || h->sched.reward_lpe != 1) return false;
  if (h->prof || io->counters || h->sort_pending) return false;
  const bool ranks = h->cfg.ray_order == 2 && !h->sched.lane_tracks;
  for (int b = 0; b < RX_PAIR_RING; ++b)
    if (!h->snap_pose[b].p) return false;
  for (int b = 0; b < RX_TASK_RING; ++b)
    if (ranks && !h->snap_tasks[b].p) return false;
  for (int b = 0; b < RX_SHADOW_ROWS; ++b)
    if (!h->obs_shadow[b].p) return false;
  return true;
}

// K steps with the actions of all of them in device memory: rx_steps_plan's records turned
// into pointers.  Calls of at least RX_STEPS_DEEP_MIN_K steps take the deep schedule (at depth
// 4 below RX_STEPS_FULL_MIN_K steps), shorter ones (and every call of an RX_STEPS_RANK_IN_KIN
// build) the lag-1 schedule at depth 2, which costs two launches fewer per call.  The working state stays single-buffered and is current
// after every launch; a captured call replays with the same buffers (the rings count from
// the start of the call); the bookkeeping (dyn_calls, task_calls, the re-sort) advances as
// K x rx_step.
static int steps_pair(rx_env* h, const rx_io* io, const rx_io_strides& st, int32_t K, hipStream_t s) {
  const size_t N = (size_t)h->cfg.n_envs;
  rx_kargs a{};
  make_kargs(h, io, RX_MODE_STEP, nullptr, a);
  const bool ranks = a.tasks_out != nullptr;  // else this schedule sorts no ray tasks
  const int32_t* const tasks_main = h->tasks.p;
  const bool cross = RX_STEPS_CROSS && resort_on(h) && h->snap_rows[RX_CROSS_RING - 1].p &&
                     h->snap_hint[RX_CROSS_RING - 1].p;
  const int32_t si = resort_on(h) ? h->cfg.sort_interval : 0;
  rx_plan_args pa{K, 0, si, si ? (int32_t)(h->dyn_calls % (uint64_t)si) : 0,
                  ranks ? h->sched.task_sort : 0, ranks ? (int32_t)(h->task_calls % (uint64_t)h->sched.task_sort) : 0,
                  h->tasks_stale ? 1 : 0, cross ? 1 : 0, -1, 0, 0};  // depth and lag: the planner's choice for K
  std::vector<rx_plan_launch> plan((size_t)3 * K + 8);  // (at most two launches a step and the drains)
  const int32_t n_launch = rx_steps_plan(&pa, plan.data(), (int32_t)plan.size());
  if (n_launch < 0 || (size_t)n_launch > plan.size()) return fail(RX_ESTATE, "rx_steps: no schedule (%d)", n_launch);
  auto pose = [&](int32_t slot) { return h->snap_pose[slot].p; };
  auto row = [&](int32_t slot) { return slot < 0 ? nullptr : h->snap_tasks[slot].p; };
  int rc;
  for (int32_t i = 0; i < n_launch; ++i) {
    const rx_plan_launch& L = plan[i];
    a.sort_keys = nullptr, a.sort_hist = nullptr, a.sort_off = nullptr;
    a.snap_x = a.snap_y = a.snap_angle = nullptr;
    a.tasks_out = nullptr, a.tasks_snap = nullptr;
    a.rows_snap = nullptr, a.hint_snap = nullptr;
    if (L.n_sub + L.n_rank + L.n_rays > 0) {
      rx_pair p{};
      p.n_envs = (int64_t)N;
      p.n_sub = L.n_sub, p.n_rank = L.n_rank, p.n_rays = L.n_rays;
      a.io = p.io[0] = io_at(io, st, L.n_sub ? L.first_step : K - 1);
      for (int32_t j = 0; j < L.n_sub; ++j) {
        p.kin[j] = L.kin[j];
        if (!L.kin[j]) continue;
        p.io[j + 1] = io_at(io, st, L.first_step + j + 1);
        p.snap[j] = pose(L.kin_pose[j]);
        p.tasks_out[j] = row(L.kin_row[j]);
      }
      for (int32_t t = 0; t < L.n_rank; ++t) p.rank_pose[t] = pose(L.rank_pose[t]), p.rank_row[t] = row(L.rank_row[t]);
      for (int32_t r = 0; r < L.n_rays; ++r) {
        p.ray_pose[r] = pose(L.ray_pose[r]);
        p.ray_tasks[r] = L.ray_row[r] < 0 ? tasks_main : row(L.ray_row[r]);
        p.ray_rows[r] = L.ray_snap[r] < 0 ? a.perm : h->snap_rows[L.ray_snap[r]].p;
        p.ray_hint[r] = L.ray_snap[r] < 0 ? a.st.progress : h->snap_hint[L.ray_snap[r]].p;
        p.ray_obs[r] = io_at(io, st, L.ray_step[r]).obs;
      }
      // ray steps that would write the same obs rows (stride 0): all but the newest write shadow
      // rows of their own, so the caller's rows end with the newest step's
      for (int32_t r = 0; r + 1 < L.n_rays; ++r)
        if (p.ray_obs[r] == p.ray_obs[L.n_rays - 1]) p.ray_obs[r] = h->obs_shadow[L.ray_shadow[r]].p;
      if (L.keys) {
        if ((rc = arm_sort_keys(h, a, true, s)) != 0) return rc;
        if (L.keys_snap >= 0) a.rows_snap = h->snap_rows[L.keys_snap].p, a.hint_snap = h->snap_hint[L.keys_snap].p;
      }
      if (L.n_sub == 1 && !L.kin[0] && L.n_rank == 0 && L.n_rays == 1 && L.ray_step[0] == L.first_step &&
          L.ray_snap[0] < 0) {  // a KIN-less REWARD beside its own rays: the plain k_step2
        rx_kargs a2 = a;
        a2.ray_x = p.ray_pose[0], a2.ray_y = a2.ray_x + N, a2.ray_angle = a2.ray_x + 2 * N;
        a2.tasks = p.ray_tasks[0];
        if ((rc = rx_launch_split(&a2, 1, RX_SPLIT_REWARD_RAYS, s)) != 0)
          return fail(RX_EHIP, "k_step2 launch failed: %s", hipGetErrorString((hipError_t)rc));
      } else if ((rc = rx_launch_step2_pair(&a, &p, s)) != 0) {
        return fail(RX_EHIP, "k_step2_pair launch failed: %s", hipGetErrorString((hipError_t)rc));
      }
    }
    if (L.sort_after && (rc = sort_envs_now(h, s)) != 0) return rc;
    if (L.kin1_after >= 0) {
      a.io = io_at(io, st, L.kin1_after);
      a.sort_keys = nullptr, a.sort_hist = nullptr, a.sort_off = nullptr;
      a.rows_snap = nullptr, a.hint_snap = nullptr;
      a.snap_x = pose(L.kin1_pose), a.snap_y = a.snap_x + N, a.snap_angle = a.snap_x + 2 * N;
      a.tasks_out = row(L.kin1_row), a.tasks_snap = nullptr;
      if ((rc = rx_launch_split(&a, 1, RX_SPLIT_KIN, s)) != 0)
        return fail(RX_EHIP, "k_kin1 launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
  }
  if (resort_on(h)) h->dyn_calls += (uint64_t)K;
  if (ranks) {
    h->task_calls += (uint64_t)K;
    h->tasks_stale = pa.tasks_stale_out != 0;
  }
  return RX_OK;
}

int rx_steps(rx_env* h, const rx_io* io, int32_t n_steps, const rx_io_strides* strides, void* stream) {
  if (!h) return fail(RX_EINVAL, "null handle");
  if (!io) return fail(RX_EINVAL, "io is null");
  if (n_steps < 0) return fail(RX_EINVAL, "n_steps must be >= 0 (got %d)", n_steps);
  if (!io->obs || !io->actions) return fail(RX_EINVAL, "io->obs and io->actions are required");
  if (h->n_tracks <= 0 || !h->assigned || !h->bound)
    return fail(RX_ESTATE, "rx_steps needs rx_upload_tracks, rx_assign and rx_bind_state");
  const rx_io_strides st = strides ? *strides : rx_io_strides{};
  int rc;
  if (steps_carried(h, io) && n_steps > 0) return steps_pair(h, io, st, n_steps, (hipStream_t)stream);
  for (int32_t k = 0; k < n_steps; ++k) {
    const rx_io o = io_at(io, st, k);
    if ((rc = launch(h, &o, RX_MODE_STEP, nullptr, stream)) != 0) return rc;
  }
  return RX_OK;
}

// ---- track tables already on the device (ABI v25, additive): the handle's side of
// rx_build_cull_tables and rx_patch_tracks, whose checks and launches are in rx_api_tracks.cpp
int rx_upload_tracks_device(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* nrm,
                            const double* seg, const double* meta, void* stream) {
  if (!h) return fail(RX_EINVAL, "rx_upload_tracks_device: null handle");
  if (n_tracks <= 0 || !wp_off || !wp || !nrm || !seg || !meta)
    return fail(RX_EINVAL, "rx_upload_tracks_device: bad arguments");
  const int G = h->cfg.cull_chunk, SG = h->cfg.cull_super;
  std::vector<int32_t> off;
  int64_t tot[4];
  {  // the offsets' checks (rx_upload_tracks' W limits); the output pointers are the handle's, set below
    const int rc = cull_check("rx_upload_tracks_device", n_tracks, wp_off, nullptr, nullptr, nullptr, G, SG, nullptr,
                              true, &off, tot);
    if (rc != RX_OK) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  RX_HIP(hipSetDevice(h->cfg.device));
  // launches of the old table may be in flight on any stream, and buffers may be re-allocated
  RX_HIP(hipDeviceSynchronize());
  std::vector<double> meta_h(8 * (size_t)n_tracks);  // the one transfer to the host
  RX_HIP(hipMemcpyAsync(meta_h.data(), meta, meta_h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  RX_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n_tracks; ++k) {
    if (!(meta_h[8 * (size_t)k + 3] >= 0)) return fail(RX_EINVAL, "rx_upload_tracks_device: track %d width invalid", k);
    if (!(meta_h[8 * (size_t)k + 4] > 0))
      return fail(RX_EINVAL, "rx_upload_tracks_device: track %d max_track_distance must be > 0 (got %g; NaN marks a "
                             "track rx_build_tracks found invalid)", k, meta_h[8 * (size_t)k + 4]);
  }
  // nothing of the handle has changed so far; from here on the old table is gone
  const size_t n1 = (size_t)n_tracks + 1, Wt = (size_t)wp_off[n_tracks];
  int rc;
  if ((rc = reserve(h->wp_off, n1)) || (rc = reserve(h->wp, 2 * Wt)) || (rc = reserve(h->nrm, 2 * Wt)) ||
      (rc = reserve(h->seg, 8 * Wt)) || (rc = reserve(h->meta, 8 * (size_t)n_tracks)) ||
      (rc = reserve(h->seg_f, 8 * Wt)) || (rc = reserve(h->slot_hdr, (size_t)n_tracks)))
    return rc;
  if (G > 0) {
    if ((rc = reserve(h->chunk_off, n1)) || (rc = reserve(h->wchunk_off, n1)) || (rc = reserve(h->wsuper_off, n1)) ||
        (rc = reserve(h->chunk_box, 4 * (size_t)tot[0])) || (rc = reserve(h->chunk_box_f, 20 * (size_t)tot[0])) ||
        (rc = reserve(h->wchunk_box, 4 * (size_t)tot[2])) || (rc = reserve(h->wsuper_box, 4 * (size_t)tot[3])) ||
        (rc = reserve(h->slot_geo, 4 * (size_t)n_tracks)))
      return rc;
    if (SG > 0 && ((rc = reserve(h->super_off, n1)) || (rc = reserve(h->super_box, 4 * (size_t)tot[1])) ||
                   (rc = reserve(h->super_box_f, 20 * (size_t)tot[1]))))
      return rc;
  }
  h->n_tracks = 0;  // until the new table stands
  h->assigned = false;
  RX_HIP(hipMemcpyAsync(h->wp_off.p, wp_off, n1 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  RX_HIP(hipMemcpyAsync(h->wp.p, wp, 2 * Wt * sizeof(double), hipMemcpyDeviceToDevice, s));
  RX_HIP(hipMemcpyAsync(h->nrm.p, nrm, 2 * Wt * sizeof(double), hipMemcpyDeviceToDevice, s));
  RX_HIP(hipMemcpyAsync(h->seg.p, seg, 8 * Wt * sizeof(double), hipMemcpyDeviceToDevice, s));
  RX_HIP(hipMemcpyAsync(h->meta.p, meta, 8 * (size_t)n_tracks * sizeof(double), hipMemcpyDeviceToDevice, s));
  const rx_cull_tables t = {h->chunk_off.p, h->super_off.p,  h->wchunk_off.p, h->wsuper_off.p,  h->chunk_box.p,
                            h->super_box.p, h->wchunk_box.p, h->wsuper_box.p, h->slot_geo.p,    h->chunk_box_f.p,
                            h->super_box_f.p, h->seg_f.p,    h->slot_hdr.p};
  if ((rc = cull_launch("rx_upload_tracks_device", n_tracks, off, tot, h->wp.p, h->seg.p, h->meta.p, G, SG, &t, s)))
    return rc;
  RX_HIP(hipStreamSynchronize(s));
  if (G > 0) {
    h->n_chunk_boxes = (int32_t)tot[0];
    h->n_super_boxes = (int32_t)tot[1];
  }
  h->wp_off_h.assign(wp_off, wp_off + n1);
  h->n_tracks = n_tracks;
  return RX_OK;
}

int rx_replace_tracks_device(rx_env* h, const rx_track_patch* p, void* stream) {
  const char* fn = "rx_replace_tracks_device";
  if (!h) return fail(RX_EINVAL, "%s: null handle", fn);
  if (h->n_tracks <= 0) return fail(RX_ESTATE, "%s before a track table was uploaded", fn);
  const int G = h->cfg.cull_chunk, SG = h->cfg.cull_super;
  const rx_cull_tables t = {h->chunk_off.p, h->super_off.p,  h->wchunk_off.p, h->wsuper_off.p,  h->chunk_box.p,
                            h->super_box.p, h->wchunk_box.p, h->wsuper_box.p, h->slot_geo.p,    h->chunk_box_f.p,
                            h->super_box_f.p, h->seg_f.p,    h->slot_hdr.p};
  std::vector<rx_patch_slot> ps;
  int64_t tot[4];
  int rc = patch_check(fn, h->n_tracks, h->wp_off_h.data(), h->wp.p, h->nrm.p, h->seg.p, h->meta.p, G, SG, &t, p, &ps,
                       tot);
  if (rc != RX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  RX_HIP(hipSetDevice(h->cfg.device));
  RX_HIP(hipDeviceSynchronize());  // launches reading the old rows may be in flight on any stream
  std::vector<double> meta_h(8 * (size_t)p->n_upd);  // the one transfer to the host
  RX_HIP(hipMemcpyAsync(meta_h.data(), p->meta, meta_h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  RX_HIP(hipStreamSynchronize(s));
  if ((rc = patch_check_meta(fn, p, meta_h.data()))) return rc;
  // nothing of the handle has changed so far
  if ((rc = patch_launch(fn, ps, tot, h->wp.p, h->nrm.p, h->seg.p, h->meta.p, G, SG, &t, p, s))) return rc;
  RX_HIP(hipStreamSynchronize(s));
  return RX_OK;
}
