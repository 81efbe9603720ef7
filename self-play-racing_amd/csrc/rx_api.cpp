// rx_api.cpp -- C ABI (include/rx.h): handle lifetime, argument validation,
// track-table upload, env->wavefront grouping, launches.
//
// Everything that allocates or copies synchronously (rx_upload_tracks,
// rx_assign) happens outside the step path; rx_reset / rx_step / rx_gae only
// enqueue kernels on the caller's stream, so they can be graph-captured.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <type_traits>
#include <string>
#include <vector>

#include "rx.h"
#include "rx_cull.h"
#include "rx_internal.h"
#include "rx_spline.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define RX_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return fail(RX_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// a device allocation that frees itself (on the current device: rx_destroy sets the handle's)
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// room for n elements: the buffer is kept when it is large enough (its address then stays)
template <class T>
int reserve(DevBuf<T>& b, size_t n) {
  if (n > b.n) {
    b.release();
    if (hipMalloc(&b.p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      b.p = nullptr;
      return fail(RX_ENOMEM, "hipMalloc(%zu bytes) failed", n * sizeof(T));
    }
    b.n = n;
  }
  return RX_OK;
}

template <class T>
int upload(DevBuf<T>& b, const T* host, size_t n) {
  const int rc = reserve(b, n);
  if (rc != RX_OK) return rc;
  if (n) RX_HIP(hipMemcpy(b.p, host, n * sizeof(T), hipMemcpyHostToDevice));
  return RX_OK;
}

}  // namespace

#define RX_WORK_ARRAYS 14  // device arrays of one working rx_state (rx_bind_state)

struct rx_env {
  rx_config cfg{};
  int D = 0;
  // track table
  int32_t n_tracks = 0;
  std::vector<int32_t> wp_off_h;
  DevBuf<int32_t> wp_off;
  DevBuf<double> wp, nrm, seg, meta;
  // raycast culling tables (derived from the track table)
  DevBuf<int32_t> chunk_off;
  DevBuf<double> chunk_box, slot_geo, wchunk_box;
  DevBuf<int32_t> wchunk_off;
  DevBuf<int32_t> super_off;  // two-level culling: super-chunk boxes per slot
  DevBuf<double> super_box;
  DevBuf<int32_t> wsuper_off;  // two-level closest-waypoint culling
  DevBuf<double> wsuper_box;
  DevBuf<float> chunk_box_f, super_box_f;  // outward-rounded float32 copies (raycast box tests) + 4 quadrant blocks
  int32_t n_chunk_boxes = 0, n_super_boxes = 0;
  DevBuf<float> seg_f;  // [2*Wtot][4] float32 (start.x, start.y, v2.x, v2.y): the raycast's segment pre-filter
  DevBuf<rx_slot_hdr> slot_hdr;  // [n] per-slot headers (lane-varying kernels)
  // assignment
  bool assigned = false;
  DevBuf<int32_t> perm[2];  // the env order (perm[0]: env id at each position) and the re-sort's shadow
  DevBuf<rx_wave> dyn_waves, ray_waves;
  std::vector<rx_wave> ray_waves_h;  // host copy of the ray-wave table (rx_ray_waves)
  DevBuf<int32_t> slot_n;   // envs per slot (ray-major decode)
  DevBuf<uint32_t> resets;  // per-env reset count: keys the 2-car start-slot draw (graph-replay safe)
  // rx_set_start_draws: the caller's MT19937 outputs and cursor; ranks of the resetting envs
  const uint32_t* draws = nullptr;
  int64_t n_draws = 0;
  int64_t* draw_cursor = nullptr;
  DevBuf<int32_t> draw_rank, draw_tmp;
  DevBuf<int64_t> draw_base;
  rx_sched sched;  // the schedule the assignment resolved (rx_assign_plan.h): written whole, after the last upload
  DevBuf<int32_t> pos_slot;                // with lane_tracks: [N] slot of the env at each position
  DevBuf<int32_t> env_pos;                 // with lane_tracks: [N] position of each env, the inverse of perm
                                           // (rx_track_episode_step: the episodic draw rewrites pos_slot)
  DevBuf<uint8_t> policy_frag;  // the bf16 rollout's operand fragments of both trunks (k_policy_frag, rx_rollout_steps)
  DevBuf<double> rel_angles;
  std::vector<double> rel_angles_h;
  // spatial sort (scheduling only)
  DevBuf<uint32_t> keys_in;              // [N] bin per perm position (REWARD half)
  DevBuf<uint32_t> keys_off;             // [N] the position's rank within its bin (the count's atomic)
  bool sort_pending = false;             // keys written, the re-sort runs after this step's raycast
  bool sort_hist_done = false;           // the REWARD half of the keys' launch also counted the bins
  DevBuf<uint32_t> sort_hist, sort_cursor;  // [sort_bins]
  DevBuf<int32_t> sort_base;             // [n_tracks] first bin of each slot
  uint64_t dyn_calls = 0;
  // ray-task direction sort (ray_order 2): every RX_TASK_SORT_INTERVAL dynamics
  // launches, and always on the first launch after a block's membership changed
  bool tasks_stale = true;
  uint64_t task_calls = 0;
  // ray_order 2: direction-sorted (agent, ray) task ids, rewritten by k_dyn every step
  DevBuf<int32_t> tasks;
  // split step (k_kin1 + k_step2): cos / sin of the stepped angles
  DevBuf<double> cs_scratch;
  // rx_steps' carrying schedule: rings of snapshots of what the ray waves read -- the stepped
  // pose ([3][N] x, y, angle) and the sorted task ids -- written by a step's KIN part, and a
  // shadow of the obs rows for every ray step of a launch but its newest, which would write
  // the same rows (stride-0 outputs); the task rows are written by the RANK workgroups of the
  // deep launch (rx_internal.h)
  DevBuf<double> snap_pose[RX_PAIR_RING];
  DevBuf<int32_t> snap_tasks[RX_TASK_RING];
  DevBuf<float> obs_shadow[RX_SHADOW_ROWS];
  DevBuf<int32_t> snap_rows[RX_CROSS_RING];  // the crossing step's row ids and visiting-order hint (pre-sort)
  DevBuf<double> snap_hint[RX_CROSS_RING];
  // rx_profile: per recorded launch, [RX_PROF_SLOTS] wave start + [RX_PROF_SLOTS] wave end stamps
  bool prof = false;
  DevBuf<unsigned long long> prof_buf;
  std::vector<int> prof_kinds;
  // state: the caller's arrays (env order, rx_bind_state) and the engine's
  // working copy in wave order (position p = env perm[p]; the kernels read and
  // write it coalesced) plus the shadow the re-sort moves rows into
  bool bound = false;
  rx_state st{};
  rx_state work{}, work_tmp{};
  DevBuf<uint8_t> work_mem[2 * RX_WORK_ARRAYS];  // the arrays of work and work_tmp
};

namespace {
// ---- culling tables (csrc/rx_cull.h) ------------------------------------------
// What the host can check of a culling-table build, and the offsets: off receives
// wp_off and the chunk / super / wchunk / wsuper offset arrays back to back
// (n + 1 entries each), tot the four box totals.  sizes_only: the offsets alone are
// checked (rx_cull_table_sizes; rx_upload_tracks_device, whose arrays are the handle's).
int cull_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* seg, const void* meta,
               int32_t G, int32_t SG, const rx_cull_tables* out, bool sizes_only, std::vector<int32_t>* off,
               int64_t tot[4]) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!wp_off) return fail(RX_EINVAL, "%s: wp_off is null", fn);
  if (!sizes_only) {
    if (!wp) return fail(RX_EINVAL, "%s: wp is null", fn);
    if (!seg) return fail(RX_EINVAL, "%s: seg is null", fn);
    if (!meta) return fail(RX_EINVAL, "%s: meta is null", fn);
    if (!out) return fail(RX_EINVAL, "%s: out is null", fn);
    const struct {
      const void* p;
      const char* name;
      bool need;
    } fields[] = {{out->seg_f, "seg_f", true},
                  {out->slot_hdr, "slot_hdr", true},
                  {out->chunk_off, "chunk_off", G > 0},
                  {out->wchunk_off, "wchunk_off", G > 0},
                  {out->wsuper_off, "wsuper_off", G > 0},
                  {out->chunk_box, "chunk_box", G > 0},
                  {out->wchunk_box, "wchunk_box", G > 0},
                  {out->wsuper_box, "wsuper_box", G > 0},
                  {out->slot_geo, "slot_geo", G > 0},
                  {out->chunk_box_f, "chunk_box_f", G > 0},
                  {out->super_off, "super_off", G > 0 && SG > 0},
                  {out->super_box, "super_box", G > 0 && SG > 0},
                  {out->super_box_f, "super_box_f", G > 0 && SG > 0}};
    for (const auto& f : fields)
      if (f.need && !f.p) return fail(RX_EINVAL, "%s: out->%s is null", fn, f.name);
  }
  if (SG < 0 || SG > RX_CULL_MAX_SUPER)
    return fail(RX_EINVAL, "%s: cull_super must be 0 .. %d (got %d)", fn, RX_CULL_MAX_SUPER, SG);
  if (wp_off[0] != 0) return fail(RX_EINVAL, "%s: wp_off[0] must be 0 (got %d)", fn, wp_off[0]);
  const size_t n1 = (size_t)n + 1;
  if (off) off->assign(5 * n1, 0);
  int64_t run[4] = {0, 0, 0, 0};
  for (int32_t k = 0; k < n; ++k) {
    const int64_t W = (int64_t)wp_off[k + 1] - wp_off[k];
    if (W < 2) return fail(RX_EINVAL, "%s: track %d has W = %lld waypoints (need >= 2)", fn, k, (long long)W);
    if (W > RX_CULL_MAX_W)
      return fail(RX_EINVAL, "%s: track %d has W = %lld waypoints (at most %d)", fn, k, (long long)W, RX_CULL_MAX_W);
    const rx_cull_counts c = rx_cull_slot_counts((int32_t)W, G, SG);
    const int32_t add[4] = {c.leaf, c.super, c.wchunk, c.wsuper};
    for (int a = 0; a < 4; ++a) {
      run[a] += add[a];
      if (run[a] > INT32_MAX)
        return fail(RX_EINVAL, "%s: track %d: the box count overflows the int32 offsets", fn, k);
      if (off) (*off)[(a + 1) * n1 + k + 1] = (int32_t)run[a];
    }
    if (off) (*off)[k + 1] = wp_off[k + 1];
  }
  for (int a = 0; a < 4; ++a) tot[a] = run[a];
  return RX_OK;
}

// Culling tables for every slot (rx_cull.h through the host twin): chunks of G
// consecutive boundary segments per side, their end-point boxes, per slot the
// bounding circle of all boundary points and the longest segment (kernel margins,
// DESIGN.md §3), the float32 copies and the per-slot headers.
int build_chunks(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* seg,
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
}  // namespace

extern "C" {

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
  int rc = rx_plan_assignment(h->cfg, h->n_tracks, h->wp_off_h.data(), track_of_env, &plan, &err);
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

int rx_assign_plan(const rx_config* cfg, int32_t n_tracks, const int32_t* wp_off, const int32_t* track_of_env,
                   rx_assign_plan_io* io) {
  if (!cfg || !wp_off || !track_of_env || !io) return fail(RX_EINVAL, "rx_assign_plan: null argument");
  if (n_tracks <= 0) return fail(RX_EINVAL, "rx_assign_plan: n_tracks must be > 0 (got %d)", n_tracks);
  for (int k = 0; k < n_tracks; ++k)
    if (wp_off[k + 1] - wp_off[k] < 2)
      return fail(RX_EINVAL, "track %d has %d waypoints (need >= 2)", k, wp_off[k + 1] - wp_off[k]);
  rx_assignment plan;
  std::string err;
  const int rc = rx_plan_assignment(*cfg, n_tracks, wp_off, track_of_env, &plan, &err);
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

static void make_kargs(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, rx_kargs& a) {
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

static int launch(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, void* stream, int phases = 3) {
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
static int precision_arg(const char* fn, const char* field, int32_t precision) {
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

// ---- track table builders (ABI v24) ------------------------------------------
// What the host can check from the offsets alone; fills wp_off.
static int tracks_shape(const char* fn, int32_t n, int32_t factor, const int32_t* cp_off, const void* cp,
                        const void* width, int32_t* wp_off, const void* wp, const void* nrm, const void* seg,
                        const void* meta) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!cp_off || !cp || !width || !wp_off || !wp || !nrm || !seg || !meta) return fail(RX_EINVAL, "%s: null buffer", fn);
  if (factor < 1) return fail(RX_EINVAL, "%s: factor must be >= 1 (got %d)", fn, factor);
  if (cp_off[0] != 0) return fail(RX_EINVAL, "%s: cp_off[0] must be 0", fn);
  const int max_w = 64 * RX_WP_CHUNK * RX_WP_SUPER;  // rx_upload_tracks' limit
  for (int32_t k = 0; k < n; ++k) {
    const int64_t P = (int64_t)cp_off[k + 1] - cp_off[k];
    if (P < 3 || P > RX_TRACK_MAX_P)
      return fail(RX_EINVAL, "%s: track %d has P = %lld control points (3 .. %d)", fn, k, (long long)P, RX_TRACK_MAX_P);
    if (P * factor > max_w)
      return fail(RX_EINVAL, "%s: track %d has W = P * factor = %lld waypoints (at most %d)", fn, k,
                  (long long)(P * factor), max_w);
  }
  if ((int64_t)cp_off[n] * factor > INT32_MAX)
    return fail(RX_EINVAL, "%s: W summed over the tracks = %lld overflows wp_off (int32)", fn,
                (long long)cp_off[n] * factor);
  for (int32_t k = 0; k <= n; ++k) wp_off[k] = cp_off[k] * factor;
  return RX_OK;
}

int rx_build_tracks(int32_t n, int32_t factor, const int32_t* cp_off, const double* cp, const double* width,
                    int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, void* stream) {
  const int rc = tracks_shape("rx_build_tracks", n, factor, cp_off, cp, width, wp_off, wp, nrm, seg, meta);
  if (rc != RX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t* off_dev = nullptr;
  const size_t bytes = ((size_t)n + 1) * sizeof(int32_t);
  if (hipMallocAsync((void**)&off_dev, bytes, s) != hipSuccess || !off_dev)
    return fail(RX_ENOMEM, "rx_build_tracks: hipMallocAsync(%zu bytes) failed", bytes);
  hipError_t e = hipMemcpyAsync(off_dev, cp_off, bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess) lrc = rx_launch_build_tracks(n, factor, off_dev, cp, width, wp, nrm, seg, meta, s);
  const hipError_t ef = hipFreeAsync(off_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "rx_build_tracks: offset copy failed: %s", hipGetErrorString(e));
  if (lrc != 0) return fail(RX_EHIP, "rx_build_tracks: launch failed: %s", hipGetErrorString((hipError_t)lrc));
  if (ef != hipSuccess) return fail(RX_EHIP, "rx_build_tracks: hipFreeAsync failed: %s", hipGetErrorString(ef));
  return RX_OK;
}

int rx_build_tracks_host(int32_t n, int32_t factor, const int32_t* cp_off, const double* cp, const double* width,
                         int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, void* /*stream*/) {
  const int rc = tracks_shape("rx_build_tracks_host", n, factor, cp_off, cp, width, wp_off, wp, nrm, seg, meta);
  if (rc != RX_OK) return rc;
  for (int32_t k = 0; k < n; ++k) {  // the data, before anything is written
    const int P = cp_off[k + 1] - cp_off[k];
    int at = 0;
    switch (rx_track_check(P, cp + 2 * (size_t)cp_off[k], width[k], &at)) {
      case RX_TRACK_BAD_COORD:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: cp[%d] has a non-finite coordinate", k, at);
      case RX_TRACK_BAD_CHORD:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: chord %d (cp[%d] to cp[%d]) has zero or non-finite "
                               "length", k, at, at, (at + 1) % P);
      case RX_TRACK_BAD_WIDTH:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: width %g is negative or NaN", k, width[k]);
      default:
        break;
    }
  }
  rx_spline_ws ws;
  for (int32_t k = 0; k < n; ++k) {  // the kernel's steps (rx_track.hip), one lane at a time
    const int P = cp_off[k + 1] - cp_off[k], W = P * factor;
    const double* c = cp + 2 * (size_t)cp_off[k];
    const size_t base = (size_t)wp_off[k];
    for (int i = 0; i < P; ++i) rx_spline_load(i, c, &ws);
    rx_spline_knots(P, W, &ws);
    rx_spline_solve(P, 0, &ws);
    rx_spline_solve(P, 1, &ws);
    for (int i = 0; i < P; ++i) rx_spline_coef(P, i, &ws);
    double b[4] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};
    for (int j = 0; j < W; ++j) {
      double x, y;
      rx_track_point(P, W, &ws, width[k], j, wp + 2 * base, nrm + 2 * base, seg + 8 * base, &x, &y);
      rx_track_bounds(x, y, b);
    }
    double dy, dx;
    rx_track_meta(P, W, &ws, width[k], b, meta + 8 * (size_t)k, &dy, &dx);
    meta[8 * (size_t)k + 2] = atan2(dy, dx);
  }
  return RX_OK;
}

// ---- culling tables (ABI v25, additive) -----------------------------------------
int rx_cull_table_sizes(int32_t n, const int32_t* wp_off, int32_t G, int32_t SG, int64_t* out) {
  if (!out) return fail(RX_EINVAL, "rx_cull_table_sizes: out is null");
  return cull_check("rx_cull_table_sizes", n, wp_off, nullptr, nullptr, nullptr, G, SG, nullptr, true, nullptr, out);
}

int rx_build_cull_tables_host(int32_t n, const int32_t* wp_off, const double* wp, const double* seg,
                              const double* meta, int32_t G, int32_t SG, const rx_cull_tables* t, void* /*stream*/) {
  std::vector<int32_t> off;
  int64_t tot[4];
  const int rc = cull_check("rx_build_cull_tables_host", n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot);
  if (rc != RX_OK) return rc;
  const size_t n1 = (size_t)n + 1;
  for (int32_t k = 0; k < n; ++k) {  // the kernel's steps (rx_cull.hip) with one lane
    const int32_t wp0 = wp_off[k], W = wp_off[k + 1] - wp0;
    const double* s = seg + 8 * (size_t)wp0;
    rx_cull_slot o = {0, 0, 0, 0, tot[0], tot[1], t->chunk_box, t->super_box, t->wchunk_box, t->wsuper_box,
                      t->chunk_box_f, t->super_box_f};
    double b[4], longest, geo[4] = {0.0, 0.0, 0.0, 0.0};
    rx_cull_extent(s, W, 0, 1, t->seg_f + 8 * (size_t)wp0, b, &longest);
    if (G > 0) {
      rx_cull_geo(b, rx_cull_reach(s, W, 0, 1, 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])), longest, geo);
      o.chunk0 = off[n1 + k];
      o.super0 = SG > 0 ? off[2 * n1 + k] : 0;
      o.wchunk0 = off[3 * n1 + k];
      o.wsuper0 = off[4 * n1 + k];
      rx_cull_boxes(s, wp + 2 * (size_t)wp0, W, G, SG, 0, 1, &o);
      for (int c = 0; c < 4; ++c) t->slot_geo[4 * (size_t)k + c] = geo[c];
    }
    rx_cull_header((rx_slot_hdr*)t->slot_hdr + k, wp0, W, &o, geo, meta + 8 * (size_t)k);
  }
  if (G > 0) {
    std::copy(off.begin() + n1, off.begin() + 2 * n1, t->chunk_off);
    if (SG > 0) std::copy(off.begin() + 2 * n1, off.begin() + 3 * n1, t->super_off);
    std::copy(off.begin() + 3 * n1, off.begin() + 4 * n1, t->wchunk_off);
    std::copy(off.begin() + 4 * n1, off.begin() + 5 * n1, t->wsuper_off);
  }
  return RX_OK;
}

// The launch behind rx_build_cull_tables and rx_upload_tracks_device: `off` (cull_check's
// five offset arrays) goes up through a stream-ordered allocation, as rx_build_tracks'
// offsets do (a pageable source: the copy has left `off` when hipMemcpyAsync returns).
static int cull_launch(const char* fn, int32_t n, const std::vector<int32_t>& off, const int64_t tot[4],
                       const double* wp, const double* seg, const double* meta, int32_t G, int32_t SG,
                       const rx_cull_tables* t, hipStream_t s) {
  int32_t* off_dev = nullptr;
  const size_t bytes = off.size() * sizeof(int32_t);
  if (hipMallocAsync((void**)&off_dev, bytes, s) != hipSuccess || !off_dev)
    return fail(RX_ENOMEM, "%s: hipMallocAsync(%zu bytes) failed", fn, bytes);
  hipError_t e = hipMemcpyAsync(off_dev, off.data(), bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess) lrc = rx_launch_cull_tables(n, G, SG, off_dev, wp, seg, meta, t, tot[0], tot[1], s);
  const hipError_t ef = hipFreeAsync(off_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "%s: offset copy failed: %s", fn, hipGetErrorString(e));
  if (lrc != 0) return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)lrc));
  if (ef != hipSuccess) return fail(RX_EHIP, "%s: hipFreeAsync failed: %s", fn, hipGetErrorString(ef));
  return RX_OK;
}

int rx_build_cull_tables(int32_t n, const int32_t* wp_off, const double* wp, const double* seg, const double* meta,
                         int32_t G, int32_t SG, const rx_cull_tables* t, void* stream) {
  std::vector<int32_t> off;
  int64_t tot[4];
  const int rc = cull_check("rx_build_cull_tables", n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot);
  if (rc != RX_OK) return rc;
  return cull_launch("rx_build_cull_tables", n, off, tot, wp, seg, meta, G, SG, t, (hipStream_t)stream);
}

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

// ---- slots replaced in place (ABI v25, additive) ---------------------------------
// What the host can check of a patch, before any HIP call or write; ps receives the
// listed slots' rows for the kernel and the host twin, tot the table's box totals.
// t == nullptr: the four table arrays only (G and SG are then not looked at).
static int patch_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* nrm,
                       const void* seg, const void* meta, int32_t G, int32_t SG, const rx_cull_tables* t,
                       const rx_track_patch* p, std::vector<rx_patch_slot>* ps, int64_t tot[4]) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!wp_off) return fail(RX_EINVAL, "%s: wp_off is null", fn);
  if (!wp) return fail(RX_EINVAL, "%s: wp is null", fn);
  if (!nrm) return fail(RX_EINVAL, "%s: nrm is null", fn);
  if (!seg) return fail(RX_EINVAL, "%s: seg is null", fn);
  if (!meta) return fail(RX_EINVAL, "%s: meta is null", fn);
  if (!p) return fail(RX_EINVAL, "%s: the patch is null", fn);
  const struct {
    const void* q;
    const char* name;
  } fields[] = {{p->slots, "slots"}, {p->src_off, "src_off"}, {p->wp, "wp"},
                {p->nrm, "nrm"},     {p->seg, "seg"},         {p->meta, "meta"}};
  for (const auto& f : fields)
    if (!f.q) return fail(RX_EINVAL, "%s: patch->%s is null", fn, f.name);
  std::vector<int32_t> off;
  const int rc = t ? cull_check(fn, n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot)
                   : cull_check(fn, n, wp_off, nullptr, nullptr, nullptr, 0, 0, nullptr, true, &off, tot);
  if (rc != RX_OK) return rc;
  if (p->n_upd < 1 || p->n_upd > n)
    return fail(RX_EINVAL, "%s: patch->n_upd must be 1 .. n_tracks = %d (got %d)", fn, n, p->n_upd);
  if (p->src_off[0] != 0) return fail(RX_EINVAL, "%s: patch->src_off[0] must be 0 (got %d)", fn, p->src_off[0]);
  const size_t n1 = (size_t)n + 1;
  ps->assign((size_t)p->n_upd, rx_patch_slot{});
  for (int32_t j = 0; j < p->n_upd; ++j) {
    const int32_t k = p->slots[j];
    if (k < 0 || k >= n)
      return fail(RX_EINVAL, "%s: patch->slots[%d] = slot %d is outside [0, %d)", fn, j, k, n);
    if (j > 0 && k <= p->slots[j - 1])
      return fail(RX_EINVAL, "%s: patch->slots[%d] = slot %d follows slot %d: the slots must be ascending and "
                             "distinct", fn, j, k, p->slots[j - 1]);
    const int64_t Ws = (int64_t)p->src_off[j + 1] - p->src_off[j], W = (int64_t)wp_off[k + 1] - wp_off[k];
    if (Ws != W)
      return fail(RX_EINVAL, "%s: slot %d: patch->src_off gives source track %d %lld waypoints, the slot has %lld "
                             "(a replaced slot keeps its waypoint count)", fn, k, j, (long long)Ws, (long long)W);
    (*ps)[j] = rx_patch_slot{k, p->src_off[j], wp_off[k], (int32_t)W, off[n1 + k], off[2 * n1 + k],
                             off[3 * n1 + k], off[4 * n1 + k]};
  }
  return RX_OK;
}

// rx_upload_tracks' per-track checks on the source meta rows (host memory), the slot named
static int patch_check_meta(const char* fn, const rx_track_patch* p, const double* meta_h) {
  for (int32_t j = 0; j < p->n_upd; ++j) {
    const double* m = meta_h + 8 * (size_t)j;
    if (!(m[3] >= 0))
      return fail(RX_EINVAL, "%s: slot %d (source track %d): width %g is negative or NaN", fn, p->slots[j], j, m[3]);
    if (!(m[4] > 0))
      return fail(RX_EINVAL, "%s: slot %d (source track %d): max_track_distance must be > 0 (got %g; NaN marks a "
                             "track rx_build_tracks found invalid)", fn, p->slots[j], j, m[4]);
  }
  return RX_OK;
}

// The launch behind rx_patch_tracks and rx_replace_tracks_device: the listed slots' rows
// go up through a stream-ordered allocation, as cull_launch's offsets do.
static int patch_launch(const char* fn, const std::vector<rx_patch_slot>& ps, const int64_t tot[4], double* wp,
                        double* nrm, double* seg, double* meta, int32_t G, int32_t SG, const rx_cull_tables* t,
                        const rx_track_patch* p, hipStream_t s) {
  rx_patch_slot* ps_dev = nullptr;
  const size_t bytes = ps.size() * sizeof(rx_patch_slot);
  if (hipMallocAsync((void**)&ps_dev, bytes, s) != hipSuccess || !ps_dev)
    return fail(RX_ENOMEM, "%s: hipMallocAsync(%zu bytes) failed", fn, bytes);
  hipError_t e = hipMemcpyAsync(ps_dev, ps.data(), bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess)
    lrc = rx_launch_patch_slots((int)ps.size(), t ? G : 0, t ? SG : 0, ps_dev, p, wp, nrm, seg, meta, t, tot[0],
                                tot[1], s);
  const hipError_t ef = hipFreeAsync(ps_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "%s: slot list copy failed: %s", fn, hipGetErrorString(e));
  if (lrc != 0) return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)lrc));
  if (ef != hipSuccess) return fail(RX_EHIP, "%s: hipFreeAsync failed: %s", fn, hipGetErrorString(ef));
  return RX_OK;
}

int rx_patch_tracks(int32_t n, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, int32_t G,
                    int32_t SG, const rx_cull_tables* t, const rx_track_patch* p, void* stream) {
  std::vector<rx_patch_slot> ps;
  int64_t tot[4];
  const int rc = patch_check("rx_patch_tracks", n, wp_off, wp, nrm, seg, meta, G, SG, t, p, &ps, tot);
  if (rc != RX_OK) return rc;
  return patch_launch("rx_patch_tracks", ps, tot, wp, nrm, seg, meta, G, SG, t, p, (hipStream_t)stream);
}

int rx_patch_tracks_host(int32_t n, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta,
                         int32_t G, int32_t SG, const rx_cull_tables* t, const rx_track_patch* p, void* /*stream*/) {
  std::vector<rx_patch_slot> ps;
  int64_t tot[4];
  int rc = patch_check("rx_patch_tracks_host", n, wp_off, wp, nrm, seg, meta, G, SG, t, p, &ps, tot);
  if (rc != RX_OK) return rc;
  if ((rc = patch_check_meta("rx_patch_tracks_host", p, p->meta))) return rc;
  if (!t) G = SG = 0;
  for (size_t j = 0; j < ps.size(); ++j) {  // the kernel's steps (rx_cull.hip, k_patch_slots) with one lane
    const rx_patch_slot& d = ps[j];
    const int32_t k = d.slot, W = d.W;
    const double* s = p->seg + 8 * (size_t)d.src0;
    const double* w = p->wp + 2 * (size_t)d.src0;
    const double* m = p->meta + 8 * j;
    rx_cull_copy_rows<2>(w, wp + 2 * (size_t)d.wp0, W, 0, 1);
    rx_cull_copy_rows<2>(p->nrm + 2 * (size_t)d.src0, nrm + 2 * (size_t)d.wp0, W, 0, 1);
    rx_cull_copy_rows<4>(s, seg + 8 * (size_t)d.wp0, 2 * W, 0, 1);
    for (int c = 0; c < 8; ++c) meta[8 * (size_t)k + c] = m[c];
    if (!t) continue;
    rx_cull_slot o = {0, 0, 0, 0, tot[0], tot[1], t->chunk_box, t->super_box, t->wchunk_box, t->wsuper_box,
                      t->chunk_box_f, t->super_box_f};
    double b[4], longest, geo[4] = {0.0, 0.0, 0.0, 0.0};
    rx_cull_extent(s, W, 0, 1, t->seg_f + 8 * (size_t)d.wp0, b, &longest);
    if (G > 0) {
      rx_cull_geo(b, rx_cull_reach(s, W, 0, 1, 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])), longest, geo);
      o.chunk0 = d.chunk0;
      o.super0 = SG > 0 ? d.super0 : 0;
      o.wchunk0 = d.wchunk0;
      o.wsuper0 = d.wsuper0;
      rx_cull_boxes(s, w, W, G, SG, 0, 1, &o);
      for (int c = 0; c < 4; ++c) t->slot_geo[4 * (size_t)k + c] = geo[c];
    }
    rx_cull_header((rx_slot_hdr*)t->slot_hdr + k, d.wp0, W, &o, geo, m);
  }
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

// ---- rendering (ABI v25, additive) ---------------------------------------------
static int raster_static_args(const char* fn, int32_t n, int32_t size, int32_t n_edges, const void* edge_off,
                              const void* edges, const void* layer) {
  if (n <= 0 || n > RX_RASTER_MAX_IMAGES) return fail(RX_EINVAL, "%s: n=%d outside 1..%d", fn, n, RX_RASTER_MAX_IMAGES);
  if (size < RX_RASTER_SIZE_MIN || size > RX_RASTER_SIZE_MAX)
    return fail(RX_EINVAL, "%s: size=%d outside %d..%d", fn, size, RX_RASTER_SIZE_MIN, RX_RASTER_SIZE_MAX);
  if (n_edges < 0) return fail(RX_EINVAL, "%s: n_edges=%d is negative", fn, n_edges);
  if (!edge_off) return fail(RX_EINVAL, "%s: null pointer: edge_off", fn);
  if (!edges) return fail(RX_EINVAL, "%s: null pointer: edges", fn);
  if (!layer) return fail(RX_EINVAL, "%s: null pointer: layer", fn);
  return RX_OK;
}

// frame = 0: what rx_raster_trail reads; 1: what rx_raster_frame reads.
static int raster_io_args(const char* fn, const rx_raster_io* r, int frame) {
  if (!r) return fail(RX_EINVAL, "%s: null pointer: r", fn);
  if (r->size < RX_RASTER_SIZE_MIN || r->size > RX_RASTER_SIZE_MAX)
    return fail(RX_EINVAL, "%s: size=%d outside %d..%d", fn, r->size, RX_RASTER_SIZE_MIN, RX_RASTER_SIZE_MAX);
  if (r->A != 1 && r->A != 2) return fail(RX_EINVAL, "%s: A=%d must be 1 or 2", fn, r->A);
  if (r->K <= 0 || r->K > RX_RASTER_MAX_IMAGES)
    return fail(RX_EINVAL, "%s: K=%d outside 1..%d", fn, r->K, RX_RASTER_MAX_IMAGES);
  if (r->n_envs <= 0) return fail(RX_EINVAL, "%s: n_envs=%d must be > 0", fn, r->n_envs);
#define RX_RASTER_PTR(f) \
  if (!r->f) return fail(RX_EINVAL, "%s: null pointer: " #f, fn)
  RX_RASTER_PTR(env_ids);
  RX_RASTER_PTR(x);
  RX_RASTER_PTR(y);
  RX_RASTER_PTR(view);
  RX_RASTER_PTR(trail);
  if (!frame) {
    RX_RASTER_PTR(last);
    return RX_OK;
  }
  RX_RASTER_PTR(angle);
  RX_RASTER_PTR(layer_of);
  RX_RASTER_PTR(layer);
  RX_RASTER_PTR(out);
  RX_RASTER_PTR(out_off);
#undef RX_RASTER_PTR
  if (r->n_layers <= 0) return fail(RX_EINVAL, "%s: n_layers=%d must be > 0", fn, r->n_layers);
  if (r->out_pitch < 0) return fail(RX_EINVAL, "%s: out_pitch=%lld is negative", fn, (long long)r->out_pitch);
  if (r->out_pitch < 3 * (int64_t)r->size)
    return fail(RX_EINVAL, "%s: out_pitch=%lld below 3*size=%d", fn, (long long)r->out_pitch, 3 * r->size);
  if (r->out_size < 0) return fail(RX_EINVAL, "%s: out_size=%lld is negative", fn, (long long)r->out_size);
  return RX_OK;
}

int rx_raster_static(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                     uint8_t* layer, void* stream) {
  int rc = raster_static_args("rx_raster_static", n, size, n_edges, edge_off, edges, layer);
  if (rc != RX_OK) return rc;
  if ((rc = rx_launch_raster_static(n, size, n_edges, edge_off, edges, layer, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_raster_static: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_raster_trail(const rx_raster_io* r, void* stream) {
  int rc = raster_io_args("rx_raster_trail", r, 0);
  if (rc != RX_OK) return rc;
  if ((rc = rx_launch_raster_trail(r, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_raster_trail: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_raster_frame(const rx_raster_io* r, void* stream) {
  int rc = raster_io_args("rx_raster_frame", r, 1);
  if (rc != RX_OK) return rc;
  if ((rc = rx_launch_raster_frame(r, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_raster_frame: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// The host twins: argument checks here, the loops in rx_raster_host.cpp.
int rx_raster_static_host(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                          uint8_t* layer, void* /*stream*/) {
  const int rc = raster_static_args("rx_raster_static_host", n, size, n_edges, edge_off, edges, layer);
  if (rc != RX_OK) return rc;
  rx_host_raster_static(n, size, n_edges, edge_off, edges, layer);
  return RX_OK;
}

int rx_raster_trail_host(const rx_raster_io* r, void* /*stream*/) {
  const int rc = raster_io_args("rx_raster_trail_host", r, 0);
  if (rc != RX_OK) return rc;
  rx_host_raster_trail(r);
  return RX_OK;
}

int rx_raster_frame_host(const rx_raster_io* r, void* /*stream*/) {
  const int rc = raster_io_args("rx_raster_frame_host", r, 1);
  if (rc != RX_OK) return rc;
  rx_host_raster_frame(r);
  return RX_OK;
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

int rx_ppo_n_params(int32_t obs_dim);  // rx_ppo.hip

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

// ABI v25, additive: league training (csrc/rx_league.h).  The checks of the three entry
// points and their host twins, before any HIP call; what: 0 = weights, 1 = draw, 2 = rollout.
static int league_args(const char* fn, const rx_league_io* lg, int what) {
  if (!lg) return fail(RX_EINVAL, "%s: null league io", fn);
  if (lg->n_slots < 1 || lg->n_slots > 64) return fail(RX_EINVAL, "%s: n_slots=%d outside 1..64", fn, lg->n_slots);
  if (!lg->tally || !lg->cdf) return fail(RX_EINVAL, "%s: null %s", fn, !lg->tally ? "tally" : "cdf");
  if (what == 0) return RX_OK;
  if (lg->agent != 0 && lg->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, lg->agent);
  if (!lg->opp_id || !lg->draw_count)
    return fail(RX_EINVAL, "%s: null %s", fn, !lg->opp_id ? "opp_id" : "draw_count");
  if (what == 1) return RX_OK;
  if (!lg->params || !lg->log_std) return fail(RX_EINVAL, "%s: null %s", fn, !lg->params ? "params" : "log_std");
  if (lg->params_stride < rx_ppo_n_params(19))
    return fail(RX_EINVAL, "%s: params_stride=%lld < the %d parameters of obs_dim 19", fn,
                (long long)lg->params_stride, rx_ppo_n_params(19));
  return precision_arg(fn, "opp_precision", lg->opp_precision);
}

static int league_weights_args(const char* fn, const rx_league_io* lg, int32_t n_live, int32_t power, double mix,
                               double prior) {
  const int rc = league_args(fn, lg, 0);
  if (rc) return rc;
  if (n_live < 1 || n_live > lg->n_slots)
    return fail(RX_EINVAL, "%s: n_live=%d outside 1..n_slots=%d", fn, n_live, lg->n_slots);
  if (power < 0 || power > 4) return fail(RX_EINVAL, "%s: power=%d outside 0..4", fn, power);
  if (!(mix >= 0.0 && mix <= 1.0)) return fail(RX_EINVAL, "%s: mix=%g outside [0, 1]", fn, mix);
  if (!(prior > 0.0)) return fail(RX_EINVAL, "%s: prior=%g must be > 0", fn, prior);
  return RX_OK;
}

static int league_draw_args(const char* fn, const rx_league_io* lg, int64_t n, const float* done, const double* info) {
  const int rc = league_args(fn, lg, 1);
  if (rc) return rc;
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (done && !info) return fail(RX_EINVAL, "%s: null info (required with done)", fn);
  return RX_OK;
}

int rx_league_weights(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior, void* stream) {
  int rc = league_weights_args("rx_league_weights", lg, n_live, power, mix, prior);
  if (rc) return rc;
  if ((rc = rx_launch_league_weights(lg, n_live, power, mix, prior, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_league_weights: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_league_weights_host(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior,
                           void* /*stream*/) {
  const int rc = league_weights_args("rx_league_weights_host", lg, n_live, power, mix, prior);
  if (rc) return rc;
  rx_host_league_weights(lg, n_live, power, mix, prior);
  return RX_OK;
}

int rx_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* stream) {
  int rc = league_draw_args("rx_league_draw", lg, n, done, info);
  if (rc) return rc;
  if ((rc = rx_launch_league_draw(lg, n, done, info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_league_draw: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_league_draw_host(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* /*stream*/) {
  const int rc = league_draw_args("rx_league_draw_host", lg, n, done, info);
  if (rc) return rc;
  rx_host_league_draw(lg, n, done, info);
  return RX_OK;
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

// ABI v25, additive: the track curriculum (csrc/rx_curriculum.h).  The checks of the four entry
// points and their host twins, before any HIP call; what: 0 = tally, 1 = scores, 2 = draw.
static int track_args(const char* fn, const rx_track_io* tc, int what) {
  if (!tc) return fail(RX_EINVAL, "%s: null track io", fn);
  if (tc->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, tc->n_tracks);
  if (what == 0 && (!tc->track || !tc->tally))
    return fail(RX_EINVAL, "%s: null %s", fn, !tc->track ? "track" : "tally");
  if (what == 1) {
    if (!tc->tally || !tc->cdf || !tc->p)
      return fail(RX_EINVAL, "%s: null %s", fn, !tc->tally ? "tally" : !tc->cdf ? "cdf" : "p");
    if (tc->score != 0 && tc->score != 1) return fail(RX_EINVAL, "%s: score=%d must be 0 or 1", fn, tc->score);
  }
  if (what == 2 && (!tc->cdf || !tc->track_of_env))
    return fail(RX_EINVAL, "%s: null %s", fn, !tc->cdf ? "cdf" : "track_of_env");
  return RX_OK;
}

static int track_tally_args(const char* fn, const rx_track_io* tc, int64_t n, const float* done,
                            const uint8_t* terminated, const double* info) {
  const int rc = track_args(fn, tc, 0);
  if (rc) return rc;
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!done || !terminated || !info)
    return fail(RX_EINVAL, "%s: null %s", fn, !done ? "done" : !terminated ? "terminated" : "info");
  return RX_OK;
}

static int track_scores_args(const char* fn, const rx_track_io* tc, int32_t power, double prior) {
  const int rc = track_args(fn, tc, 1);
  if (rc) return rc;
  if (power < 0 || power > 4) return fail(RX_EINVAL, "%s: power=%d outside 0..4", fn, power);
  if (!(prior > 0.0)) return fail(RX_EINVAL, "%s: prior=%g must be > 0", fn, prior);
  return RX_OK;
}

static int track_draw_args(const char* fn, const rx_track_io* tc, int64_t n, double mix) {
  const int rc = track_args(fn, tc, 2);
  if (rc) return rc;
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!(mix >= 0.0 && mix <= 1.0)) return fail(RX_EINVAL, "%s: mix=%g outside [0, 1]", fn, mix);
  return RX_OK;
}

int rx_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated, const double* info,
                   void* stream) {
  int rc = track_tally_args("rx_track_tally", tc, n, done, terminated, info);
  if (rc) return rc;
  if ((rc = rx_launch_track_tally(tc, n, done, terminated, info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_tally: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_tally_host(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                        const double* info, void* /*stream*/) {
  const int rc = track_tally_args("rx_track_tally_host", tc, n, done, terminated, info);
  if (rc) return rc;
  rx_host_track_tally(tc, n, done, terminated, info);
  return RX_OK;
}

int rx_track_scores(const rx_track_io* tc, int32_t power, double prior, void* stream) {
  int rc = track_scores_args("rx_track_scores", tc, power, prior);
  if (rc) return rc;
  if ((rc = rx_launch_track_scores(tc, power, prior, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_scores: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_scores_host(const rx_track_io* tc, int32_t power, double prior, void* /*stream*/) {
  const int rc = track_scores_args("rx_track_scores_host", tc, power, prior);
  if (rc) return rc;
  rx_host_track_scores(tc, power, prior);
  return RX_OK;
}

int rx_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* stream) {
  int rc = track_draw_args("rx_track_draw", tc, n, mix);
  if (rc) return rc;
  if ((rc = rx_launch_track_draw(tc, n, generation, mix, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_draw: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_draw_host(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* /*stream*/) {
  const int rc = track_draw_args("rx_track_draw_host", tc, n, mix);
  if (rc) return rc;
  rx_host_track_draw(tc, n, generation, mix);
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
  if (!io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null io->%s (the tally reads the terminal step's rows)", fn,
                !io->terminated ? "terminated" : "info");
  return rollout_loop(fn, h, io, r, tc, precision, stream);
}

// ABI v25, additive: the track curriculum for self-play (csrc/rx_track_duel.h).  The checks of the
// three entry points and their host twins, before any HIP call.
static int track_duel_io(const char* fn, const rx_track_duel_io* td) {
  if (!td) return fail(RX_EINVAL, "%s: null track duel io", fn);
  if (td->agent != 0 && td->agent != 1) return fail(RX_EINVAL, "%s: agent=%d must be 0 or 1", fn, td->agent);
  if (!td->duel) return fail(RX_EINVAL, "%s: null duel", fn);
  return RX_OK;
}

static int track_tally2_args(const char* fn, const rx_track_io* tc, const rx_track_duel_io* td, int64_t n,
                             const float* done, const uint8_t* terminated, const double* info) {
  int rc = track_args(fn, tc, 0);
  if (rc || (rc = track_duel_io(fn, td)) != 0) return rc;
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!done || !terminated || !info)
    return fail(RX_EINVAL, "%s: null %s", fn, !done ? "done" : !terminated ? "terminated" : "info");
  return RX_OK;
}

static int track_duel_scores_args(const char* fn, const rx_track_io* tc, const rx_track_duel_io* td, int32_t power,
                                  double prior) {
  if (!tc) return fail(RX_EINVAL, "%s: null track io", fn);
  if (tc->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, tc->n_tracks);
  if (!tc->tally || !tc->cdf || !tc->p)
    return fail(RX_EINVAL, "%s: null %s", fn, !tc->tally ? "tally" : !tc->cdf ? "cdf" : "p");
  if (tc->score < 0 || tc->score > 3) return fail(RX_EINVAL, "%s: score=%d outside 0..3", fn, tc->score);
  const int rc = track_duel_io(fn, td);
  if (rc) return rc;
  if (power < 0 || power > 4) return fail(RX_EINVAL, "%s: power=%d outside 0..4", fn, power);
  if (!(prior > 0.0)) return fail(RX_EINVAL, "%s: prior=%g must be > 0", fn, prior);
  return RX_OK;
}

int rx_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                    const uint8_t* terminated, const double* info, void* stream) {
  int rc = track_tally2_args("rx_track_tally2", tc, td, n, done, terminated, info);
  if (rc) return rc;
  if ((rc = rx_launch_track_tally2(tc, td, n, done, terminated, info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_tally2: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_tally2_host(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                         const uint8_t* terminated, const double* info, void* /*stream*/) {
  const int rc = track_tally2_args("rx_track_tally2_host", tc, td, n, done, terminated, info);
  if (rc) return rc;
  rx_host_track_tally2(tc, td, n, done, terminated, info);
  return RX_OK;
}

int rx_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                         void* stream) {
  int rc = track_duel_scores_args("rx_track_duel_scores", tc, td, power, prior);
  if (rc) return rc;
  if ((rc = rx_launch_track_duel_scores(tc, td, power, prior, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_duel_scores: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_duel_scores_host(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                              void* /*stream*/) {
  const int rc = track_duel_scores_args("rx_track_duel_scores_host", tc, td, power, prior);
  if (rc) return rc;
  rx_host_track_duel_scores(tc, td, power, prior);
  return RX_OK;
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
  if (!io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null io->%s (the tally reads the terminal step's rows)", fn,
                !io->terminated ? "terminated" : "info");
  return two_car_rollout_loop(h, io, r, sp, lg, precision, stream, tc, td);
}

// ABI v25, additive: episodic track draws (rx_track_episode, csrc/rx_curriculum.h).  The checks that
// need no handle: rx_track_tally's, rx_track_draw's table and mix, and the episode io.
// table: whether the draw reads tc->cdf (the replay forms read rx_track_learn_io's tables instead).
static int track_episode_args(const char* fn, const rx_track_io* tc, const rx_track_episode_io* ep,
                              bool table = true) {
  const int rc = track_args(fn, tc, 0);
  if (rc) return rc;
  if (table && !tc->cdf) return fail(RX_EINVAL, "%s: null cdf", fn);
  if (!ep) return fail(RX_EINVAL, "%s: null episode io", fn);
  if (!ep->draws) return fail(RX_EINVAL, "%s: null draws", fn);
  if (!ep->env_pos != !ep->pos_slot)
    return fail(RX_EINVAL, "%s: null %s (env_pos and pos_slot: both or neither)", fn,
                !ep->env_pos ? "env_pos" : "pos_slot");
  if (!(ep->mix >= 0.0 && ep->mix <= 1.0)) return fail(RX_EINVAL, "%s: mix=%g outside [0, 1]", fn, ep->mix);
  return RX_OK;
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

int rx_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                     const uint8_t* terminated, const double* info, void* stream) {
  const char* fn = "rx_track_episode";
  int rc = track_episode_args(fn, tc, ep);
  if (rc || (rc = track_tally_args(fn, tc, n, done, terminated, info)) != 0) return rc;
  if ((rc = rx_launch_track_episode(tc, ep, n, done, terminated, info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_episode_host(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                          const uint8_t* terminated, const double* info, void* /*stream*/) {
  const char* fn = "rx_track_episode_host";
  int rc = track_episode_args(fn, tc, ep);
  if (rc || (rc = track_tally_args(fn, tc, n, done, terminated, info)) != 0) return rc;
  rx_host_track_episode(tc, ep, n, done, terminated, info);
  return RX_OK;
}

int rx_track_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_episode_io* ep, const rx_io* io,
                          const float* done, void* stream) {
  const char* fn = "rx_track_episode_step";
  int rc = track_episode_args(fn, tc, ep);
  if (rc || (rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io) return fail(RX_EINVAL, "%s: null io", fn);
  if (!done) done = io->done_f32;
  if (!done || !io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null %s", fn, !done ? "done" : !io->terminated ? "io->terminated" : "io->info");
  rx_track_episode_io e = *ep;
  e.env_pos = h->env_pos.p;
  e.pos_slot = h->pos_slot.p;
  if ((rc = rx_launch_track_episode(tc, &e, h->cfg.n_envs, done, io->terminated, io->info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// the single-agent rollout loop with the tally and the episodic draw (rollout_loop)
int rx_track_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                    const rx_track_episode_io* ep, int32_t* slots, int32_t precision, void* stream) {
  const char* fn = "rx_track_episodic_rollout_steps";
  // the track and episode ios first: their refusals need no handle
  int rc = track_episode_args(fn, tc, ep);
  if (rc) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if ((rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io || !r) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : "rollout io");
  if ((rc = rollout_dims(fn, h, r)) != 0 || (rc = rollout_bufs(fn, r)) != 0) return rc;
  if (!io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null io->%s (the tally reads the terminal step's rows)", fn,
                !io->terminated ? "terminated" : "info");
  rx_track_episode_io e = *ep;
  e.env_pos = h->env_pos.p;
  e.pos_slot = h->pos_slot.p;
  return rollout_loop(fn, h, io, r, tc, precision, stream, &e, slots);
}

// ABI v25, additive: the curriculum's replay scores (csrc/rx_track_replay.h).  The checks of the four
// entry points and their host twins, before any HIP call.
static int learn_null(const char* fn, const char* name) { return fail(RX_EINVAL, "%s: null %s", fn, name); }

static int learn_io(const char* fn, const rx_track_learn_io* lt) {
  if (!lt) return fail(RX_EINVAL, "%s: null track learn io", fn);
  if (lt->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, lt->n_tracks);
  return RX_OK;
}

static int learn_tally_args(const char* fn, const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (lt->kind != 0 && lt->kind != 1) return fail(RX_EINVAL, "%s: kind=%d must be 0 or 1", fn, lt->kind);
  if (!lt->track) return learn_null(fn, "track");
  if (!lt->learn) return learn_null(fn, "learn");
  if (T <= 0) return fail(RX_EINVAL, "%s: T=%d must be > 0", fn, T);
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!adv) return learn_null(fn, "adv");
  return RX_OK;
}

static int learn_fold_args(const char* fn, const rx_track_learn_io* lt, double alpha) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->learn) return learn_null(fn, "learn");
  if (!lt->score) return learn_null(fn, "score");
  if (!lt->seen) return learn_null(fn, "seen");
  if (!(alpha > 0.0 && alpha <= 1.0)) return fail(RX_EINVAL, "%s: alpha=%g outside (0, 1]", fn, alpha);
  return RX_OK;
}

static int learn_tables_args(const char* fn, const rx_track_learn_io* lt, int32_t power, int32_t now) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->score) return learn_null(fn, "score");
  if (!lt->seen) return learn_null(fn, "seen");
  if (!lt->rank) return learn_null(fn, "rank");
  if (!lt->cdf_score) return learn_null(fn, "cdf_score");
  if (!lt->cdf_stale) return learn_null(fn, "cdf_stale");
  if (power < 0 || power > 10) return fail(RX_EINVAL, "%s: power=%d outside 0..10", fn, power);
  if (now < 0) return fail(RX_EINVAL, "%s: now=%d must be >= 0", fn, now);
  return RX_OK;
}

static int learn_draw_args(const char* fn, const rx_track_learn_io* lt, int64_t n, double mix, double stale_mix) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (!lt->cdf_score) return learn_null(fn, "cdf_score");
  if (!lt->track_of_env) return learn_null(fn, "track_of_env");
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!(mix >= 0.0 && mix <= 1.0)) return fail(RX_EINVAL, "%s: mix=%g outside [0, 1]", fn, mix);
  if (!(stale_mix >= 0.0 && stale_mix <= 1.0))
    return fail(RX_EINVAL, "%s: stale_mix=%g outside [0, 1]", fn, stale_mix);
  if (!(mix + stale_mix <= 1.0))
    return fail(RX_EINVAL, "%s: mix + stale_mix = %g + %g above 1", fn, mix, stale_mix);
  if (stale_mix > 0.0 && !lt->cdf_stale) return learn_null(fn, "cdf_stale");
  return RX_OK;
}

int rx_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* stream) {
  int rc = learn_tally_args("rx_track_learn_tally", lt, T, n, adv);
  if (rc) return rc;
  if ((rc = rx_launch_track_learn_tally(lt, T, n, adv, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_learn_tally: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_tally_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* /*stream*/) {
  const int rc = learn_tally_args("rx_track_learn_tally_host", lt, T, n, adv);
  if (rc) return rc;
  rx_host_track_learn_tally(lt, T, n, adv);
  return RX_OK;
}

int rx_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha, void* stream) {
  int rc = learn_fold_args("rx_track_learn_fold", lt, alpha);
  if (rc) return rc;
  if ((rc = rx_launch_track_learn_fold(lt, update, alpha, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_learn_fold: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_fold_host(const rx_track_learn_io* lt, int32_t update, double alpha, void* /*stream*/) {
  const int rc = learn_fold_args("rx_track_learn_fold_host", lt, alpha);
  if (rc) return rc;
  rx_host_track_learn_fold(lt, update, alpha);
  return RX_OK;
}

int rx_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now, void* stream) {
  int rc = learn_tables_args("rx_track_learn_tables", lt, power, now);
  if (rc) return rc;
  if ((rc = rx_launch_track_learn_tables(lt, power, now, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_learn_tables: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_tables_host(const rx_track_learn_io* lt, int32_t power, int32_t now, void* /*stream*/) {
  const int rc = learn_tables_args("rx_track_learn_tables_host", lt, power, now);
  if (rc) return rc;
  rx_host_track_learn_tables(lt, power, now);
  return RX_OK;
}

int rx_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix, double stale_mix,
                        void* stream) {
  int rc = learn_draw_args("rx_track_learn_draw", lt, n, mix, stale_mix);
  if (rc) return rc;
  if ((rc = rx_launch_track_learn_draw(lt, n, generation, mix, stale_mix, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_learn_draw: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_draw_host(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                             double stale_mix, void* /*stream*/) {
  const int rc = learn_draw_args("rx_track_learn_draw_host", lt, n, mix, stale_mix);
  if (rc) return rc;
  rx_host_track_learn_draw(lt, n, generation, mix, stale_mix);
  return RX_OK;
}

// ABI v25, additive: the replay scores on episodic draws -- the tally by per-step slot and the
// episode-end draw from the replay tables (csrc/rx_track_replay.h).  Checks before any HIP call.
static int learn_tally_slots_args(const char* fn, const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                  const int32_t* slots) {
  const int rc = learn_io(fn, lt);
  if (rc) return rc;
  if (lt->kind != 0 && lt->kind != 1) return fail(RX_EINVAL, "%s: kind=%d must be 0 or 1", fn, lt->kind);
  if (!lt->learn) return learn_null(fn, "learn");
  if (T <= 0) return fail(RX_EINVAL, "%s: T=%d must be > 0", fn, T);
  if (n <= 0 || n > INT32_MAX) return fail(RX_EINVAL, "%s: n=%lld must be in 1..2^31-1", fn, (long long)n);
  if (!adv) return learn_null(fn, "adv");
  if (!slots) return learn_null(fn, "slots");
  return RX_OK;
}

int rx_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                               const int32_t* slots, const float* dones, void* stream) {
  const char* fn = "rx_track_learn_tally_slots";
  int rc = learn_tally_slots_args(fn, lt, T, n, adv, slots);
  if (rc) return rc;
  if ((rc = rx_launch_track_learn_tally_slots(lt, T, n, adv, slots, dones, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_tally_slots_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                    const int32_t* slots, const float* dones, void* /*stream*/) {
  const int rc = learn_tally_slots_args("rx_track_learn_tally_slots_host", lt, T, n, adv, slots);
  if (rc) return rc;
  rx_host_track_learn_tally_slots(lt, T, n, adv, slots, dones);
  return RX_OK;
}

// the checks of the replay episodic forms that need no handle: rx_track_episode's but for tc->cdf,
// then the learn io's tables and the two mixes (rx_track_learn_draw's rules)
static int learn_episode_args(const char* fn, const rx_track_io* tc, const rx_track_learn_io* lt,
                              const rx_track_episode_io* ep, double stale_mix) {
  int rc = track_episode_args(fn, tc, ep, false);
  if (rc || (rc = learn_io(fn, lt)) != 0) return rc;
  if (lt->n_tracks != tc->n_tracks)
    return fail(RX_EINVAL, "%s: n_tracks=%d of the track learn io != n_tracks=%d of the track io", fn, lt->n_tracks,
                tc->n_tracks);
  if (!lt->cdf_score) return learn_null(fn, "cdf_score");
  if (!(stale_mix >= 0.0 && stale_mix <= 1.0))
    return fail(RX_EINVAL, "%s: stale_mix=%g outside [0, 1]", fn, stale_mix);
  if (!(ep->mix + stale_mix <= 1.0))
    return fail(RX_EINVAL, "%s: mix + stale_mix = %g + %g above 1", fn, ep->mix, stale_mix);
  if (stale_mix > 0.0 && !lt->cdf_stale) return learn_null(fn, "cdf_stale");
  return RX_OK;
}

int rx_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                           double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                           const double* info, void* stream) {
  const char* fn = "rx_track_learn_episode";
  int rc = learn_episode_args(fn, tc, lt, ep, stale_mix);
  if (rc || (rc = track_tally_args(fn, tc, n, done, terminated, info)) != 0) return rc;
  if ((rc = rx_launch_track_learn_episode(tc, lt, ep, stale_mix, n, done, terminated, info, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_learn_episode_host(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                                double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                                const double* info, void* /*stream*/) {
  const char* fn = "rx_track_learn_episode_host";
  int rc = learn_episode_args(fn, tc, lt, ep, stale_mix);
  if (rc || (rc = track_tally_args(fn, tc, n, done, terminated, info)) != 0) return rc;
  rx_host_track_learn_episode(tc, lt, ep, stale_mix, n, done, terminated, info);
  return RX_OK;
}

int rx_track_learn_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_learn_io* lt,
                                const rx_track_episode_io* ep, double stale_mix, const rx_io* io, const float* done,
                                void* stream) {
  const char* fn = "rx_track_learn_episode_step";
  int rc = learn_episode_args(fn, tc, lt, ep, stale_mix);
  if (rc || (rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io) return fail(RX_EINVAL, "%s: null io", fn);
  if (!done) done = io->done_f32;
  if (!done || !io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null %s", fn, !done ? "done" : !io->terminated ? "io->terminated" : "io->info");
  rx_track_episode_io e = *ep;
  e.env_pos = h->env_pos.p;
  e.pos_slot = h->pos_slot.p;
  if ((rc = rx_launch_track_learn_episode(tc, lt, &e, stale_mix, h->cfg.n_envs, done, io->terminated, io->info,
                                          (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "%s: launch failed: %s", fn, hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

// the single-agent rollout loop with the tally and the episodic draw from the replay tables (rollout_loop)
int rx_track_learn_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                          const rx_track_learn_io* lt, const rx_track_episode_io* ep, double stale_mix,
                                          int32_t* slots, int32_t precision, void* stream) {
  const char* fn = "rx_track_learn_episodic_rollout_steps";
  // the track, learn and episode ios first: their refusals need no handle
  int rc = learn_episode_args(fn, tc, lt, ep, stale_mix);
  if (rc) return rc;
  if ((rc = precision_arg(fn, "precision", precision)) != 0) return rc;
  if ((rc = track_episode_handle(fn, h, tc)) != 0) return rc;
  if (!io || !r) return fail(RX_EINVAL, "%s: null %s", fn, !io ? "io" : "rollout io");
  if ((rc = rollout_dims(fn, h, r)) != 0 || (rc = rollout_bufs(fn, r)) != 0) return rc;
  if (!io->terminated || !io->info)
    return fail(RX_EINVAL, "%s: null io->%s (the tally reads the terminal step's rows)", fn,
                !io->terminated ? "terminated" : "info");
  rx_track_episode_io e = *ep;
  e.env_pos = h->env_pos.p;
  e.pos_slot = h->pos_slot.p;
  return rollout_loop(fn, h, io, r, tc, precision, stream, &e, slots, lt, stale_mix);
}

// ABI v25, additive: track evolution (csrc/rx_track_evolve.h).  The checks of the two entry points and
// their host twins, before any HIP call.
static int evolve_null(const char* fn, const char* name) { return fail(RX_EINVAL, "%s: null %s", fn, name); }

static int evolve_io(const char* fn, const rx_track_evolve_io* ev) {
  if (!ev) return fail(RX_EINVAL, "%s: null track evolve io", fn);
  if (ev->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, ev->n_tracks);
  if (ev->n_spawn < 0 || ev->n_spawn > ev->n_tracks)
    return fail(RX_EINVAL, "%s: n_spawn=%d outside 0..n_tracks=%d", fn, ev->n_spawn, ev->n_tracks);
  if (ev->n_spawn > 0) {
    if (!ev->slots) return evolve_null(fn, "slots");
    if (!ev->plan) return evolve_null(fn, "plan");
  }
  if (!ev->cp_off) return evolve_null(fn, "cp_off");
  return RX_OK;
}

static int evolve_plan_args(const char* fn, const rx_track_evolve_io* ev, double edit_frac) {
  const int rc = evolve_io(fn, ev);
  if (rc) return rc;
  if (!ev->cdf_score) return evolve_null(fn, "cdf_score");
  if (!(edit_frac >= 0.0 && edit_frac <= 1.0))
    return fail(RX_EINVAL, "%s: edit_frac=%g outside [0, 1]", fn, edit_frac);
  return RX_OK;
}

static int evolve_args(const char* fn, const rx_track_evolve_io* ev) {
  const int rc = evolve_io(fn, ev);
  if (rc) return rc;
  if (!ev->cp) return evolve_null(fn, "cp");
  if (!ev->width) return evolve_null(fn, "width");
  if (!ev->cp_off_new) return evolve_null(fn, "cp_off_new");
  if (!ev->cp_new) return evolve_null(fn, "cp_new");
  if (!ev->width_new) return evolve_null(fn, "width_new");
  return RX_OK;
}

int rx_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* stream) {
  int rc = evolve_plan_args("rx_track_evolve_plan", ev, edit_frac);
  if (rc) return rc;
  if (ev->n_spawn == 0) return RX_OK;
  if ((rc = rx_launch_track_evolve_plan(ev, generation, edit_frac, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_evolve_plan: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_evolve_plan_host(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* /*stream*/) {
  const int rc = evolve_plan_args("rx_track_evolve_plan_host", ev, edit_frac);
  if (rc) return rc;
  rx_host_track_evolve_plan(ev, generation, edit_frac);
  return RX_OK;
}

int rx_track_evolve(const rx_track_evolve_io* ev, uint32_t generation, void* stream) {
  int rc = evolve_args("rx_track_evolve", ev);
  if (rc) return rc;
  if ((rc = rx_launch_track_evolve(ev, generation, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_evolve: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_evolve_host(const rx_track_evolve_io* ev, uint32_t generation, void* /*stream*/) {
  const int rc = evolve_args("rx_track_evolve_host", ev);
  if (rc) return rc;
  rx_host_track_evolve(ev, generation);
  return RX_OK;
}

// ABI v25, additive: track evolution in place.  which: 0 classes, 1 inplace, 2 commit.
static int evolve_inplace_args(const char* fn, const rx_track_evolve_inplace_io* ev, int which, double edit_frac) {
  if (!ev) return fail(RX_EINVAL, "%s: null track evolve inplace io", fn);
  if (ev->n_tracks <= 0) return fail(RX_EINVAL, "%s: n_tracks=%d must be > 0", fn, ev->n_tracks);
  if (ev->n_spawn < 0 || ev->n_spawn > ev->n_tracks)
    return fail(RX_EINVAL, "%s: n_spawn=%d outside 0..n_tracks=%d", fn, ev->n_spawn, ev->n_tracks);
  if (which == 1 && !(edit_frac >= 0.0 && edit_frac <= 1.0))
    return fail(RX_EINVAL, "%s: edit_frac=%g outside [0, 1]", fn, edit_frac);
  if (which != 0 && ev->n_spawn == 0) return RX_OK;  // nothing is read
  if (which != 0 && !ev->slots) return evolve_null(fn, "slots");
  if (!ev->cp_off) return evolve_null(fn, "cp_off");
  if (which != 0) {
    if (!ev->cp) return evolve_null(fn, "cp");
    if (!ev->width) return evolve_null(fn, "width");
  }
  if (which == 0 && !ev->cdf_score) return evolve_null(fn, "cdf_score");
  if (which != 2) {
    if (!ev->order) return evolve_null(fn, "order");
    if (!ev->cdf_class) return evolve_null(fn, "cdf_class");
    if (!ev->class_end) return evolve_null(fn, "class_end");
  }
  if (which == 1 && !ev->plan) return evolve_null(fn, "plan");
  if (which != 0) {
    if (!ev->out_off) return evolve_null(fn, "out_off");
    if (!ev->cp_out) return evolve_null(fn, "cp_out");
    if (!ev->width_out) return evolve_null(fn, "width_out");
  }
  return RX_OK;
}

int rx_track_evolve_classes(const rx_track_evolve_inplace_io* ev, void* stream) {
  int rc = evolve_inplace_args("rx_track_evolve_classes", ev, 0, 0.0);
  if (rc) return rc;
  if ((rc = rx_launch_track_evolve_classes(ev, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_evolve_classes: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_evolve_classes_host(const rx_track_evolve_inplace_io* ev, void* /*stream*/) {
  const int rc = evolve_inplace_args("rx_track_evolve_classes_host", ev, 0, 0.0);
  if (rc) return rc;
  rx_host_track_evolve_classes(ev);
  return RX_OK;
}

int rx_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac, void* stream) {
  int rc = evolve_inplace_args("rx_track_evolve_inplace", ev, 1, edit_frac);
  if (rc) return rc;
  if (ev->n_spawn == 0) return RX_OK;
  if ((rc = rx_launch_track_evolve_inplace(ev, generation, edit_frac, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_evolve_inplace: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_evolve_inplace_host(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac,
                                 void* /*stream*/) {
  const int rc = evolve_inplace_args("rx_track_evolve_inplace_host", ev, 1, edit_frac);
  if (rc) return rc;
  if (ev->n_spawn == 0) return RX_OK;
  rx_host_track_evolve_inplace(ev, generation, edit_frac);
  return RX_OK;
}

int rx_track_evolve_commit(const rx_track_evolve_inplace_io* ev, void* stream) {
  int rc = evolve_inplace_args("rx_track_evolve_commit", ev, 2, 0.0);
  if (rc) return rc;
  if (ev->n_spawn == 0) return RX_OK;
  if ((rc = rx_launch_track_evolve_commit(ev, (hipStream_t)stream)) != 0)
    return fail(RX_EHIP, "rx_track_evolve_commit: launch failed: %s", hipGetErrorString((hipError_t)rc));
  return RX_OK;
}

int rx_track_evolve_commit_host(const rx_track_evolve_inplace_io* ev, void* /*stream*/) {
  const int rc = evolve_inplace_args("rx_track_evolve_commit_host", ev, 2, 0.0);
  if (rc) return rc;
  if (ev->n_spawn == 0) return RX_OK;
  rx_host_track_evolve_commit(ev);
  return RX_OK;
}

}  // extern "C"
