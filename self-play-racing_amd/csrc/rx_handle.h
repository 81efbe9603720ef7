// rx_handle.h -- private to the C ABI layer (the rx_api*.cpp files; no .hip includes it): the
// handle, its self-freeing device buffers, the error state's entry points and the helpers that
// cross those files.  Everything declared here has hidden visibility: librx.so exports include/rx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rx.h"
#include "rx_cull.h"
#include "rx_internal.h"

#pragma GCC visibility push(hidden)

// rx_api.cpp: the message becomes rx_last_error() of the calling thread; returns code
int fail(int code, const char* fmt, ...);
// RX_OK, or RX_EHIP with "<fn>: launch failed: <the HIP error rc>"
int launched(const char* fn, int rc);

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
  int32_t lane_cars = -1;  // rx_set_lane_cars (two-car handles): -1 off, 0 auto, 1 on; rx_assign resolves it
  rx_sched sched;  // the schedule the assignment resolved (rx_assign_plan.h): written whole, after the last upload
  DevBuf<int32_t> pos_slot;                // with lane_tracks: [N] slot of the env at each position
  DevBuf<int32_t> env_pos;                 // with lane_tracks: [N] position of each env, the inverse of perm
                                           // (rx_track_episode_step: the episodic draw rewrites pos_slot)
  // rx_regroup_slots (lane_tracks, single-agent; reserved by rx_assign so the call allocates nothing):
  // the sort's scratch, src [N] and the new pos_slot [N] before the copy back (the new perm goes to perm[1])
  DevBuf<uint8_t> regroup_scratch;
  DevBuf<int32_t> regroup_src, regroup_slot;
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

// rx_api.cpp: the kernel arguments of a handle, and rx_reset / rx_step's launches
void make_kargs(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, rx_kargs& a);
int launch(rx_env* h, const rx_io* io, int mode, const uint8_t* mask, void* stream, int phases = 3);

// Argument checks that more than one file runs.  fn is the entry point's name; every check
// returns before any HIP call.
// rx_api_loops.cpp
int precision_arg(const char* fn, const char* field, int32_t precision);
// rx_api_tracks.cpp: the table checks and launches rx_upload_tracks_device / rx_replace_tracks_device share
int cull_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* seg, const void* meta,
               int32_t G, int32_t SG, const rx_cull_tables* out, bool sizes_only, std::vector<int32_t>* off,
               int64_t tot[4]);
int cull_launch(const char* fn, int32_t n, const std::vector<int32_t>& off, const int64_t tot[4], const double* wp,
                const double* seg, const double* meta, int32_t G, int32_t SG, const rx_cull_tables* t, hipStream_t s);
int patch_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* nrm, const void* seg,
                const void* meta, int32_t G, int32_t SG, const rx_cull_tables* t, const rx_track_patch* p,
                std::vector<rx_patch_slot>* ps, int64_t tot[4]);
int patch_check_meta(const char* fn, const rx_track_patch* p, const double* meta_h);
int patch_launch(const char* fn, const std::vector<rx_patch_slot>& ps, const int64_t tot[4], double* wp, double* nrm,
                 double* seg, double* meta, int32_t G, int32_t SG, const rx_cull_tables* t, const rx_track_patch* p,
                 hipStream_t s);
// rx_api_curriculum.cpp: the handle-free checks of the ios that the *_rollout_steps and *_episode_step entries take
int league_args(const char* fn, const rx_league_io* lg, int what);
int track_args(const char* fn, const rx_track_io* tc, int what, int max_score = 1);
int track_duel_io(const char* fn, const rx_track_duel_io* td);
int track_episode_args(const char* fn, const rx_track_io* tc, const rx_track_episode_io* ep, bool table = true);
int learn_episode_args(const char* fn, const rx_track_io* tc, const rx_track_learn_io* lt,
                       const rx_track_episode_io* ep, double stale_mix);

#pragma GCC visibility pop
