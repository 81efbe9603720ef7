// rx_internal.h -- kernel argument block shared by rx_api.cpp (host) and
// rx_kernels.hip (device).  Not part of the public ABI (include/rx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rx.h"
#include "rx_assign_plan.h"  // rx_wave and the schedule thresholds (no HIP: the host-only planner shares them)

#define RX_MODE_STEP 0
#define RX_MODE_RESET 1

// Every per-slot scalar the lane-varying kernels read, in ONE 128-byte record (one
// cache line per env instead of one per table: the slot's waypoint range, its culling
// table offsets, bounding circle and meta).  Built by rx_upload_tracks.
struct rx_slot_hdr {
  int32_t wp0, W, chunk_off, super_off, wchunk_off, wsuper_off, pad0, pad1;
  double geo[4];   // slot_geo: bounding-circle centre x, y, radius, longest segment
  double meta[8];  // rx_upload_tracks meta row
};
static_assert(sizeof(rx_slot_hdr) == 128, "one cache line per slot");

struct rx_track_view {
  const int32_t* wp_off;     // [n+1]
  const double* wp;          // [Wtot][2]
  const double* nrm;         // [Wtot][2]
  const double* seg;         // [2*Wtot][4]
  const double* meta;        // [n][8]
  // raycast culling (derived by rx_upload_tracks)
  const int32_t* chunk_off;  // [n+1] first chunk of each slot (2*ceil(W/G) chunks per slot: left side, right side)
  const double* chunk_box;   // [n_chunks][4] xmin, ymin, xmax, ymax of the chunk's segment end points
  const double* slot_geo;    // [n][4] bounding-circle centre x, y, radius of all boundary points; max |v2|
  // closest-waypoint culling: chunks of RX_WP_CHUNK consecutive waypoints
  const int32_t* wchunk_off; // [n+1]
  const double* wchunk_box;  // [n_wchunks][4]
  // two-level raycast culling: super-chunks of cull_super consecutive chunks
  const int32_t* super_off;  // [n+1] first super-chunk of each slot (both sides)
  const double* super_box;   // [n_super][4] union of the member chunk boxes
  // closest-waypoint super-chunks: RX_WP_SUPER consecutive waypoint chunks
  const int32_t* wsuper_off; // [n+1]
  const double* wsuper_box;  // [n_wsuper][4]
  const float* chunk_box_f;  // chunk_box / super_box in float32, rounded outward (k_rays' packed-f32 box tests),
  const float* super_box_f;  // then 4 quadrant blocks of (near.x, near.y, far.x, far.y) (rx_api.cpp)
  int32_t n_chunk_boxes;     // boxes per block
  int32_t n_super_boxes;
  const float* seg_f;        // [2*Wtot][4] float32 copy of seg (culled raycast: segment pre-filter)
  const rx_slot_hdr* hdr;    // [n] per-slot header (lane-varying kernels)
};

#ifndef RX_WP_CHUNK
#define RX_WP_CHUNK 8  // waypoints per closest-waypoint culling leaf
#endif
#ifndef RX_WP_SUPER
#define RX_WP_SUPER 4  // leaves per waypoint super-chunk
#endif

struct rx_kargs {
  rx_track_view tr;
  rx_state st;                // the engine's working state, position order (element A*p + q is agent q of
                              // env perm[p]); track and speed_weight are the caller's (env order)
  rx_io io;
  const rx_wave* dyn_waves;
  const rx_wave* ray_waves;
  const int32_t* perm;        // env order the kernels read (sorted by slot, then position)
  const double* rel_angles;   // [n_sensors]
  const uint8_t* reset_mask;  // RX_MODE_RESET: [N] or nullptr (= all)
  uint32_t* sort_keys;        // [N] k_dyn writes the sort bin (sort_base[slot] + (waypoint >> sort_shift)) at its perm position, or nullptr
  uint32_t* sort_hist;        // with sort_keys: the REWARD half also counts the bins (the re-sort then skips k_sort_hist), or nullptr
  uint32_t* sort_off;         // with sort_hist: [N] the position's rank within its bin (the count atomic's return + lane rank)
  // with sort_keys, k_step2_pair only (rx_steps' crossing step): the REWARD half also stores the
  // position's env id and new progress -- the row ids and the visiting-order hint that the step's
  // ray waves read AFTER the re-sort has rewritten perm and moved progress; nullptr = no snapshot
  int32_t* rows_snap;         // [N]
  double* hint_snap;          // [N]
  const int32_t* sort_base;   // [n_tracks] first sort bin of each slot (ascending with the slot id)
  int32_t sort_shift;         // waypoints per sort bin = 1 << sort_shift
  // ray_order 2: k_dyn writes the direction-sorted (agent, ray) task ids of
  // each dynamics wave's envs to tasks_out[perm_start*A*R ..]; k_rays reads
  // tasks[task_start + lane] (the same buffer)
  int32_t* tasks_out;
  const int32_t* tasks;
  int32_t n_dyn_waves;
  int32_t n_ray_waves;
  int32_t n_sensors;
  int32_t D;
  int32_t max_steps;
  int32_t autoreset;
  int32_t mode;
  int32_t cull_chunk;         // segments per culling chunk G (0 = brute force over all segments)
  int32_t ray_order;          // rx_config.ray_order
  int32_t cull_super;         // leaves per super-chunk (0 = one-level culling)
  int32_t dyn_lpe;            // k_dyn1 lanes per env (1 or RX_DYN1_LPE_SMALL)
  int32_t argmin_window;      // half-width of the closest-waypoint scan around the previous one
  int32_t wide;               // small N: k_dyn1 one env per wave (dyn_lpe 64), k_rays_wide one ray per wave
  int32_t n_wide_tasks;       // N * A * R ray tasks of k_rays_wide
  double* cs_scratch;         // split step: [N*A][2] cos / sin of the stepped angle, k_kin -> k_step2
  unsigned long long* prof_ts;  // rx_profile: [2][prof_stride] per-wave start / end wall-clock stamps, or nullptr
  int32_t prof_stride;          // waves per stamp array (>= waves of any launch)
  const int32_t* slot_nenv;   // [n_tracks] envs assigned to each slot (ray-major task decode)
  double speed_weight;
  uint64_t seed;
  uint32_t* reset_count;  // [N] (2-car envs), advanced by k_dyn2 at every reset
  int32_t box_quadrants;  // k_rays: single-quadrant waves use the quadrant-ordered box tables (RX_BOX_QUAD=0: off)
  int32_t seg_filter;     // k_rays: float32 pre-filter before each exact segment test (RX_SEG_FILTER=0: off)
  int32_t ray_lpr;        // culled raycast: lanes per ray task (1; 4 for few envs, 16 tasks a ray wave)
  int32_t reward_lpe;     // k_step2<1> REWARD half: lanes per env (1, 2 or 4; more for few envs)
  int32_t lane_tracks;    // lane-varying slots (rx_config.lane_tracks): waves of 64 positions of any slots
  const int32_t* pos_slot;  // with lane_tracks: [N] the slot of the env at each position (the order is fixed)
  int32_t ray_tail_from;  // ray waves >= this one (the dispatch tail) hold 64 / ray_tail_lpr tasks each, cast at
  int32_t ray_tail_lpr;   // ray_tail_lpr lanes per ray (2 or 4); -1 = no tail split (rx_config.ray_tail)
  // rx_set_start_draws (two-car envs): the start-slot order of the env that is the
  // j-th to reset in this launch, in env order, comes from draws[*draw_base + j]
  // (j = reset_rank[e], k_reset_rank) instead of the device hash; nullptr = hash
  const uint32_t* draws;
  int64_t n_draws;
  const int64_t* draw_base;
  const int32_t* reset_rank;
  // Ray inputs: what a ray wave reads of the stepped state (position order) -- st.x, st.y,
  // st.angle (and `tasks` above) in every launch but those of rx_steps' carrying schedule,
  // where they are the step's pose snapshot: the REWARD workgroups of a k_step2_pair launch run
  // later steps' KIN parts, which overwrite the working state under the launch's ray waves.
  const double* ray_x;
  const double* ray_y;
  const double* ray_angle;
  // the culled raycast's visiting-order hint, [N * A] by position: st.progress in every launch
  // but the paired one that casts a crossing step (below), where it is the hint snapshot
  const double* ray_hint;
  // rx_steps' carrying launches: a KIN part (k_kin1 at the head of a window, k_step2_pair's
  // REWARD workgroups after it) also stores its stepped pose here -- the snapshot its step's
  // ray waves read in a later launch -- and its sorted task row to tasks_snap; nullptr = no
  // snapshot
  double* snap_x;
  double* snap_y;
  double* snap_angle;
  int32_t* tasks_snap;
};

// rx_steps' carrying schedule (DESIGN.md §3 "The carried step", "The paired launch"): the
// REWARD workgroups of a k_step2_pair launch also run the next step's KIN part, so k_kin1
// leaves the step; a launch advances up to two steps that way (REWARD k, KIN k + 1, REWARD
// k + 1, KIN k + 2) and its ray workgroups cast the rays of up to two EARLIER-stepped steps,
// whose KIN parts completed in a previous launch -- half the launch boundaries, half the
// drains (the lag-1 schedule; the deep launch below takes this to RX_STEPS_DEPTH steps).
// 0 = a k_kin1 and a k_step2 launch per step.
#ifndef RX_STEPS_CARRY
#define RX_STEPS_CARRY 1
#endif
#ifdef RX_STEPS_PAIR
#error "RX_STEPS_PAIR is retired: the paired launches are the one carrying schedule; RX_STEPS_CARRY=0 selects a k_kin1 and a k_step2 launch per step"
#endif
// The deep launch (DESIGN.md §3 "The deep launch"): a k_step2_pair launch advances up to
// RX_STEPS_DEPTH steps in its REWARD workgroups, ranks the ray tasks of up to as many steps in
// RANK workgroups of its own (off the REWARD+KIN chain) and casts up to as many steps' rays.
// A step's KIN, its ranking and its rays run in three different launches, in that order.
// Same-session A/B at 65,536 envs, 1,000-step calls (profiles/steps_deep/): depth 2 / 4 / 8 =
// 1,257 / 1,373 / 1,403 M env-steps/s against the parent's 1,192 M.
#ifndef RX_STEPS_DEPTH
#define RX_STEPS_DEPTH 8
#endif
#if RX_STEPS_DEPTH < 2 || RX_STEPS_DEPTH > 8
#error "RX_STEPS_DEPTH must be 2 .. 8"
#endif
// 1 = the ranking stays in the KIN parts and every call takes the lag-1 schedule of two
// sub-steps and two ray steps per launch (what calls shorter than RX_STEPS_DEEP_MIN_K take)
#ifndef RX_STEPS_RANK_IN_KIN
#define RX_STEPS_RANK_IN_KIN 0
#endif
// rx_steps calls of fewer steps take the lag-1 schedule: the deep one pays two more launches
// per call (a prologue that casts nothing and a drain that only casts).  20 is the smallest
// measured call length at which the deep schedule is not slower (5 / 10 steps: lag 1 ahead by
// 11 % / 3 %; 20 / 40 steps: depth 4 ahead by 2.5 % / 5 %; profiles/steps_deep/).
#ifndef RX_STEPS_DEEP_MIN_K
#define RX_STEPS_DEEP_MIN_K 20
#endif
// ... and deep calls of fewer steps than this are planned at depth 4: a deeper launch fills and
// drains longer (20 / 40 steps: depth 4 ahead of depth 8 by 7 % / 1.5 %; 100 / 250 / 1,000
// steps: depth 8 ahead by 1.5 % / 1 % / 2.3 %)
#ifndef RX_STEPS_FULL_MIN_K
#define RX_STEPS_FULL_MIN_K 100
#endif
// Rings of the snapshots, by the step's index in the call (pose), by the call's rankings
// (task rows) and by the call's re-sorts (row ids / hint).  In one launch: poses of the steps
// it advances, of those it ranks and of those it casts; the rows it ranks, the rows it casts
// from and the row of the last ranked step before them; the snapshots of the windows of the
// steps it casts (KIN two launches back) and the one its key-writing REWARD stores.
#define RX_PAIR_RING (3 * RX_STEPS_DEPTH)
#define RX_TASK_RING (2 * RX_STEPS_DEPTH + 1)
#define RX_SHADOW_ROWS (RX_STEPS_DEPTH - 1)

// The paired schedule's crossing step (DESIGN.md §3 "The crossing step"): the REWARD of a step
// whose re-sort is due runs as the last sub-step of the launch before it, KIN-less, and its
// rays are cast AFTER the sort, from pre-sort snapshots of the row ids and the visiting-order
// hint -- the re-sort step's own launch leaves the window.  In the deep schedule every step
// still queued at a sort crosses it on that window's snapshots.
// 0 = the re-sort step keeps its own launch (REWARD and rays before the sort).
#ifndef RX_STEPS_CROSS
#define RX_STEPS_CROSS 1
#endif
#define RX_CROSS_RING 3

// What one k_step2_pair launch runs beside rx_kargs (whose io, ray_*, snap_*, tasks,
// tasks_out and tasks_snap it ignores).
struct rx_pair {
  int32_t n_sub;   // REWARD sub-steps of the launch (0 .. RX_STEPS_DEPTH); the sort keys go with the last one
  int32_t n_rays;  // ray steps of the launch (0 .. RX_STEPS_DEPTH), oldest first
  // sub-step j: REWARD on io[j]'s rows, then -- with kin[j] -- KIN on io[j + 1]'s
  rx_io io[RX_STEPS_DEPTH + 1];
  int32_t kin[RX_STEPS_DEPTH];
  double* snap[RX_STEPS_DEPTH];         // KIN j's pose snapshot: x, y at + N, angle at + 2 N
  int32_t* tasks_out[RX_STEPS_DEPTH];   // KIN j's ray-task sort (nullptr = not in the chain), and its second copy
  int32_t* tasks_snap[RX_STEPS_DEPTH];
  // ray step s: the pose snapshot its KIN stored, its task row, and the obs rows it writes
  const double* ray_pose[RX_STEPS_DEPTH];
  const int32_t* ray_tasks[RX_STEPS_DEPTH];
  float* ray_obs[RX_STEPS_DEPTH];
  // ... and its row ids (position -> env: the obs row) and visiting-order hint: rx_kargs' perm
  // and st.progress, or -- a step that crossed a re-sort -- their pre-sort snapshots
  const int32_t* ray_rows[RX_STEPS_DEPTH];
  const double* ray_hint[RX_STEPS_DEPTH];
  int64_t n_envs;
  // rank step t: RANK workgroup (t, b) ranks block b's ray tasks by the angles of the pose
  // snapshot rank_pose[t] (stored by the step's KIN in an EARLIER launch) into rank_row[t],
  // which a LATER launch's ray waves read
  int32_t n_rank;  // 0 .. RX_STEPS_DEPTH
  const double* rank_pose[RX_STEPS_DEPTH];
  int32_t* rank_row[RX_STEPS_DEPTH];
};

extern "C" int rx_launch_step(const rx_kargs* a, int n_agents, int phases, hipStream_t s);
// k_step2_pair (single-agent, one lane per env).  Refuses (hipErrorInvalidValue) a launch that
// writes a snapshot or sorts into a row that one of its own ray steps reads (the row-id and
// hint snapshots of its key-writing REWARD included), and two ray steps that write the same
// obs rows.
extern "C" int rx_launch_step2_pair(const rx_kargs* a, const rx_pair* p, hipStream_t s);
// sizes and field offsets of rx_kargs / rx_pair for a caller that fills them as bytes (see the definition)
extern "C" int64_t rx_pair_layout(int what);
// split step (STEP mode, next-step / no autoreset): k_kin1 / k_kin2, then k_step2<A>
#define RX_SPLIT_KIN 0
#define RX_SPLIT_REWARD 1
#define RX_SPLIT_REWARD_RAYS 2
extern "C" int rx_launch_split(const rx_kargs* a, int n_agents, int part, hipStream_t s);
// persistent small-N rollout (k_rollout): a->n_dyn_waves workgroups, one env
// each, its slot staged in max_w * 96 bytes of dynamic LDS
#define RX_ROLLOUT_MAX_W 1024
extern "C" int rx_launch_rollout(const rx_kargs* a, const rx_rollout_io* r, int max_w, hipStream_t s);
// rx_set_start_draws: ranks (env order) of the envs the next dynamics launch resets
// (mode RX_MODE_RESET: mask[e] or all; RX_MODE_STEP: the next-step autoreset flag of
// the env's working-state row), *base = cursor[0], cursor[0] += their count,
// cursor[1] += the draws missing when the count overruns n_draws
extern "C" int rx_launch_reset_rank(int N, int mode, const uint8_t* mask, const uint8_t* env_flags, const int32_t* perm,
                                    int32_t* tmp, int32_t* rank, int64_t* cursor, int64_t* base, int64_t n_draws,
                                    hipStream_t s);
extern "C" int rx_launch_agent_rows(int N, int D, int q, const float* obs, const float* rew, float* obs_out,
                                    float* rew_out, hipStream_t s);
extern "C" int rx_launch_gae(int T, int N, const float* r, const float* v, const float* d, const float* nv,
                             const float* nd, float g, float gl, float* adv, float* ret, int scan, hipStream_t s);
// rx_track.hip: the track table of n_tracks tracks, a wavefront per track (cp_off on the device)
extern "C" int rx_launch_build_tracks(int n_tracks, int factor, const int32_t* cp_off, const double* cp,
                                      const double* width, double* wp, double* nrm, double* seg, double* meta,
                                      hipStream_t s);
// rx_cull.hip: the culling tables of n_tracks slots, a wavefront per slot.  off (device): wp_off and the
// chunk / super / wchunk / wsuper offset arrays back to back, n_tracks + 1 entries each; n_leaf / n_super:
// the leaf and super box totals (the float tables' block stride); arguments checked by rx_api.cpp
extern "C" int rx_launch_cull_tables(int n_tracks, int G, int SG, const int32_t* off, const double* wp,
                                     const double* seg, const double* meta, const rx_cull_tables* t, int64_t n_leaf,
                                     int64_t n_super, hipStream_t s);
// rx_cull.hip: k_patch_slots, the listed slots rewritten in place (ps: rx_cull.h's rx_patch_slot rows in device
// memory; t may be null: the four table arrays only)
struct rx_patch_slot;
extern "C" int rx_launch_patch_slots(int n_upd, int G, int SG, const rx_patch_slot* ps, const rx_track_patch* p,
                                     double* wp, double* nrm, double* seg, double* meta, const rx_cull_tables* t,
                                     int64_t n_leaf, int64_t n_super, hipStream_t s);
// rx_render.hip: the renderer's three kernels (arguments checked by rx_api.cpp)
extern "C" int rx_launch_raster_static(int n, int size, int n_edges, const int32_t* edge_off, const int32_t* edges,
                                       uint8_t* layer, hipStream_t s);
extern "C" int rx_launch_raster_trail(const rx_raster_io* r, hipStream_t s);
extern "C" int rx_launch_raster_frame(const rx_raster_io* r, hipStream_t s);
// rx_raster_host.cpp: the same three as host loops (plain C++, no HIP call)
extern "C" void rx_host_raster_static(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off,
                                      const int32_t* edges, uint8_t* layer);
extern "C" void rx_host_raster_trail(const rx_raster_io* r);
extern "C" void rx_host_raster_frame(const rx_raster_io* r);
// Adam's per-step scalars for step count s (torch.optim.Adam, non-capturable):
// out[0] = step_size = -lr / (1 - beta1^s), out[1] = sqrt(1 - beta2^s).  Written
// once per optimizer step next to the clip-norm partials (rx_adam_workspace_floats
// counts the 2 floats) by the launch that bumps the step count.
__device__ __forceinline__ void rx_adam_scalars(const rx_adam_config& cfg, float step, double lr, float* out) {
  const double s = (double)step;
  out[0] = (float)(-(lr / (1.0 - pow(cfg.beta1, s))));
  out[1] = (float)sqrt(1.0 - pow(cfg.beta2, s));
}
// torch.optim.Adam's element update (foreach, non-capturable) after the clip
// coefficient: g *= coef; m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g;
// p += step_size * m / (sqrt(v)/bc2_sqrt + eps).  ONE definition for
// k_adam_apply (rx_optim.hip) and the fused minibatch tail (rx_ppo.hip), so both
// optimizer paths round every element identically.
__device__ __forceinline__ void rx_adam_elem(float& g, float& m, float& v, float& p, float coef, float w1, float fb2,
                                             float w2, float eps, float step_size, float bc2_sqrt) {
  g = g * coef;
  m = m + w1 * (g - m);  // torch.lerp, weight < 0.5 branch
  v = v * fb2;
  v = v + w2 * g * g;
  const float den = sqrtf(v) / bc2_sqrt + eps;
  p = p + step_size * (m / den);
}
// The re-sort's bin count for the wave's calling lanes (one per env, key =
// its bin): lanes grouped by bin (ballot), then ONE vector atomic in which
// every group leader adds its group size to hist[bin]; the returned old count
// plus the lane's rank inside its group is the env's rank within its bin --
// the scatter's offset, so k_sort_scatter needs no atomics of its own.
__device__ __forceinline__ uint32_t rx_bin_count(uint32_t* hist, uint32_t key) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long pending = __ballot(1);
  uint32_t cnt = 0, rank = 0;
  int leader_of_mine = lane;
  while (pending) {  // wave-uniform: one iteration per distinct bin of the wave
    const int leader = __builtin_ctzll(pending);
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
    const unsigned long long m = __ballot(key == lb);
    if (key == lb) {
      leader_of_mine = leader;
      rank = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
    if (lane == leader) cnt = (uint32_t)__builtin_popcountll(m);
    pending &= ~m;
  }
  uint32_t old = 0;
  if (cnt) old = atomicAdd(&hist[key], cnt);
  old = (uint32_t)__builtin_amdgcn_ds_bpermute(leader_of_mine << 2, (int)old);
  return old + rank;
}
extern "C" int rx_launch_adam(const rx_adam_config* cfg, float* p, float* g, float* m, float* v, float* step,
                              const double* lr, const uint8_t* stop, float* ws, hipStream_t s);
extern "C" size_t rx_ppo_partial_floats(int obs_dim, int mb);
extern "C" int rx_ppo_n_wg(int mb);
// frag: NULL, or (bf16) the rollout's fragment image from rx_launch_policy_frag
extern "C" int rx_launch_policy_act(const rx_policy_io* io, hipStream_t s, const void* frag = nullptr);
// rx_policy_act with per-row parameters from a bank (k_policy_act_bank); b is validated by the caller
extern "C" int rx_launch_policy_act_bank(const rx_policy_bank_io* b, hipStream_t s);
extern "C" size_t rx_policy_frag_bytes();
extern "C" int rx_launch_policy_frag(int obs_dim, const float* params, void* img, hipStream_t s);
// both self-play policies of a rollout step in one launch (obs_dim 19; k_selfplay_act)
extern "C" int rx_launch_selfplay_act(const rx_policy_io* ag, const rx_policy_io* op, float* obs_out,
                                      const float* rew_src, float* rew_out, int agent, hipStream_t s);
// a league rollout step's policies in one launch (obs_dim 19; k_league_act): op's params / log_std are
// the bank bases, env e's opponent is bank member lg->opp_id[e]; with prev_done (the previous step's done
// flags, prev_info its info rows) the opponent waves first tally and redraw the envs that ended, as
// rx_launch_league_draw would have
extern "C" int rx_launch_league_act(const rx_policy_io* ag, const rx_policy_io* op, const rx_league_io* lg,
                                    const float* prev_done, const double* prev_info, float* obs_out,
                                    const float* rew_src, float* rew_out, hipStream_t s);
// rx_league.hip: tallies -> sampling table; tally + redraw of the opponent ids (arguments checked by rx_api.cpp)
extern "C" int rx_launch_league_weights(const rx_league_io* lg, int n_live, int power, double mix, double prior,
                                        hipStream_t s);
extern "C" int rx_launch_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info,
                                     hipStream_t s);
// rx_league_host.cpp: the same two as host loops (plain C++, no HIP call)
extern "C" void rx_host_league_weights(const rx_league_io* lg, int n_live, int power, double mix, double prior);
extern "C" void rx_host_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info);
// rx_curriculum.hip: per-slot tally of the envs that ended; tallies -> integer sampling table; env -> slot draw
// (arguments checked by rx_api.cpp)
extern "C" int rx_launch_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                                     const double* info, hipStream_t s);
extern "C" int rx_launch_track_scores(const rx_track_io* tc, int power, double prior, hipStream_t s);
extern "C" int rx_launch_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, hipStream_t s);
// rx_curriculum_host.cpp: the same three as host loops (plain C++, no HIP call)
extern "C" void rx_host_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                                    const double* info);
extern "C" void rx_host_track_scores(const rx_track_io* tc, int power, double prior);
extern "C" void rx_host_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix);
// the episodic draw: the tally plus the next slot of every env that ended, on the device and as a host loop
extern "C" int rx_launch_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n,
                                       const float* done, const uint8_t* terminated, const double* info,
                                       hipStream_t s);
extern "C" void rx_host_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n,
                                      const float* done, const uint8_t* terminated, const double* info);
// the two-car tally and the scores over its win columns (rx_track_duel.h), on the device and as host loops
extern "C" int rx_launch_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                                      const uint8_t* terminated, const double* info, hipStream_t s);
extern "C" int rx_launch_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int power, double prior,
                                           hipStream_t s);
extern "C" void rx_host_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                                     const uint8_t* terminated, const double* info);
extern "C" void rx_host_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int power, double prior);
// rx_track_replay.hip: advantages -> per-slot (samples, mag_q); the score fold; rank + the two integer tables;
// the three-way env -> slot draw (arguments checked by rx_api.cpp)
extern "C" int rx_launch_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                           hipStream_t s);
extern "C" int rx_launch_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha, hipStream_t s);
extern "C" int rx_launch_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now, hipStream_t s);
extern "C" int rx_launch_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                                          double stale_mix, hipStream_t s);
// the tally by per-step slot and the episodic draw from the replay tables (rx_track_learn_tally_slots,
// rx_track_learn_episode), on the device and as host loops
extern "C" int rx_launch_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                                 const int32_t* slots, const float* dones, hipStream_t s);
extern "C" int rx_launch_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt,
                                             const rx_track_episode_io* ep, double stale_mix, int64_t n,
                                             const float* done, const uint8_t* terminated, const double* info,
                                             hipStream_t s);
extern "C" void rx_host_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                                const int32_t* slots, const float* dones);
extern "C" void rx_host_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt,
                                            const rx_track_episode_io* ep, double stale_mix, int64_t n,
                                            const float* done, const uint8_t* terminated, const double* info);
// rx_track_replay_host.cpp: the same four as host loops (plain C++, no HIP call)
extern "C" void rx_host_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv);
extern "C" void rx_host_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha);
extern "C" void rx_host_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now);
extern "C" void rx_host_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                                         double stale_mix);
// rx_track_evolve.hip: the plan of the spawned slots; the new control-point buffer (arguments checked by rx_api.cpp)
extern "C" int rx_launch_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac,
                                           hipStream_t s);
extern "C" int rx_launch_track_evolve(const rx_track_evolve_io* ev, uint32_t generation, hipStream_t s);
// rx_track_evolve_host.cpp: the same two as host loops (plain C++, no HIP call)
extern "C" void rx_host_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac);
extern "C" void rx_host_track_evolve(const rx_track_evolve_io* ev, uint32_t generation);
// the in-place form (rx_track_evolve.hip; rx_track_evolve_host.cpp)
extern "C" int rx_launch_track_evolve_classes(const rx_track_evolve_inplace_io* ev, hipStream_t s);
extern "C" int rx_launch_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation,
                                              double edit_frac, hipStream_t s);
extern "C" int rx_launch_track_evolve_commit(const rx_track_evolve_inplace_io* ev, hipStream_t s);
extern "C" void rx_host_track_evolve_classes(const rx_track_evolve_inplace_io* ev);
extern "C" void rx_host_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation,
                                             double edit_frac);
extern "C" void rx_host_track_evolve_commit(const rx_track_evolve_inplace_io* ev);
extern "C" int rx_launch_adv_stats(const rx_ppo_batch* b, int n_mb, float* stats, double* moments, hipStream_t s);
extern "C" int rx_adv_chunks(int mb);
extern "C" int rx_launch_adv_stats_ws(const rx_ppo_batch* b, int n_mb, double* ws, float* stats, double* moments,
                                      hipStream_t s);
extern "C" int rx_launch_adv_finalize(const double* moments, int n_mb, int64_t count, float* stats, hipStream_t s);
extern "C" int rx_launch_kl_check(const float* kl, float kl_target, uint8_t* stop, float* kl_at_stop, hipStream_t s);
extern "C" int rx_launch_ppo_grad(const rx_ppo_batch* b, int m, float scale, uint8_t* stop, float* kl_at_stop,
                                  float* kl_out, float* partial, double* klp, float* grad, hipStream_t s,
                                  const rx_adam_config* cfg = nullptr, float* norm_ws = nullptr,
                                  float* step = nullptr, const double* lr = nullptr);
extern "C" int rx_ppo_reduce_blocks(int obs_dim);
extern "C" int rx_launch_adam_apply(const rx_adam_config* cfg, float* p, float* g, float* m, float* v, float* step,
                                    const double* lr, const uint8_t* stop, float* ws, int nb, hipStream_t s);
// spatial re-sort (rx_sort.hip): counting sort of the perm positions by the
// bin keys the REWARD half wrote; hist must be zero on entry and is left zero
// (at most RX_SORT_MAX_BINS bins, rx_assign_plan.h)
// and moves the working state rows with their envs (perm, work -> perm_tmp,
// tmp -> back); rx_state_sync: working copy <-> the caller's arrays
extern "C" int rx_sort_envs(const uint32_t* keys, uint32_t* off, int n, int A, uint32_t* hist, uint32_t* cursor, int nbins,
                            int32_t* perm, int32_t* perm_tmp, const rx_state* work, const rx_state* tmp,
                            hipStream_t s, int hist_done = 0);
extern "C" int rx_launch_permutation(int64_t n, uint64_t seed, int64_t* out, hipStream_t s);
extern "C" int rx_state_sync(const rx_state* work, const rx_state* user, const int32_t* perm, int n, int A,
                             int to_user, hipStream_t s);
// positions regrouped by slot (rx_sort.hip; include/rx.h rx_regroup_plan): the stable order of the
// positions by (pos_slot, position) and what follows from it, in `scratch` of rx_regroup_scratch_size(n)
// bytes; rx_launch_regroup_move: the single-agent working rows gathered by src into the shadow copy
// and copied back with the new perm and pos_slot
extern "C" size_t rx_regroup_scratch_size(int n);
extern "C" int rx_launch_regroup_plan(int n, int n_tracks, const int32_t* perm, const int32_t* pos_slot,
                                      int32_t* src_out, int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out,
                                      void* scratch, hipStream_t s);
extern "C" int rx_launch_regroup_move(int n, const int32_t* src, const int32_t* perm_tmp, int32_t* perm,
                                      const int32_t* slot_tmp, int32_t* pos_slot, const rx_state* work,
                                      const rx_state* tmp, hipStream_t s);
// rx_eval_steps' per-step metric accumulation (rx_eval.hip): one lane per env position,
// x / y / flags from the working state (position order), the rest in env order
extern "C" int rx_launch_eval_acc(int n, int A, const int32_t* perm, const rx_state* work, const rx_io* io,
                                  double* acc, uint8_t* active, int32_t* n_active, hipStream_t s);
