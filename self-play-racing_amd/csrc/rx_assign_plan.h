// rx_assign_plan.h -- the assignment as a pure function (rx_assign_plan_host.cpp): the
// launch schedule rx_assign resolves from rx_config and the env order and wave tables it
// builds, from a few integers.  No HIP: rx_internal.h includes this header for rx_wave
// and the thresholds, the planner unit is plain C++, and rx_api.cpp uploads a plan.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "rx.h"

// One wavefront's work item: 64 consecutive tasks of ONE track slot.
//  dyn waves: lane -> env perm[perm_start + lane], lane < count
//  ray waves: lane -> task task_start + lane (task = env_local*A*R + agent*R + ray),
//             env = perm[perm_start + env_local]
struct rx_wave {
  int32_t track;
  int32_t perm_start;
  int32_t task_start;
  int32_t count;
};

// lanes per env in k_dyn1 (a dynamics wave holds 64 / lpe envs): 4 when there
// are few envs (latency-bound: more lanes per env shorten the chain), 1 when
// the chip is fuller.  One lane per env also selects the split step (k_kin1 +
// k_step2: the REWARD half beside the raycast), which beats k_dyn1<4> + k_rays
// from 4,096 envs on (41.4 vs 52.8 us at 4,096, 42.7 vs 54.3 at 8,192; equal
// at 2,048, where the wide kernels run anyway: tools/gpu_lpe_ab.sh)
#define RX_DYN1_LPE_SMALL 4
#define RX_DYN1_SMALL_N 2048
// Lanes per ray task (ray_order 2): 4 (16 tasks a ray wave) up to
// RX_RAY_LPR4_N (env, agent) pairs, 2 up to RX_RAY_LPR2_N, 1 above: with few
// envs the raycast is a latency chain over too few waves to fill the chip
// ("Lanes per ray"; crossovers measured on MI355X)
#ifndef RX_RAY_LPR4_N
#define RX_RAY_LPR4_N 8192
#endif
#ifndef RX_RAY_LPR2_N
#define RX_RAY_LPR2_N 16384
#endif
// k_step2<1>'s REWARD half at 2 lanes per env up to this many envs (it is the
// launch's critical path there once the raycast runs at 4 lanes per ray;
// from 8,192 envs on it only slows the raycast beside it)
#ifndef RX_REWARD_LPE2_N
#define RX_REWARD_LPE2_N 4096
#endif
// two-car envs: k_step2<2>'s REWARD half with a lane per car (one closest-waypoint
// pass per wave instead of two) up to this many envs.  Same-session A/B
// (profiles/r04/ab_two_car_*.jsonl): 4,096 envs 67.2 -> 79.2 M env-steps/s,
// 8,192 128.1 -> 134.7 M (with one lane per ray), 16,384 213.2 -> 220.3 M,
// 65,536 389 -> 387 M (off there)
#ifndef RX_REWARD2_LPE2_N
#define RX_REWARD2_LPE2_N 16384
#endif
// two-car envs: 2 lanes per ray only up to this many (env, car) pairs (the
// single-agent RX_RAY_LPR2_N band is empty for them: with the REWARD half at a
// lane per car, 8,192 envs run 134.7 M at 1 lane per ray vs 128.6 M at 2)
#ifndef RX_RAY2_LPR2_N
#define RX_RAY2_LPR2_N 8192
#endif
// Ray-wave dispatch order (rx_assign's placement of the ray-wave table, ray_order 2).
// Class j of a 64-env group = its j-th wave of direction-sorted tasks (the cars of a
// group head alike, so class j ~ sensor ray j: the edge classes look sideways, the
// centre ones down the track and cost ~1.3x).  0 = group-octet-major (round 2),
// 1 = class-major centre classes first, 2 = class-major ascending j, 3 = class-major
// EDGE classes first, the centre ones last (default: 65,536 envs 752 -> 826-833 M
// env-steps/s, 4,096 envs +3 %, same session, DESIGN.md §3 "Ray-wave dispatch order").
#ifndef RX_RAY_DISPATCH
#define RX_RAY_DISPATCH 3
#endif
// rx_config.ray_tail / ray_tail_lpr automatic values: the last RX_RAY_TAIL classes of the
// dispatch order cast at RX_RAY_TAIL_LPR lanes per ray (0 = no tail split)
#ifndef RX_RAY_TAIL
#define RX_RAY_TAIL 0
#endif
#ifndef RX_RAY_TAIL_LPR
#define RX_RAY_TAIL_LPR 2
#endif
// rx_config.task_sort automatic value: the ray-task direction sort every other
// dynamics launch up to this many (env, car) pairs, every launch above.  Same-session
// A/B (profiles/r04/ab_task_sort.txt): 4,096 single-agent envs 129.8 / 128.9 ->
// 132.3 / 132.7 M env-steps/s (k_kin1 6.2 -> 3.6 us), 8,192 two-car envs 135.1 / 136.7
// -> 137.2 / 138.8 M; 65,536 envs 833 -> 804-810 M (every 4th / 8th: 761 / 715 M) and
// 65,536 two-car envs -0.5 %: the stale order costs more ray work than the sort
#ifndef RX_TASK_SORT2_PAIRS
#define RX_TASK_SORT2_PAIRS 16384
#endif
// at most this many single-agent envs: one env per dynamics wave and one ray
// per raycast wave (k_rays_wide), brute force over the lanes -- the kernels
// are latency chains there, and 64 lanes shorten them
#define RX_WIDE_N 2048
// the spatial re-sort's key space (rx_sort.hip): at most this many bins over all slots
#define RX_SORT_MAX_BINS 65536

// The schedule an assignment resolves (rx_env::sched; rx_schedule reports it).
struct rx_sched {
  bool split = true;         // the split step (k_kin1 + k_step2) where it applies (rx_config.split)
  int32_t dyn_lpe = 1;       // k_dyn1 lanes per env: 64 / dyn_lpe envs a dynamics wave (64 = the wide kernels)
  int32_t ray_lpr = 1;       // lanes per ray task (ray_order 2, not wide): 64 / ray_lpr tasks a ray wave
  int32_t reward_lpe = 1;    // split step, single-agent: lanes per env in k_step2's REWARD half
  int32_t argmin_window = 2;
  int32_t ray_dispatch = RX_RAY_DISPATCH;  // resolved class order of the ray-wave table (rx_config.ray_dispatch)
  int32_t ray_tail = 0, ray_tail_lpr = 2;  // tail classes cast at ray_tail_lpr lanes per ray (0 = none)
  int32_t ray_tail_from = -1;              // first ray wave of the tail (-1 = none)
  int32_t task_sort = 1;                   // ray-task direction sort every task_sort dynamics launches
  int32_t lane_tracks = 0;                 // lane-varying slots (rx_config.lane_tracks; two-car handles:
                                           // rx_set_lane_cars -- the plan's choice either way)
  bool sort_on = false;                    // spatial re-sort: sort_bins bins of 1 << sort_shift waypoints
  int32_t sort_bins = 0, sort_shift = 0;   // (both 0 without it)
  int32_t n_dyn_waves = 0, n_ray_waves = 0;
};

// What rx_assign uploads: the schedule, the env order and the two wave tables.
struct rx_assignment {
  rx_sched sched;
  std::vector<int32_t> perm;               // [N] env id at each position: grouped by slot, env order inside a slot
  std::vector<int32_t> slot_n;             // [n_tracks] envs per slot
  std::vector<rx_wave> dyn, ray;
  std::vector<int32_t> pos_slot, env_pos;  // lane-varying: [N] slot at each position, position of each env
  std::vector<int32_t> sort_base;          // sort_on: [n_tracks] first bin of each slot
};

// rx_config's ranges (everything rx_create checks without a device).  RX_OK, or the
// code with the message in *err.
int rx_config_check(const rx_config* cfg, std::string* err);

// The assignment of track_of_env [n_envs] over n_tracks slots of wp_off[k + 1] - wp_off[k]
// waypoints.  RX_OK, or a refusal (config range, slot id, ray_order 2 sensor count) with
// the message in *err and *out as it was.  lane_cars: a two-car handle's lane-varying option
// (rx_set_lane_cars: -1 off, 0 auto, 1 on; rx_config.lane_tracks never reaches two-car envs), which
// single-agent configs ignore; outside -1 .. 1 it is refused.
int rx_plan_assignment(const rx_config& cfg, int32_t n_tracks, const int32_t* wp_off, const int32_t* track_of_env,
                       rx_assignment* out, std::string* err, int32_t lane_cars = -1);

// rx_regroup_plan_host's body (rx_regroup_plan_host.cpp): the positions of a lane-varying env
// regrouped by slot, a stable sort by (pos_slot[p], p).  RX_OK, or RX_EINVAL with the message in
// *err and nothing written.  The outputs must not overlap the inputs.
int rx_plan_regroup(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot, int32_t* src_out,
                    int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out, std::string* err);

// rx_schedule's row (int32 [RX_SCHEDULE_W]) of a resolved schedule.
void rx_sched_row(const rx_config& cfg, const rx_sched& s, int32_t dyn_calls, int32_t* out);
