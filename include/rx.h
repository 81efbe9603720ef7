/* rx.h -- C ABI of the MI355X racing-env engine (librx.so).
 *
 * The reference (LucasHJin/self-play-racing) is pure Python and has no FFI; its
 * hot path is the per-env Gymnasium step loop that agent/ppo.py drives through
 * gymnasium.vector.SyncVectorEnv.  This header is the boundary a maintainer
 * binds (ctypes stub: INTEGRATION.md) to replace that loop with one batched
 * device call.  Each entry point names the reference interface it replaces.
 *
 * Conventions
 *  - Every function returns RX_OK (0) or a negative RX_E* code; rx_last_error()
 *    returns a thread-local message for the last failure on this thread.
 *  - "dev" pointers are device memory owned by the CALLER (e.g. torch tensors);
 *    the library never frees them.  Host arrays are read during the call only.
 *  - Work is enqueued on the caller's stream (a hipStream_t passed as void*,
 *    NULL = the legacy default stream) with no host synchronisation, so the
 *    step can sit inside a captured hipGraph.
 *  - One host thread per handle; handles are independent (one per GPU rank).
 *  - Agents: A = 1 (environment/racing_env.py RacingEnv) or A = 2
 *    (environment/multi_racing_env.py MultiRacingEnv with 2 cars).
 *    Observation width D = n_sensors + 4 + 4*(A-1)   (racing_env.py:37-42,
 *    multi_racing_env.py:38).
 *  - All env arithmetic is binary64 in the reference's operation order; see
 *    DESIGN.md §Parity for the two libm calls (sin/cos, pow(x,2)) whose
 *    results may differ from glibc's by 1 ulp.
 */
#ifndef RX_H_
#define RX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RX_OK 0
#define RX_EINVAL (-1)   /* bad argument / shape / state */
#define RX_EHIP (-2)     /* HIP runtime error */
#define RX_ENOMEM (-3)   /* device allocation failed */
#define RX_ESTATE (-4)   /* call order: tracks/assignment/state not set */

#define RX_ABI_VERSION 25
#define RX_EP_SHARDS 64  /* episode-statistics accumulator rows (rx_io.ep_stats) */

/* state flag bits (rx_state.flags, per agent) */
#define RX_F_CRASHED 1u      /* Car.crashed                      car.py:22,80 */
#define RX_F_FINISHED 2u     /* Car.finished                     racing_env.py:147 */
#define RX_F_CP25 4u         /* checkpoints[0.25]                racing_env.py:21-25 */
#define RX_F_CP50 8u         /* checkpoints[0.50] */
#define RX_F_CP75 16u        /* checkpoints[0.75] */
#define RX_F_HAS_CRASHED 32u /* agents_data['has_crashed']       multi_racing_env.py:147,192-194 */
/* env flag bits (rx_state.env_flags, per env) */
#define RX_EF_PENDING_RESET 1u /* episode ended last step: next-step autoreset */

/* autoreset modes (gymnasium 1.x SyncVectorEnv: NEXT_STEP is its default) */
#define RX_AUTORESET_NEXT_STEP 0 /* step after a terminal one resets, reward 0 */
#define RX_AUTORESET_SAME_STEP 1 /* terminal step returns the reset obs (SB3 style) */
#define RX_AUTORESET_DISABLED 2  /* caller resets explicitly (rx_reset) */

/* info columns (rx_io.info, f64 [N][A][RX_INFO_W]) */
#define RX_INFO_W 4
#define RX_INFO_SPEED 0          /* info['speed']          racing_env.py:80 */
#define RX_INFO_PROGRESS 1       /* info['progress'] (1.0 once finished) :81,158-159 */
#define RX_INFO_PROGRESS_DELTA 2 /* info['progress_delta'] :157 (single-agent) */
#define RX_INFO_PLACEMENT 3      /* info['placement'] (0 = none) multi_racing_env.py:210-211,252-259 */

typedef struct rx_env rx_env;

typedef struct {
  int32_t n_envs;          /* N */
  int32_t n_agents;        /* A: 1 or 2 */
  int32_t n_sensors;       /* rays per agent (11 in train.py:47-49,94-101) */
  int32_t max_steps;       /* truncation, 3000 (racing_env.py:162) */
  int32_t autoreset;       /* RX_AUTORESET_* */
  int32_t device;          /* HIP device ordinal */
  uint64_t seed;           /* device RNG (two-car start-slot shuffle) */
  double sensor_half_cone; /* pi/3 (racing_env.py:45) or pi/2 (multi_racing_env.py:50) */
  double speed_weight;     /* RacingEnv.speed_weight, 8.0 (racing_env.py:9,26) */
  int32_t cull_chunk;      /* raycast culling: segments per chunk (16 recommended; 0 = test every segment) */
  int32_t sort_interval;   /* re-sort envs by track position every k dynamics launches (0 = never): a
                              counting sort by (slot, waypoint bin), rx_sort.hip; scheduling only.  Skipped
                              when the pool has more than 65,536 slots (at most ~1 env per slot). */
  int32_t ray_order;       /* raycast lane order: 0 = (env, agent, ray), 11 rays of ~6 envs per wave;
                              1 = ray-major: one (agent, ray) of 64 consecutive envs per wave -- with
                              sort_interval > 0 those envs are track neighbours, so a wave's rays are
                              nearly parallel and share culling chunks; 2 = sorted ray tasks: every
                              step the dynamics kernel orders the A*R tasks of each 64-env wave by the
                              absolute direction of the ray (64 sectors, LDS counting sort), so a ray
                              wave holds rays with nearby origins and nearly equal directions.
                              Scheduling only: same results. */
  int32_t cull_super;      /* two-level raycast culling: chunks per super-chunk box (0 = one level) */
  /* ABI v17: launch schedule.  Scheduling only -- every setting gives bit-identical results (the tests
     force each path) -- so 0 = automatic (the measured best for the env count) everywhere; -1 = off /
     none where a field has an off state.  Out-of-range values fail rx_create with RX_EINVAL.  These
     replace the RX_* environment variables earlier versions read: the library reads no environment. */
  int32_t split;           /* split step (k_kin + k_step2: REWARD beside the raycast): 0 auto (on), 1 on, -1 off */
  int32_t wide_n;          /* wide kernels (a wave per env / per ray) up to this many single-agent envs:
                              0 auto (2,048), -1 never, > 0 the threshold */
  int32_t dyn_lpe;         /* k_dyn1 lanes per env: 0 auto, or 1, 2, 4, 64 */
  int32_t ray_lpr;         /* lanes per ray task (ray_order 2): 0 auto (4 / 2 / 1 by (env, car) pairs; two cars:
                              4 / 1), or 1, 2, 4 */
  int32_t reward_lpe;      /* k_step2 REWARD lanes per env: 0 auto (single agent: 2 up to 4,096 envs; two cars:
                              2 = a lane per car up to 16,384 envs), or 1, 2, 4 (two cars: 1 or 2) */
  int32_t argmin_window;   /* closest-waypoint scan half-width around the previous one: 0 auto (2), -1 none,
                              1 .. 32 */
  int32_t seg_filter;      /* float32 pre-filter before each exact segment test: 0 auto (on), 1 on, -1 off */
  int32_t box_quadrants;   /* quadrant-ordered float32 box tables for single-quadrant ray waves: 0 auto (on),
                              1 on, -1 off */
  /* ABI v19: ray-wave dispatch (ray_order 2).  Class j of a 64-env group = its j-th wave of
     direction-sorted ray tasks (the group's cars head alike, so class j ~ sensor ray j). */
  int32_t ray_dispatch;    /* order in which the classes are dispatched: 0 auto (3), 1 centre classes first,
                              2 ascending j, 3 edge classes first / centre last, -1 group-octet-major */
  int32_t ray_tail;        /* the LAST ray_tail classes of that order (the tail of the launch, whose waves
                              run as the chip drains) cast at ray_tail_lpr lanes per ray: each of their
                              64-task waves becomes ray_tail_lpr waves of 64 / ray_tail_lpr tasks.  Only
                              with 1 lane per ray elsewhere.  0 auto, -1 none, 1 .. 16 */
  int32_t ray_tail_lpr;    /* 0 auto (2), 2 or 4 */
  /* ABI v20: the dynamics kernel re-sorts each block's ray tasks by direction every task_sort
     launches (and after every spatial re-sort); in between the ray waves keep the previous
     order.  0 auto (2 up to 16,384 (env, car) pairs, 1 above), 1 .. 16 */
  int32_t task_sort;
  /* ABI v23: lane-varying track slots.  Normally every wavefront holds envs of ONE track slot, so its
     track-table reads are wave-uniform scalar loads; a pool of many distinct tracks (SURVEY.md §8(d)'s
     stress variant: gen_tracks(N, seed=None), one slot per env) then leaves a wave with one env.  With
     lane_tracks on, the single-agent kernels take waves of 64 consecutive envs of ANY slots and every lane
     reads its own slot's tables with vector loads (culling decisions per lane).  0 auto: on when grouping
     by slot would fill the dynamics waves less than half on average (more than 2 x ceil(N / 64) waves);
     1 on; -1 off.  Single-agent envs on the split step at one lane per env and per ray only (wide kernels:
     off; two-car envs: this field has no effect on them, their switch is rx_set_lane_cars, off unless
     called).  Scheduling only: bit-identical results. */
  int32_t lane_tracks;
  int32_t reserved0;       /* ABI v23: must be 0 (was kin_sort, a dropped A/B schedule) */
} rx_config;

/* Per-env / per-agent SoA state, caller-owned device memory.  [N*A] arrays are
 * agent-minor: element e*A + a.  Mirrors Car (car.py:15-24), RacingEnv
 * (racing_env.py:17-26), MultiRacingEnv.agents_data (multi_racing_env.py:
 * 142-148) and RecordEpisodeStatistics' episode counters.
 * The engine steps a working copy of these arrays kept in wave order (ABI
 * v15: coalesced state traffic; see rx_state_import / rx_state_export): the
 * bound arrays are read at rx_bind_state / rx_assign and otherwise only
 * synchronised on request.  track and speed_weight are read in place. */
typedef struct {
  double* x;             /* [N*A] */
  double* y;             /* [N*A] */
  double* angle;         /* [N*A] */
  double* vx;            /* [N*A] */
  double* vy;            /* [N*A] */
  double* progress;      /* [N*A] Car.progress */
  double* last_progress; /* [N*A] */
  double* last_steering; /* [N*A] */
  int32_t* finished_step;/* [N*A] -1 = None (A==2 only; may be NULL for A==1) */
  uint8_t* flags;        /* [N*A] RX_F_* */
  int32_t* steps;        /* [N] */
  int32_t* track;        /* [N] track slot: set by rx_assign, read-only for the step kernels; rewritten per
                            env by rx_track_episode (episodic track draws) when its episode ends */
  uint8_t* env_flags;    /* [N] RX_EF_* */
  double* ep_return;     /* [N] episode return of agent 0 */
  int32_t* ep_length;    /* [N] */
  const double* speed_weight; /* [N] per-env RacingEnv.speed_weight, or NULL = rx_config.speed_weight */
} rx_state;

/* One step's inputs/outputs, caller-owned device memory.  NULL = not wanted
 * (except actions/obs, which are required). */
typedef struct {
  const float* actions;  /* [N][A][2] float32, as the Box(float32) action space */
  float* obs;            /* [N][A][D] float32 */
  float* reward;         /* [N][A] float32 (rollout buffer dtype, agent/ppo.py:116-117) */
  double* reward64;      /* [N][A] float64 (SyncVectorEnv's reward dtype) */
  uint8_t* terminated;   /* [N] */
  uint8_t* truncated;    /* [N] */
  float* done_f32;       /* [N] float(terminated | truncated): next_done, agent/ppo.py:120 */
  double* info;          /* [N][A][RX_INFO_W] */
  uint8_t* ep_done;      /* [N] an episode ended this step (infos['_episode']) */
  double* ep_stats;      /* [RX_EP_SHARDS][4] += (sum return, sum length, count, -) of episodes ended;
                            the caller sums the shard rows */
  unsigned long long* counters; /* [4] profiling, NULL = off: += per wave (raycast chunk tests,
                                   raycast chunks scanned, waypoint chunk tests, waypoint chunks scanned) */
} rx_io;

const char* rx_last_error(void);
int rx_abi_version(void);

/* Create/destroy a handle.  Replaces gym.vector.SyncVectorEnv([...]) construction,
 * agent/ppo.py:70,85-95. */
int rx_create(const rx_config* cfg, rx_env** out);
int rx_destroy(rx_env* h);

/* Host copy of the sensor angle offsets the kernels use: [n_sensors] =
 * np.linspace(-half_cone, half_cone, n_sensors) (racing_env.py:45). */
int rx_sensor_angles(const rx_env* h, double* out);

/* Diagnostics (ABI v15): the env id at each position of the current wave
 * order (envs grouped by slot, re-sorted by track position every
 * sort_interval dynamics launches), host array [n_envs]; synchronises the
 * device.  *sort_bins / *sort_shift (either may be NULL) receive the spatial
 * sort's bin count and waypoints-per-bin shift (0 bins = no re-sort).  The
 * reference has no counterpart (its SyncVectorEnv steps envs in order). */
int rx_env_order(rx_env* h, int32_t* perm_out, int32_t* sort_bins, int32_t* sort_shift);

/* Diagnostics (ABI v17, v19, v20): the launch schedule rx_assign resolved from rx_config
 * for this handle, out int32 [RX_SCHEDULE_W] = split step (0/1), wide kernels
 * (0/1), k_dyn1 lanes per env, lanes per ray task, REWARD lanes per env,
 * closest-waypoint window half-width, segment pre-filter (0/1), quadrant box
 * tables (0/1), dynamics waves, ray waves, ray-wave dispatch order, tail
 * classes, tail lanes per ray, first tail wave (-1 = none), ray-task sort interval, lane-varying
 * track slots (0/1, ABI v23), dynamics launches so far (the re-sort cadence counter: the launch
 * with count % sort_interval == 0 writes the re-sort keys; ABI v21), 0 (reserved).  Host only,
 * no device call. */
#define RX_SCHEDULE_W 18
int rx_schedule(const rx_env* h, int32_t* out);

/* Track table (host arrays, copied to the device).  Replaces the per-env
 * Track.__init__ geometry (environment/track.py:61-148): slot k has
 * W_k = wp_off[k+1]-wp_off[k] waypoints and 2*W_k boundary segments.
 *   wp_off int32 [n+1];  wp, nrm f64 [Wtot][2];
 *   seg f64 [2*Wtot][4] = (start.x, start.y, v2.x, v2.y): left boundary
 *       segments then right ones, per slot (track.py:134-148);
 *   meta f64 [n][8] = start x, y, angle (Track.get_start_pos, track.py:154-157),
 *       track_width, max_track_distance (track.py:88-91), normals[0].x,
 *       normals[0].y, 0. */
int rx_upload_tracks(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* nrm,
                     const double* seg, const double* meta);

/* Assign a track slot to every env (host int32 [N]); also written to
 * state.track.  Replaces Track(track_pool, track_id, track_width) per env
 * (train.py:47-49,94-101).  Groups envs by slot so a wavefront shares one
 * track (segment loads become scalar/broadcast). */
int rx_assign(rx_env* h, const int32_t* track_of_env);

/* The assignment as a pure function (no device, no handle; additive to ABI v25): what
 * rx_assign would resolve and build for a handle created with *cfg over n_tracks slots of
 * wp_off[k + 1] - wp_off[k] waypoints (host int32 [n_tracks + 1]) and track_of_env (host
 * int32 [n_envs]).  rx_assign uploads exactly this plan, so the tables that decide which lane
 * casts which ray can be checked on the CPU.  Refusals are rx_create's range checks of *cfg
 * (cfg->device is not looked at) and rx_assign's own (a slot id out of range, more than 16
 * sensors at ray_order 2), with the same codes and rx_last_error texts; a refused call
 * writes nothing.  Sizes by cap and count, as rx_ray_waves: the call always writes
 * n_dyn_waves and n_ray_waves, and nothing else unless schedule, perm, dyn_waves and
 * ray_waves are set and the two caps suffice. */
typedef struct {
  int32_t dyn_cap, ray_cap;         /* in: records that dyn_waves / ray_waves can hold */
  int32_t n_dyn_waves, n_ray_waves; /* out: the tables' lengths */
  int32_t sort_bins, sort_shift;    /* out: as rx_env_order reports them (0 bins = no re-sort) */
  int32_t* schedule;                /* [RX_SCHEDULE_W], rx_schedule's layout; dynamics launches so far = 0 */
  int32_t* perm;                    /* [n_envs] the env order before any re-sort (rx_env_order) */
  int32_t* dyn_waves;               /* [dyn_cap][4] (track slot or -1 = lane-varying, perm start, 0, env count) */
  int32_t* ray_waves;               /* [ray_cap][4] as rx_ray_waves */
  /* optional, NULL = not wanted: */
  int32_t* slot_n;                  /* [n_tracks] envs per slot (the ray-major decode's stride) */
  int32_t* pos_slot;                /* [n_envs] lane-varying schedules: the slot at each position, */
  int32_t* env_pos;                 /* [n_envs] and the position of each env; otherwise left as they are */
  int32_t* sort_base;               /* [n_tracks] with sort_bins > 0: the first bin of each slot */
} rx_assign_plan_io;
int rx_assign_plan(const rx_config* cfg, int32_t n_tracks, const int32_t* wp_off, const int32_t* track_of_env,
                   rx_assign_plan_io* io);

/* Lane-varying track slots for two-car envs (additive to ABI v25; DESIGN.md §3 "Lane-varying two-car
 * envs").  rx_config.lane_tracks governs single-agent handles only; a two-car handle takes the same
 * schedule -- dynamics waves of 64 consecutive positions of ANY slots, every lane reading its own
 * slot's tables, one lane per env, per ray and per REWARD env, no ray-task sort, no spatial re-sort,
 * bit-identical results -- from this option, in rx_config.lane_tracks' encoding: -1 off (a fresh
 * handle), 0 auto (on when grouping by slot needs more than 2 x ceil(N / 64) dynamics waves), 1 on.
 * The call only records the choice: the next rx_assign resolves it, and every later one again, so
 * under 0 a new assignment may switch the schedule on or off.  RX_EINVAL for a null handle, a mode
 * outside -1 .. 1, and a single-agent handle (rx_config.lane_tracks governs it).  On such a handle
 * rx_schedule's lane-varying word is 1; its ray-wave table is block-major without padding records
 * (per 64-position block ceil(count * 2 * n_sensors / 64) waves, task_start relative to the block). */
int rx_set_lane_cars(rx_env* h, int32_t mode);

/* rx_assign_plan with that option: the plan of a two-car handle on which rx_set_lane_cars(h,
 * lane_cars) was called (rx_assign_plan is this with -1).  n_agents = 1: RX_EINVAL. */
int rx_assign_plan_cars(const rx_config* cfg, int32_t lane_cars, int32_t n_tracks, const int32_t* wp_off,
                        const int32_t* track_of_env, rx_assign_plan_io* io);

/* Bind the caller-owned device state (pointers are kept until re-bound).
 * Once both rx_bind_state and rx_assign have run, the engine copies the bound
 * arrays into its working copy (blocking). */
int rx_bind_state(rx_env* h, const rx_state* st);

/* ABI v15.  The engine keeps the env state in wave order (position p holds
 * env rx_env_order()[p]) so its kernels read and write it coalesced, and
 * moves it with each spatial re-sort.  rx_state_export writes the working
 * copy to the bound arrays (env order) -- call before reading them;
 * rx_state_import reads the bound arrays into the working copy -- call after
 * writing them (state injection).  Both are enqueued on `stream` (a
 * hipStream_t, NULL = legacy default) without a host sync.  The reference
 * keeps this state in per-env Python objects (car.py:15-24, racing_env.py:
 * 17-26), always current. */
int rx_state_import(rx_env* h, void* stream);
int rx_state_export(rx_env* h, void* stream);

int rx_set_speed_weight(rx_env* h, double speed_weight);

/* Reset envs (mask: device uint8 [N], NULL = all).  Replaces
 * SyncVectorEnv.reset -> RacingEnv.reset (racing_env.py:86-102) /
 * MultiRacingEnv.reset (multi_racing_env.py:118-153).  Writes obs (and zeros
 * reward/terminated/truncated/done_f32 of the reset envs when given). */
int rx_reset(rx_env* h, const uint8_t* mask, const rx_io* io, void* stream);

/* ABI v20.  The two-car start-slot order from the reference's own RNG stream:
 * MultiRacingEnv.reset draws it with np.random.shuffle(agent_order) on the
 * global numpy RNG (multi_racing_env.py:127-128), one MT19937 output u per
 * reset (j = u & 1: the two cars swap when j == 0), and SyncVectorEnv resets
 * its envs in env order.  With draws set, the env that is the j-th to reset in
 * a launch (env order: rx_reset's mask, or the next-step autoreset of rx_step)
 * takes draws[cursor[0] + j], and the launch advances cursor[0] by its reset
 * count.  draws: device uint32 [n_draws], the caller's upcoming MT19937 outputs
 * (e.g. np.random.randint(0, 2**32, n, dtype=np.uint32) from a copy of the
 * global state); cursor: device int64 [2], cursor[1] += the draws a launch
 * needed beyond n_draws (those resets are then wrong: refill and redo).
 * draws = NULL restores the device hash.  Two-car handles, next-step or no
 * autoreset (same-step autoreset draws inside the step: RX_EINVAL). */
int rx_set_start_draws(rx_env* h, const uint32_t* draws, int64_t n_draws, int64_t* cursor);

/* One vectorised step.  Replaces SyncVectorEnv.step -> RecordEpisodeStatistics
 * -> RacingEnv.step (racing_env.py:104-167) / SelfPlayWrapper.step ->
 * MultiRacingEnv.step (multi_racing_env.py:213-269), with the configured
 * autoreset semantics. */
int rx_step(rx_env* h, const rx_io* io, void* stream);

/* ABI v21.  n_steps consecutive steps from one call, each equal to an rx_step of
 * the io rows at that step (bit for bit: the same kernels' arithmetic on the same
 * rows).  Step s reads actions + s * strides->actions and writes obs + s *
 * strides->obs, reward + s * strides->reward, ... (element strides; a stride of 0
 * writes every step into the same rows, which then hold the last step's outputs;
 * strides = NULL: all 0; with stride-0 rows a step's kernels may write next-step
 * columns while an earlier step's are still being written, so such rows are
 * defined once the call's work has completed on the stream, not between its
 * launches).  ep_stats and counters accumulate.  The actions of all
 * n_steps steps must be in device memory when the call is made: open-loop
 * action sequences (the env-throughput benchmark: a bank of random actions) --
 * a policy-in-the-loop rollout is rx_rollout_steps.  Replaces n_steps iterations
 * of SyncVectorEnv.step (agent/ppo.py:112) with precomputed actions. */
typedef struct {
  int64_t actions, obs, reward, reward64, terminated, truncated, done_f32, info, ep_done;
} rx_io_strides;
int rx_steps(rx_env* h, const rx_io* io, int32_t n_steps, const rx_io_strides* strides, void* stream);

/* The launch schedule of an rx_steps call on a single-agent split-step handle, as a pure
 * function (no device, no handle; additive to ABI v25): the launches of K steps, in order.
 * A step passes through a KIN part (behind the REWARD of the step before it, or a k_kin1
 * launch at the head of the call and after every re-sort), a REWARD part, optionally a
 * ranking of its ray tasks, and its ray cast; rx_steps turns the records into pointers.
 * Slots index rings: pose 3 * depth (by step), task rows 2 * depth + 1 (by ranking; -1 = the
 * handle's task buffer), crossing snapshots RX_PLAN_CROSS_RING (by re-sort; -1 = the live
 * row ids and progress), shadow obs rows depth - 1 (-1 = the caller's rows).
 * rx_steps_plan fills at most `cap` records and returns how many the call has (< 0: bad
 * arguments); record 0 is the prologue: no launch, only kin1_after = 0. */
#define RX_PLAN_MAX_DEPTH 8
#define RX_PLAN_CROSS_RING 3
typedef struct {
  int32_t n_steps;        /* K >= 1 */
  int32_t depth;          /* sub-steps, rank steps and ray steps per launch: 2 .. RX_PLAN_MAX_DEPTH; 0 = what
                             rx_steps takes for a call of n_steps (written back) */
  int32_t sort_interval;  /* 0 = no re-sort; step s is a re-sort step when (dyn_calls + s) % sort_interval == 0 */
  int32_t dyn_calls;      /* the handle's dynamics launches so far (any value with the right phase) */
  int32_t task_sort;      /* rank every task_sort-th step and after every re-sort; 0 = the handle ranks nothing */
  int32_t task_calls;     /* the handle's ranking turns so far (phase) */
  int32_t tasks_stale;    /* the handle's task buffer is stale: the next step is ranked */
  int32_t cross;          /* steps may stay queued across a re-sort (snapshots available) */
  int32_t rank_in_kin;    /* 1 = the lag-1 schedule: KIN parts rank, rays are cast one launch after the KIN;
                             -1 = what rx_steps takes for a call of n_steps (written back) */
  /* out: */
  int32_t ranked;           /* steps ranked by the call */
  int32_t tasks_stale_out;  /* the handle's task buffer is stale after the call */
} rx_plan_args;
typedef struct {
  int32_t n_sub, n_rank, n_rays;
  int32_t first_step;                    /* sub-step j is REWARD first_step + j */
  int32_t kin[RX_PLAN_MAX_DEPTH];        /* ... followed by KIN first_step + j + 1 */
  int32_t kin_pose[RX_PLAN_MAX_DEPTH];   /* pose slot that KIN stores */
  int32_t kin_row[RX_PLAN_MAX_DEPTH];    /* rank_in_kin: task row that KIN ranks into, or -1 */
  int32_t keys;                          /* the last REWARD is a re-sort step's: it writes the sort keys */
  int32_t keys_snap;                     /* ... and this crossing snapshot, or -1 (nothing stays queued) */
  int32_t rank_step[RX_PLAN_MAX_DEPTH], rank_pose[RX_PLAN_MAX_DEPTH], rank_row[RX_PLAN_MAX_DEPTH];
  int32_t ray_step[RX_PLAN_MAX_DEPTH], ray_pose[RX_PLAN_MAX_DEPTH], ray_row[RX_PLAN_MAX_DEPTH];
  int32_t ray_snap[RX_PLAN_MAX_DEPTH], ray_shadow[RX_PLAN_MAX_DEPTH];
  int32_t sort_after;                    /* the re-sort runs behind this launch */
  int32_t kin1_after;                    /* then a k_kin1 launch of this step (-1: none) */
  int32_t kin1_pose, kin1_row;           /* its pose slot; rank_in_kin: its task row or -1 */
} rx_plan_launch;
int32_t rx_steps_plan(rx_plan_args* args, rx_plan_launch* out, int32_t cap);

/* rx_step split into its two kernels, for per-kernel timing with stream
 * events: phases bit 0 = dynamics/reward/done/autoreset (k_dyn), bit 1 =
 * raycast observations (k_rays).  rx_step == phases 3.  Running bit 1 alone
 * recomputes the ray observations of the current state. */
#define RX_PHASE_DYNAMICS 1
#define RX_PHASE_RAYS 2
int rx_step_phases(rx_env* h, const rx_io* io, int32_t phases, void* stream);

/* Kernel timing for benchmarks.  While profiling, every wave of a recorded
 * launch stamps the device wall clock (s_memrealtime, 100 MHz, one chip-wide
 * counter) at its start and end; a launch's duration is last end - first
 * start: its execution span, as rocprofv3 --kernel-trace measures it, without
 * the dispatch and end-of-kernel cache-flush time that stream events around a
 * launch include.  rx_profile(h, 1) starts a fresh record of the kernels that
 * rx_step / rx_reset / rx_step_phases launch (up to 512 launches; the call
 * synchronises the device), rx_profile(h, 0) pauses recording and
 * rx_profile(h, 2) resumes it (record selected steps only), rx_profile_read
 * synchronises and returns per kernel kind the mean duration (ms) and the
 * launch count.  No counterpart in the reference (it has no benchmarks). */
#define RX_KERNEL_DYN 0    /* k_dyn1 / k_dyn2: one-kernel dynamics (reset, small N, two-car) */
#define RX_KERNEL_RAYS 1   /* k_rays launched on its own (rx_step_phases, one-kernel step) */
#define RX_KERNEL_KIN 2    /* k_kin1: first kernel of the split step */
#define RX_KERNEL_STEP2 3  /* k_step2: REWARD half + raycast in one launch (split step) */
#define RX_KERNEL_REWARD 4 /* k_step2 with the REWARD half only (rx_step_phases dynamics) */
#define RX_KERNEL_KINDS 5
int rx_profile(rx_env* h, int32_t enable);
int rx_profile_read(rx_env* h, double* mean_ms, int32_t* count);
/* Diagnostics (ABI v18): the raw per-wave stamps of recorded launch `launch`
 * (0-based, record order; synchronises).  *n_waves = the launch's wave slots
 * (wave index = workgroup index for k_step2: REWARD waves first, then the ray
 * waves); start[i] / end[i] = device wall-clock ticks (0 = no wave in that
 * slot) for i < min(*n_waves, cap); *kind = its RX_KERNEL_*; *khz = the clock
 * rate.  Used to see how a launch's waves fill the chip over time (tail,
 * per-wave cost by dispatch order).  No counterpart in the reference. */
int rx_profile_waves(rx_env* h, int32_t launch, uint64_t* start, uint64_t* end, int32_t cap, int32_t* n_waves,
                     int32_t* kind, int32_t* khz);
/* Diagnostics (ABI v19): the ray-wave table rx_assign built, host int32 [cap][4]
 * = (track slot, perm start, first task, task count) per ray wave in dispatch
 * order (wave i is k_step2 workgroup n_reward + i, k_rays workgroup i);
 * *n_waves = the table length.  A wave's class j within its 64-env group is
 * (first task - perm start * A * n_sensors) / 64 (ray_order 2, 1 lane per ray
 * outside the tail).  Host only, no device call.  No counterpart in the
 * reference. */
int rx_ray_waves(const rx_env* h, int32_t* out, int32_t cap, int32_t* n_waves);
/* Diagnostics (ABI v22): the device ray-task list the last sorting launch wrote
 * (ray_order 2: per 64-env block its A * n_sensors task ids (A p + q) R + r in
 * direction-sector order), copied to host int32 out[cap] after the stream
 * drains; *n = its length (N * A * n_sensors).  cap = 0 queries *n only. */
int rx_ray_tasks(rx_env* h, int32_t* out, int64_t cap, int64_t* n, void* stream);

/* GAE (agent/ppo.py:134-154), float32, bit-exact lane-per-env recurrence.
 * rewards/values/dones [T][N]; next_value/next_done [N]; adv/returns [T][N]. */
int rx_gae(int32_t T, int32_t N, const float* rewards, const float* values, const float* dones,
           const float* next_value, const float* next_done, double gamma, double gae_lambda, float* advantages,
           float* returns, void* stream);

/* Same recurrence evaluated as a wavefront-parallel affine scan over T
 * (chunks of T per lane, combined with a 64-lane prefix scan): for few envs
 * and long horizons.  Not bit-exact (different association); |error| <=
 * ~1e-6 * max|A| (tests/test_gae_gpu.py). */
int rx_gae_scan(int32_t T, int32_t N, const float* rewards, const float* values, const float* dones,
                const float* next_value, const float* next_done, double gamma, double gae_lambda, float* advantages,
                float* returns, void* stream);

/* Track table builders (ABI v24), handle-free like rx_gae.  They replace the
 * per-track Track.__init__ geometry (environment/track.py:61-148: two scipy
 * CubicSpline solves and a chain of numpy calls per track) with one call for
 * n_tracks tracks and write the rx_upload_tracks layout above.
 *   inputs : factor (waypoints per control point; the reference uses 30);
 *            cp_off HOST int32 [n+1], cp_off[0] = 0: track k owns control points
 *            cp[cp_off[k] .. cp_off[k+1]) -- P_k of them, 3 <= P_k <= 64;
 *            cp f64 [cp_off[n]][2]; width f64 [n].
 *   outputs: wp_off HOST int32 [n+1] (filled by the call: wp_off[k] =
 *            cp_off[k] * factor, W_k = P_k * factor); wp, nrm f64 [Wtot][2];
 *            seg f64 [2*Wtot][4]; meta f64 [n][8].
 * Geometry (csrc/rx_spline.h): the chord-length periodic cubic spline of
 * track.py:100-115 -- the knot derivatives from the cyclic tridiagonal system
 * by Sherman-Morrison over two Thomas sweeps, scipy's power-basis coefficients
 * and evaluation order -- sampled at np.linspace(0, t[-1], W, endpoint=False),
 * then track.py:82-96,117-148 operation for operation.  scipy solves the system
 * through LAPACK, so the waypoints agree with the reference's to rounding
 * (a few ulp of the coordinates), not bit for bit; nrm, seg and
 * meta are exact functions of the waypoints.  Two columns of meta differ from
 * the reference's numpy expressions in the last bit at most: meta[2] uses the
 * platform's atan2 (ocml on the device, libm on the host), and meta[4] squares
 * with x * x where numpy's scalar ** 2 calls pow.  rx.track overwrites both
 * with the numpy expressions.
 *
 * rx_build_tracks: cp, width and the four outputs are DEVICE pointers.  Checks
 * everything the host can see before any launch (RX_EINVAL, the message names
 * the track and the field): P < 3 or P > 64, factor < 1, W above the limit of
 * rx_upload_tracks, a table above int32 rows.  The launch is enqueued on
 * `stream` and the call does not wait for it; the (n+1) offsets travel through
 * a stream-ordered allocation (hipMallocAsync / hipMemcpyAsync from the
 * caller's pageable array / hipFreeAsync), so the call is not capturable into
 * a hipGraph.  What lives in device memory cannot be checked without a wait: a
 * track with a non-finite coordinate, a zero-length chord or a negative width
 * gets meta[k][4] = NaN, which rx_upload_tracks refuses.
 *
 * rx_build_tracks_host: the same arguments with HOST pointers (`stream` is
 * ignored), the same rx_spline.h code in a plain loop.  It makes no HIP call,
 * so it works on a machine with no GPU, and it checks the data too: RX_EINVAL
 * for a non-finite coordinate, a zero-length chord (two consecutive control
 * points coincide; scipy raises there too) and a negative width, before
 * anything is written.  Its output equals the device's bit for bit except
 * meta[2] (atan2 above). */
int rx_build_tracks(int32_t n_tracks, int32_t factor, const int32_t* cp_off, const double* cp, const double* width,
                    int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, void* stream);
int rx_build_tracks_host(int32_t n_tracks, int32_t factor, const int32_t* cp_off, const double* cp,
                         const double* width, int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta,
                         void* stream);

/* ABI v25, additive: the culling tables of a track table, handle-free like the
 * builders above, and the device-resident door into a handle.  rx_upload_tracks
 * derives these tables from its host arrays; the entry points below derive the
 * same tables from a table that already lives in device memory (rx_build_tracks),
 * so it is never downloaded.  The rules live in csrc/rx_cull.h, shared by the
 * kernel (csrc/rx_cull.hip), the host twin and rx_upload_tracks; DESIGN.md §3.
 *
 * Per slot k with W = wp_off[k+1] - wp_off[k] waypoints and its 2 W boundary
 * segments (left side, then right side), G = cull_chunk, S = cull_super:
 *   leaf boxes   per side ceil(W / G) boxes (xmin, ymin, xmax, ymax) over both end
 *                points of G consecutive segments: 2 ceil(W / G) per slot, left first;
 *   super boxes  (S > 0) per side the union of S consecutive leaf boxes;
 *   wchunk boxes the box of RX_WP_CHUNK = 8 consecutive waypoints; wsuper boxes the
 *                union of RX_WP_SUPER = 4 consecutive wchunk boxes;
 *   *_off [n+1]  first box of each slot in the four box arrays (running sums);
 *   slot_geo     [n][4] = centre of the box of all segment end points, a radius
 *                r * (1 + 1e-12) + 1e-9 with r the largest hypot distance from the
 *                centre to an end point, and l * (1 + 1e-12) + 1e-12 with l the
 *                longest segment sqrt(v2.x * v2.x + v2.y * v2.y);
 *   chunk_box_f, super_box_f  float [5][count][4]: block 0 the boxes in float32
 *                rounded outward (min corner towards -inf, max corner towards +inf),
 *                block 1 + q the same boxes as (near.x, near.y, far.x, far.y) for a
 *                ray whose x (bit 0 of q) / y (bit 1) direction is negative;
 *   seg_f        float [2*Wtot][4], seg rounded to nearest;
 *   slot_hdr     [n] rows of 128 bytes: int32 wp_off[k], W, chunk_off[k],
 *                super_off[k], wchunk_off[k], wsuper_off[k], 0, 0; then f64
 *                slot_geo[k][0..3], meta[k][0..7].
 * G <= 0: only seg_f and slot_hdr are written (offsets and geo in the rows are 0)
 * and the other pointers may be null.  S == 0: no super tables (super_off,
 * super_box and super_box_f may be null, the rows hold 0).
 *
 * rx_cull_table_sizes: out[4] = the leaf, super, wchunk and wsuper box counts of
 * the whole table.  Host only, no HIP call.
 * rx_build_cull_tables_host: every pointer is a HOST pointer; no HIP call.
 * rx_build_cull_tables: wp_off is a HOST array; wp, seg, meta and every pointer of
 * `out` are DEVICE pointers.  One launch (a wavefront per slot) enqueued on
 * `stream`; the call does not wait for it.  The offset arrays are computed on the
 * host and travel as rx_build_tracks' do (stream-ordered allocation: not
 * capturable).  Both write the same values, with one exception: slot_geo[k][2] and
 * its copy in the row use the platform's hypot (ocml / libm), so the device's
 * radius agrees with the host's to 1e-13 relative and stays an upper bound of the
 * exact one.  Zeros may differ in sign (min / max of +0.0 and -0.0).
 * Checked before any HIP call (RX_EINVAL, the message names the track and the
 * field): n_tracks <= 0, a null pointer, wp_off[0] != 0, W < 2, W above
 * 64 * RX_WP_CHUNK * RX_WP_SUPER, cull_super outside 0..64, a box count above int32. */
typedef struct rx_cull_tables {
  int32_t* chunk_off;   /* [n+1] */
  int32_t* super_off;   /* [n+1] */
  int32_t* wchunk_off;  /* [n+1] */
  int32_t* wsuper_off;  /* [n+1] */
  double* chunk_box;    /* [leaf][4] */
  double* super_box;    /* [super][4] */
  double* wchunk_box;   /* [wchunk][4] */
  double* wsuper_box;   /* [wsuper][4] */
  double* slot_geo;     /* [n][4] */
  float* chunk_box_f;   /* [5][leaf][4] */
  float* super_box_f;   /* [5][super][4] */
  float* seg_f;         /* [2*Wtot][4] */
  void* slot_hdr;       /* [n] rows of 128 bytes */
} rx_cull_tables;
int rx_cull_table_sizes(int32_t n_tracks, const int32_t* wp_off, int32_t cull_chunk, int32_t cull_super,
                        int64_t* out);
int rx_build_cull_tables_host(int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* seg,
                              const double* meta, int32_t cull_chunk, int32_t cull_super, const rx_cull_tables* out,
                              void* stream);
int rx_build_cull_tables(int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* seg,
                         const double* meta, int32_t cull_chunk, int32_t cull_super, const rx_cull_tables* out,
                         void* stream);

/* rx_upload_tracks for a table in DEVICE memory (wp_off stays a HOST array): the
 * same per-track checks, the handle copies what it keeps (device to device, into
 * buffers it reuses when they are large enough: a swap to a table of the same
 * shape keeps every address) and builds its culling tables with
 * rx_build_cull_tables' kernel; rx_assign is required again.  The only transfer to
 * the host is the [n][8] meta block, for the width and max_track_distance checks:
 * a NaN meta[k][4] (rx_build_tracks' mark of a bad track) is refused with the
 * track named.  Everything is checked before anything is written, so a refused
 * call leaves the handle stepping on its old table.  Synchronous: waits for the
 * device before it starts and for `stream` before it returns; not capturable. */
int rx_upload_tracks_device(rx_env* h, int32_t n_tracks, const int32_t* wp_off, const double* wp, const double* nrm,
                            const double* seg, const double* meta, void* stream);

/* Replacing slots in place (ABI v25, additive).  A slot's table rows, seg_f rows,
 * boxes, slot_geo row and header depend on that slot's own rows and offsets only,
 * so a new track with the SAME waypoint count as the slot it replaces can be
 * written over that slot: no offset, no box count and no address changes, and every
 * other slot stays bit for bit what it was.
 *
 * rx_track_patch: the n_upd replacement tracks as a small table of their own
 * (rx_build_tracks' layout for n_upd tracks, src_off its waypoint offsets) and the
 * slots they go to.
 *
 * rx_patch_tracks / rx_patch_tracks_host: handle-free, like rx_build_cull_tables.
 * For every j < n_upd with k = slots[j] they copy source track j's wp, nrm, seg and
 * meta rows over slot k's rows of the destination table (wp_off: the destination's
 * offsets), and, when `t` is given, rewrite slot k's seg_f rows, leaf, super, wchunk
 * and wsuper boxes (f64 and the five float blocks), slot_geo row and slot_hdr row by
 * the rules of csrc/rx_cull.h at the offsets slot k already has.  The offset arrays
 * of `t` are not written (nor read: the offsets are recomputed from wp_off, as
 * rx_build_cull_tables does).  With t == NULL only the four table arrays are
 * patched.  cull_chunk <= 0 and cull_super == 0 mean what they mean in
 * rx_build_cull_tables.  rx_patch_tracks: wp_off, slots and src_off are HOST
 * arrays, everything else DEVICE pointers; one launch (a wavefront per listed slot,
 * csrc/rx_cull.hip k_patch_slots) on `stream`, no host wait; the listed slots'
 * offsets travel through a stream-ordered allocation (not capturable).
 * rx_patch_tracks_host: every pointer a HOST pointer, no HIP call.
 *
 * The contract is bytes: after the call every destination array equals, byte for
 * byte, what rx_build_tracks(_host) plus rx_build_cull_tables(_host) write for the
 * updated pool -- host against host, device against device (device against host
 * keeps rx_build_cull_tables' hypot and signed-zero differences).  Nothing outside
 * the listed slots' spans is written.
 *
 * Checked before any HIP call or write (RX_EINVAL, the message names the slot and
 * the field): a null pointer among the ones read, n_upd outside 1..n_tracks, slots
 * not ascending and distinct or out of range, src_off[0] != 0, a source track whose
 * waypoint count differs from its slot's (a replaced slot keeps its waypoint
 * count), and what rx_build_cull_tables checks on wp_off, G and S.  The host twin
 * also refuses a source meta row with width < 0 or max_track_distance not > 0 (NaN
 * is rx_build_tracks' mark of a bad track).
 *
 * rx_replace_tracks_device: the same patch on the handle's own buffers, whichever
 * door its table came through.  The checks above against the handle's offsets;
 * then it waits for the device (launches reading the old rows may be in flight on
 * any stream), downloads the [n_upd][8] source meta block for rx_upload_tracks_device's
 * width and max_track_distance checks (the slot named), and only then launches and
 * waits for `stream`.  A refused call leaves the handle byte for byte as it was.
 * The assignment, n_tracks, the wave order, the bound state and every buffer
 * address stay; no env is reset: the caller resets the envs on the replaced slots
 * (rx_reset with a mask).  Single-agent and two-car handles, every schedule.
 * RX_ESTATE before a table has been uploaded. */
typedef struct rx_track_patch {
  int32_t n_upd;           /* slots to replace, 1..n_tracks */
  const int32_t* slots;    /* HOST [n_upd], ascending, distinct, in [0, n_tracks) */
  const int32_t* src_off;  /* HOST [n_upd + 1], src_off[0] = 0: waypoint offsets of the source table */
  const double *wp, *nrm, *seg, *meta; /* the source table: rx_build_tracks' layout for n_upd tracks */
} rx_track_patch;
int rx_patch_tracks(int32_t n_tracks, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta,
                    int32_t cull_chunk, int32_t cull_super, const rx_cull_tables* t, const rx_track_patch* p,
                    void* stream);
int rx_patch_tracks_host(int32_t n_tracks, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta,
                         int32_t cull_chunk, int32_t cull_super, const rx_cull_tables* t, const rx_track_patch* p,
                         void* stream);
int rx_replace_tracks_device(rx_env* h, const rx_track_patch* p, void* stream);

/* Fused optimizer step of PPO.ppo_update (agent/ppo.py:204-207):
 * nn.utils.clip_grad_norm_(params, max_grad_norm) then torch.optim.Adam.step()
 * (the default eps=1e-5 Adam of agent/ppo.py:83, no weight decay/amsgrad),
 * over parameters stored back to back in ONE float32 buffer: tensor k owns
 * elements [offsets[k], offsets[k+1]).  Two launches: per-slice, per-tensor
 * sums of squares into ws, then per element: global norm -> clip coefficient
 * -> Adam update.
 *
 *   step    device f32 scalar, the Adam step count (incremented here);
 *   lr      device f64 scalar (read at run time, so a captured graph follows
 *           the host-side lr anneal);
 *   stop    device bool or NULL: when *stop != 0 the launch changes nothing
 *           (the KL early stop of agent/ppo.py:178-182 without a host sync);
 *   ws      device f32 scratch of rx_adam_workspace_floats(cfg) elements
 *           (the clip-norm partials, then Adam's two step scalars),
 *           owned by the caller (one per concurrently stepping optimizer).
 * max_grad_norm <= 0 disables clipping.  Grads are scaled in place, as
 * clip_grad_norm_ does.  Equal to torch's clip + Adam within float rounding
 * (tests/test_optim_gpu.py), not bit for bit (reduction order). */
#define RX_ADAM_MAX_TENSORS 32
typedef struct rx_adam_config {
  int32_t n_tensors;
  int64_t offsets[RX_ADAM_MAX_TENSORS + 1];
  double beta1, beta2, eps, max_grad_norm;
} rx_adam_config;
#define RX_ADAM_NORM_ELEMS 64  /* gradient entries per clip-norm partial (rx_adam_workspace_floats) */
size_t rx_adam_workspace_floats(const rx_adam_config* cfg); /* 0 for an invalid cfg */
int rx_adam_clip_step(const rx_adam_config* cfg, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                      float* step, const double* lr, const uint8_t* stop, float* ws, void* stream);

/* Fused PPO minibatch gradient (agent/ppo.py:170-203) for the reference's
 * actor-critic (agent/ppo.py:11-62: Linear(D,64)-tanh-Linear(64,64)-tanh-
 * Linear(64,2)-tanh actor, same trunk with a 1-wide linear head for the
 * critic, fixed log_std buffer), parameters flat in module.parameters() order
 * (rx_adam_clip_step layout).  For minibatch m of an epoch (rows
 * perm[m*mb .. (m+1)*mb)) it computes the gradient of
 *   pg_loss - ent_coef * entropy + vf_coef * v_loss
 * (the entropy term has no parameter gradient: it depends on log_std only)
 * into grad [P], and approx_kl = mean(old_logp - new_logp); if approx_kl >
 * kl_target it sets *stop (and *kl_at_stop) so the rx_adam_clip_step that
 * follows is skipped.  With *stop already set the call does nothing.
 * fp32; equal to torch autograd within float rounding (tests/test_ppo_fused_gpu.py). */
/* Matrix-core precision of the policy kernels (rx_ppo_batch / rx_policy_io):
 * FP32 = v_mfma_f32_16x16x4_f32, exact float32 products (an fmaf chain);
 * BF16 = v_mfma_f32_16x16x32_bf16: weights / activations / gradients rounded to
 * bf16 as matrix operands, float32 accumulation, float32 everywhere else
 * (BASELINE.json configs[1], "PPO bf16").  Biases are never rounded; a bias
 * gradient is the sum of the ROUNDED operand of its layer's weight gradient
 * (db = sum over rows of bf16(dZ), through a ones column of the same MFMA).
 * DESIGN.md §4, "The bf16 contract", lists every rounded operand;
 * tests/bf16_ref.py restates them in float64. */
#define RX_PREC_FP32 0
#define RX_PREC_BF16 1
typedef struct rx_ppo_batch {
  int32_t obs_dim;          /* D: 15 (single-agent) or 19 (two-car) */
  int32_t mb;               /* minibatch rows */
  int64_t n_rows;           /* B = rows of the flattened rollout; perm entries must be < B */
  const float* obs;         /* [B][D] */
  const float* actions;     /* [B][2] */
  const float* logprobs;    /* [B] */
  const float* advantages;  /* [B] */
  const float* returns;     /* [B] */
  const float* values;      /* [B] */
  const int64_t* perm;      /* [n_mb*mb] this epoch's shuffled row indices (b_inds); an entry outside
                             * [0, n_rows) is an absent row: it adds nothing to the gradient, the KL sum
                             * or the advantage moments (the divisors stay mb) */
  const float* params;      /* [P] flat parameters */
  const float* log_std;     /* [2] Agent.log_std buffer */
  const float* adv_stats;   /* [n_mb][2] (mean, unbiased std) from rx_ppo_adv_stats */
  float clip_coef, vf_coef, kl_target;
  int32_t precision;        /* RX_PREC_FP32 (default) or RX_PREC_BF16 (ABI v14) */
} rx_ppo_batch;
/* P for obs_dim (10,563 for 15, 11,075 for 19; 0 = unsupported). */
int rx_ppo_n_params(int32_t obs_dim);
/* float / double workspace sizes rx_ppo_minibatch_grad needs for minibatch size mb. */
size_t rx_ppo_workspace_floats(int32_t obs_dim, int32_t mb);
size_t rx_ppo_workspace_doubles(int32_t mb);
/* (mean, unbiased std) of advantages[perm[m*mb ..]] for every minibatch m < n_mb. */
int rx_ppo_adv_stats(const rx_ppo_batch* b, int32_t n_mb, float* stats, void* stream);
int rx_ppo_minibatch_grad(const rx_ppo_batch* b, int32_t m, float* ws_f32, double* ws_f64, float* grad,
                          uint8_t* stop, float* kl_at_stop, void* stream);

/* One whole optimizer step of the single-rank update (agent/ppo.py:170-207:
 * minibatch forward / loss / backward, KL check, clip_grad_norm_, Adam) in
 * three launches: rx_ppo_minibatch_grad's gradient + reduce (which also writes
 * the per-tensor sums of squares to adam_ws and bumps *step unless it raises
 * *stop), then the clip + Adam update of params / exp_avg / exp_avg_sq
 * (rx_adam_clip_step's arithmetic; skipped when *stop is set).  params must be
 * b->params; cfg the rx_adam_clip_step layout of the same P parameters;
 * adam_ws holds rx_ppo_update_workspace_floats(obs_dim, cfg) floats (ABI v23: the
 * per-tensor norm partials and Adam's two step scalars; no control block). */
size_t rx_ppo_update_workspace_floats(int32_t obs_dim, const rx_adam_config* cfg);
int rx_ppo_minibatch_update(const rx_ppo_batch* b, int32_t m, const rx_adam_config* cfg, float* params,
                            float* ws_f32, double* ws_f64, float* grad, float* exp_avg, float* exp_avg_sq, float* step,
                            const double* lr, uint8_t* stop, float* kl_at_stop, float* adam_ws, void* stream);

/* Data-parallel variant of the same minibatch step (one rank's shard of a
 * global minibatch; rx.dist).  Replaces the per-rank part of
 * agent/ppo.py:170-207 when the batch is sharded over W ranks:
 *
 *   rx_ppo_adv_moments     per minibatch (sum, square-sum) of this shard's
 *                          advantages, f64 [n_mb][2] -> caller all-reduces;
 *   rx_ppo_adv_finalize    (mean, unbiased std) from all-reduced moments over
 *                          count = W*mb rows -> adv_stats of the batch
 *                          (moments -> finalize with count = mb equals
 *                          rx_ppo_adv_stats bit for bit);
 *   rx_ppo_minibatch_grad_shard
 *                          the shard's gradient times ``scale`` (= 1/W: an
 *                          all-reduce SUM then gives the global-minibatch mean
 *                          gradient) into grad, and scale * mean(old_logp -
 *                          new_logp) into *kl_out.  Reads *stop (does nothing
 *                          when set) but never writes it: with grad and kl_out
 *                          adjacent in one buffer a single all-reduce carries
 *                          both;
 *   rx_ppo_kl_check        after the all-reduce: *kl > kl_target -> *stop = 1,
 *                          *kl_at_stop = *kl (agent/ppo.py:178-182), so the
 *                          rx_adam_clip_step that follows is skipped on every
 *                          rank alike. */
int rx_ppo_adv_moments(const rx_ppo_batch* b, int32_t n_mb, double* moments, void* stream);
/* ABI v17: rx_ppo_adv_stats / rx_ppo_adv_moments spread over many workgroups
 * per minibatch (chunks of 2,048 rows, a partial-moment workspace ws of
 * rx_ppo_adv_workspace_doubles(mb, n_mb) doubles, two launches: chunk moments,
 * then a fold in chunk order).  Writes the raw (sum, square-sum) moments when
 * `moments` is given (data parallel: all-reduce, then rx_ppo_adv_finalize),
 * else (mean, unbiased std) into stats; moments -> rx_ppo_adv_finalize(count =
 * mb) equals the stats output bit for bit.  Its own summation order: not
 * bit-identical to rx_ppo_adv_stats. */
size_t rx_ppo_adv_workspace_doubles(int32_t mb, int32_t n_mb);
int rx_ppo_adv_stats_ws(const rx_ppo_batch* b, int32_t n_mb, double* ws, float* stats, double* moments, void* stream);
int rx_ppo_adv_finalize(const double* moments, int32_t n_mb, int64_t count, float* stats, void* stream);
int rx_ppo_minibatch_grad_shard(const rx_ppo_batch* b, int32_t m, float scale, float* ws_f32, double* ws_f64,
                                float* grad, float* kl_out, const uint8_t* stop, void* stream);
int rx_ppo_kl_check(const float* kl, float kl_target, uint8_t* stop, float* kl_at_stop, void* stream);

/* ABI v16.  The minibatch shuffle of PPO.ppo_update (agent/ppo.py:165-171,
 * np.random.shuffle(b_inds)) on the device, for config shuffle = "device": out
 * [n] int64 receives a pseudo-random permutation of 0 .. n-1 keyed by seed
 * (4-round unbalanced Feistel network on ceil(log2 n) bits, cycle-walked to
 * [0, n)); one launch, no host
 * round trip.  Same seed, same permutation. */
int rx_random_permutation(int64_t n, uint64_t seed, int64_t* out, void* stream);

/* Rollout policy step (agent/ppo.py:105-110: agent.get_action_and_value(obs)
 * under no_grad) for the same policy layout: per row, actor + critic forward,
 *   action = clamp(eps * exp(log_std) + mu, -1, 1)   (Normal.sample(), then
 *            the reference's clamp; eps = N(0,1) noise drawn by the caller,
 *            e.g. torch normal_(), so the sampling stream stays torch's)
 *   logprob = sum_j Normal(mu, std).log_prob(action_j);  value = critic(obs).
 * fp32; equal to the torch forward within float rounding
 * (tests/test_ppo_fused_gpu.py). */
typedef struct rx_policy_io {
  int32_t obs_dim;        /* 15 or 19 */
  int64_t n;              /* rows */
  const float* obs;       /* [n] rows of D floats, obs_stride floats apart (0 = D) */
  const float* eps;       /* [n][2] */
  const float* params;    /* flat parameters */
  const float* log_std;   /* [2] */
  float* actions;         /* [n] rows of 2 floats, act_stride floats apart (0 = 2) out */
  float* logprobs;        /* [n] out */
  float* values;          /* [n] out */
  int64_t obs_stride;     /* e.g. 2*19 for one car's rows of a two-car [n][2][19] buffer */
  int64_t act_stride;     /* e.g. 4 for one car's actions in [n][2][2] */
  int32_t precision;      /* RX_PREC_FP32 (default) or RX_PREC_BF16 (ABI v14) */
  float* actions2;        /* ABI v19: NULL, or a second copy of the actions (e.g. the agent's slot of a two-car
                             env's [n][2][2] action buffer), rows act2_stride floats apart (0 = 2) */
  int64_t act2_stride;
} rx_policy_io;
int rx_policy_act(const rx_policy_io* io, void* stream);

/* A whole rollout of few single-agent envs in ONE persistent launch.
 * Replaces PPO.collect_rollout's step loop (agent/ppo.py:97-132: per step
 * agent.get_action_and_value(next_obs) at :105-110, envs.step(action) at
 * :112-120) for handles in the small-N configuration (one env per dynamics
 * wave: rx_rollout_supported).  Per step t the env's workgroup evaluates the
 * policy on obs[t] exactly as rx_policy_act does with eps[t] (actions,
 * log-probs, values), then steps the env exactly as rx_step does, writing
 * obs[t+1] (next_obs after the last step), rewards[t], dones[t+1] (next_done
 * after the last step).  obs[0] and dones[0] are the caller's.  io supplies the
 * env's terminated / truncated / ep_done / ep_stats buffers (its obs, reward,
 * done and actions pointers are ignored).  Same stream semantics as rx_step. */
typedef struct rx_rollout_io {
  int32_t T;              /* steps */
  int32_t obs_dim;        /* 15 or 19 (= the handle's observation width) */
  const float* params;    /* flat policy parameters (rx_policy_act layout) */
  const float* log_std;   /* [2] */
  const float* eps;       /* [T][N][2] N(0,1) noise */
  float* obs;             /* [T][N][D] */
  float* actions;         /* [T][N][2] out */
  float* logprobs;        /* [T][N] out */
  float* values;          /* [T][N] out */
  float* rewards;         /* [T][N] out */
  float* dones;           /* [T][N] out (rows 1..T-1) */
  float* next_obs;        /* [N][D] out */
  float* next_done;       /* [N] out */
} rx_rollout_io;
int rx_rollout_supported(const rx_env* h);
int rx_rollout(rx_env* h, const rx_io* io, const rx_rollout_io* r, void* stream);

/* ABI v19: the same T-step rollout for ANY single-agent handle as a sequence of
 * launches enqueued by ONE call: per step t, rx_policy_act on obs[t] with
 * eps[t] (actions[t], logprobs[t], values[t]) at matrix-core `precision`, then
 * rx_step of actions[t] writing obs[t+1] (next_obs at t = T-1), rewards[t] and
 * dones[t+1] (next_done).  Every kernel and every output equals the per-step
 * Python loop (rx_policy_act + rx_step per step) with the same eps bit for bit;
 * what it removes is T x (tensor slicing + two ctypes calls + a noise launch)
 * of host time per rollout -- the eager rollout of a few thousand envs was
 * host-bound.  `io` as for rx_rollout.  Replaces the step loop of
 * PPO.collect_rollout, agent/ppo.py:97-132. */
int rx_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, int32_t precision, void* stream);

/* ABI v19: the self-play rollout (environment/wrappers.py:29-55 inside
 * agent/self_play_ppo.py's collect_rollout) of a TWO-CAR handle the same way:
 * per step t the frozen opponent's rx_policy_act on its rows of the env's obs
 * buffer (opp_eps[t], actions into its slot of the env's action buffer), the
 * agent's rx_policy_act on obs[t] (eps[t]; actions into actions[t] AND its slot
 * of the env's action buffer), rx_step, then one copy of the agent's obs row and
 * reward out of the env's [N][2] buffers into obs[t+1] / rewards[t].  Five
 * launches per step from one call (the Python step ran nine: two noise draws,
 * three copies).  Every output equals SelfPlayVectorEnv's per-step path with
 * the same noise bit for bit.  `r` is the agent's rollout (obs_dim 19). */
typedef struct rx_selfplay_io {
  const float* opp_params;   /* the frozen opponent's flat parameters */
  const float* opp_log_std;  /* [2] */
  const float* opp_eps;      /* [T][N][2] N(0,1) noise of the opponent */
  float* env_actions;        /* [N][2][2] the handle's action buffer */
  float* env_obs;            /* [N][2][D] the handle's observation buffer (rx_io.obs) */
  float* env_reward;         /* [N][2] the handle's reward buffer (rx_io.reward) */
  float* sink;               /* [2N] float32 scratch: the opponent's log-probs / values */
  int32_t agent;             /* the learning agent's car (0 or 1); the opponent is the other */
  int32_t opp_precision;     /* RX_PREC_* of the opponent's forward */
} rx_selfplay_io;
int rx_selfplay_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                              int32_t precision, void* stream);

/* ABI v25: an evaluation's step loop from one call.  Replaces the per-episode
 * loops of utils/metrics.py:39-78 (eval_single_agent) and utils/metrics.py:80-150
 * (eval_multi_agent) that evaluate.py:12-122 runs once per (track, run), for every
 * episode of the protocol at once: per step t, with no host wait in between,
 *   policy mode (params != NULL): one rx_policy_act over the N*A rows of io->obs
 *     (contiguous [N][A][D]; two cars: both driven by the same policy, as
 *     utils/metrics.py:94-101 does) with eps[t], actions into actions[t] (bf16: the
 *     operand fragments are built once per call, as rx_rollout_steps does);
 *   open loop (params == NULL): actions[t] are the caller's;
 *   rx_step of actions[t], writing io->obs in place;
 *   k_eval_acc (csrc/rx_eval.hip): for every env e with active[e], per car q,
 *     acc[e][q]: total_reward += reward64; total_distance += sqrt(dx*dx + dy*dy)
 *     against the stored previous post-step position (not on the episode's first
 *     step, utils/metrics.py:59-64); prev_x, prev_y = the position; steps += 1;
 *     progress, speed, placement = this step's info columns; flags = the car's
 *     RX_F_* byte; then active[e] = 0 if done_f32[e] != 0, and *n_active -= the
 *     envs that ended.  An env whose episode has ended is never touched again (its
 *     record keeps the terminal step's values); with *n_active == 0 the kernel
 *     returns at once.
 * The kernel reads the post-step positions and flags from the engine's working
 * state, so no rx_state_export is needed.  The record is bit-equal to the one
 * rx.evaluate's eager loop accumulates with torch from the same actions (the same
 * float64 operations in the same order: separate multiply and add, IEEE sqrt);
 * policy-mode actions are rx_policy_act's, equal to the torch forward within
 * float rounding.
 *   acc      f64 [N][A][RX_EVAL_W], env order: 0 total_reward, 1 total_distance,
 *            2 steps (per env, written to every car's record), 3 progress, 4 speed,
 *            5 placement, 6 flags, 7 prev_x, 8 prev_y, 9 zero; integers as exact
 *            doubles, so a result is one device-to-host copy;
 *   active   uint8 [N];  n_active  int32 [1].
 * Before the first call of an evaluation the caller resets the envs (rx_reset
 * into io->obs) and sets acc = 0, active = 1, *n_active = N; later calls continue
 * the same episodes.  io supplies obs, reward64, info and done_f32 (all required;
 * its actions pointer is ignored).  Any autoreset mode is accepted; an evaluation
 * uses RX_AUTORESET_DISABLED.  Same stream semantics as rx_step. */
#define RX_EVAL_W 10
typedef struct rx_eval_io {
  int32_t obs_dim;       /* the handle's D */
  int32_t precision;     /* RX_PREC_*; policy mode only */
  const float* params;   /* flat policy parameters, or NULL = open loop (actions are inputs) */
  const float* log_std;  /* [2] (policy mode) */
  const float* eps;      /* [n_steps][N*A][2] N(0,1) noise (policy mode); all zeros = deterministic mu */
  float* actions;        /* [n_steps][N][A][2]: read in open-loop mode, WRITTEN in policy mode */
  float* logp_sink;      /* [N*A] scratch (policy mode) */
  float* value_sink;     /* [N*A] scratch (policy mode) */
  double* acc;           /* [N][A][RX_EVAL_W] */
  uint8_t* active;       /* [N] */
  int32_t* n_active;     /* [1] */
} rx_eval_io;
int rx_eval_steps(rx_env* h, const rx_io* io, const rx_eval_io* ev, int32_t n_steps, void* stream);

/* ABI v25, additive: rgb_array rendering on the device.  Replaces the drawing of
 * utils/visualization.py:103-120, :218-250 (pygame) by three handle-free kernels
 * (csrc/rx_render.hip) with bit-identical host twins; the rules live in
 * csrc/rx_raster.h and DESIGN.md §4 -- this project's own exact rules, not
 * pygame's pixels, and no HUD text.
 *
 * Pixel classes of the static layer (one byte per pixel, later overwrites
 * earlier) and the bits of the trail layer: */
#define RX_PX_BACKGROUND 0  /* (50,50,50) */
#define RX_PX_TRACK 1       /* (180,180,180): even-odd fill of track_polygon */
#define RX_PX_BORDER 2      /* (0,0,0): both boundary loops, closed, width 4 */
#define RX_PX_START 3       /* (0,255,0): the start line, width 5 */
#define RX_PX_TRAIL0 0x10   /* (255,100,100): car 0's path, width 3 */
#define RX_PX_TRAIL1 0x20   /* (100,100,255): car 1's path, drawn over car 0's */
#define RX_RASTER_SIZE_MIN 16
#define RX_RASTER_SIZE_MAX 2048
#define RX_RASTER_MAX_IMAGES 65535 /* K and n_layers: one grid dimension */
/* rx_raster_static: the static layers of n tracks, once per track.
 *   edge_off int32 [n+1]: layer k owns edges [edge_off[k], edge_off[k+1]);
 *   edges    int32 [n_edges][6]: ax, ay, bx, by in integer screen coordinates
 *            (rx.render.track_view), class 1..7, width.  width 0: an edge of the
 *            polygon filled with `class` by the even-odd rule; width > 0: a thick
 *            line of `class`.  A pixel gets the highest class that covers it;
 *   layer    uint8 [n][size][size], written in full.
 * k_raster_static: a 16x16 pixel tile per block, the edges staged through LDS
 * 256 at a time, each tested against the tile first (a conservative test: the
 * layer is the same with and without it).
 *
 * rx_raster_io: K images of `size` x `size` pixels.  Image k shows env
 * env_ids[k]; the poses are the env-order state arrays rx_state_export fills
 * (element e*A+q of x, y, angle), so no handle is needed.
 *   view     f64 [K][3]: scale, offset_x, offset_y of setup_track_visualization;
 *   layer_of int32 [K]: the static layer of image k;
 *   trail    uint8 [K][size][size]; last int32 [K][A][3] = (x, y, valid), the
 *            last path point of each car.  Zero both to begin an episode;
 *   out      image k's pixel (row j, column i) is the 3 bytes R, G, B at
 *            out + out_off[k] + j*out_pitch + 3*i, so K images compose straight
 *            into one mosaic; out_size is the byte size of the buffer behind
 *            `out`, and an image that would not fit in it is not written.
 * An env id outside [0, n_envs) or a layer outside [0, n_layers) leaves the
 * image's cars / the image alone.  A car with a non-finite pose is not drawn and
 * adds no path point for that call.
 *
 * rx_raster_trail (after each step; reads env_ids, x, y, view, trail, last): per
 * car, convert_coords of (x, y); if the car has a last point, the capsule of
 * width 3 from it to the new point is OR-ed into trail with the car's bit; the
 * point becomes the last one.  One block per image, car 0 then car 1.
 * rx_raster_frame (reads everything but last): the colour of every pixel from
 * the static class, the trail bits and the up-to-two car quads (fill, then
 * outline of width 2; car 1 over car 0).  Each lane owns 4 consecutive pixels of
 * a row and stores 12 bytes, as three dwords when the image's rows start on
 * 4-byte boundaries (out + out_off[k] and out_pitch both multiples of 4) and
 * by bytes otherwise: a [K][size][size][3] stack with size % 4 == 0 takes the
 * fast path, a mosaic only when its padding keeps the rows aligned.
 *
 * All pointers are DEVICE pointers; the *_host twins take the same arguments as
 * HOST pointers, ignore `stream`, make no HIP call and give the same bytes.
 * Checked before any launch (RX_EINVAL, the message names the field): null
 * pointers, size outside 16..2048, A not 1 or 2, K <= 0 or above 65535, n_envs
 * or n_layers <= 0, out_pitch negative or below 3*size, out_size < 0; for
 * rx_raster_static n outside 1..65535 and n_edges < 0.  The launches are
 * enqueued on `stream` and no call waits. */
typedef struct rx_raster_io {
  int32_t K, A, size, n_envs, n_layers, reserved0;
  const int32_t* env_ids;  /* [K] */
  const double* x;         /* [n_envs*A] */
  const double* y;
  const double* angle;
  const double* view;      /* [K][3] */
  const int32_t* layer_of; /* [K] */
  const uint8_t* layer;    /* [n_layers][size][size] */
  uint8_t* trail;          /* [K][size][size] */
  int32_t* last;           /* [K][A][3] */
  uint8_t* out;
  const int64_t* out_off;  /* [K] */
  int64_t out_pitch;
  int64_t out_size;
} rx_raster_io;
int rx_raster_static(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                     uint8_t* layer, void* stream);
int rx_raster_static_host(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                          uint8_t* layer, void* stream);
int rx_raster_trail(const rx_raster_io* r, void* stream);
int rx_raster_trail_host(const rx_raster_io* r, void* stream);
int rx_raster_frame(const rx_raster_io* r, void* stream);
int rx_raster_frame_host(const rx_raster_io* r, void* stream);

/* ABI v25, additive: league play -- a policy forward in which every row picks
 * its weights from a BANK of policies, and the two-car match loop built on it
 * (rx.league: which of two self-play snapshots is the better racer; the
 * reference compares models by solo metrics only, evaluate.py:68-122).
 *
 * rx_policy_act_bank: rx_policy_act with per-row parameters.  Row r is evaluated
 * with policy p = policy_of_row[r]: parameters io.params + p * params_stride (the
 * flat rx_policy_act layout), log-std io.log_std + 2 p, noise io.eps[r]; every
 * output of row r (action, log-prob, value, the optional actions2 copy) equals bit
 * for bit what rx_policy_act writes for that row when launched with policy p
 * alone and the same eps, in both precisions (k_policy_act_bank, csrc/rx_ppo.hip:
 * a batch row is one MFMA column, so a 16-row tile is evaluated once per distinct
 * policy present in it and only that policy's rows store; a tile whose rows share
 * one policy costs what rx_policy_act's tile costs).
 *   tile_cars 1: a tile is rows 16 b .. 16 b + 15.
 *   tile_cars 2: the rows are [n / 2][2] (env, car), n even; a tile is car q of 16
 *     consecutive envs, so it holds one policy whenever those envs share a seating
 *     (interleaved tiles would hold two every time).  Which tile a row falls in
 *     never changes what is written for it.
 * policy_of_row lives in device memory, so it cannot be checked here: every entry
 * must lie in [0, n_policies).  A row whose entry is outside that range is
 * skipped: nothing is read and nothing is written for it.
 * Any params_stride >= rx_ppo_n_params(obs_dim) is accepted; rx.league pads it to a
 * multiple of 64 floats, so every policy starts on a 256-byte boundary as a
 * separately allocated one does.
 * Checked before any HIP call (RX_EINVAL, the message names the field): null io,
 * obs_dim not 15 or 19, n <= 0, n_policies <= 0, params_stride <
 * rx_ppo_n_params(obs_dim), precision, tile_cars not 1 or 2 (or n odd with 2),
 * row strides that overlap, null buffers. */
typedef struct rx_policy_bank_io {
  rx_policy_io io;               /* params / log_std: the bank bases [n_policies][params_stride] / [n_policies][2] */
  int32_t n_policies;
  int32_t tile_cars;             /* 1 or 2 (above) */
  int64_t params_stride;         /* floats between two policies' parameters, >= rx_ppo_n_params(obs_dim) */
  const int32_t* policy_of_row;  /* [n], device memory */
} rx_policy_bank_io;
int rx_policy_act_bank(const rx_policy_bank_io* b, void* stream);

/* rx_match_steps: rx_eval_steps' policy mode with a seating.  Per step t: ONE
 * rx_policy_act_bank launch over the N*A rows of io->obs (tile_cars = A) with
 * eps[t], car q of env e driven by policy seat[e][q], actions into actions[t];
 * rx_step of actions[t]; k_eval_acc.  Everything else is rx_eval_steps': the
 * record layout, the caller's duties before the first call, io->obs written in
 * place, active / n_active, any autoreset mode, the stream semantics.  A == 1 (any
 * bank member per env) and A == 2 are accepted.  There is no open-loop mode
 * (rx_eval_steps has one).  seat entries must lie in [0, n_policies): a car with
 * an entry outside gets no action written (rx_policy_act_bank's skip rule). */
typedef struct rx_match_io {
  int32_t obs_dim;       /* the handle's D: 15 or 19 */
  int32_t precision;     /* RX_PREC_* */
  const float* params;   /* bank base [n_policies][params_stride] */
  const float* log_std;  /* [n_policies][2] */
  const float* eps;      /* [n_steps][N*A][2] N(0,1) noise; all zeros = deterministic mu */
  float* actions;        /* [n_steps][N][A][2] out */
  float* logp_sink;      /* [N*A] scratch */
  float* value_sink;     /* [N*A] scratch */
  double* acc;           /* [N][A][RX_EVAL_W] */
  uint8_t* active;       /* [N] */
  int32_t* n_active;     /* [1] */
  int32_t n_policies;
  int32_t reserved0;
  int64_t params_stride; /* floats, >= rx_ppo_n_params(obs_dim) */
  const int32_t* seat;   /* [N][A] device memory: the policy driving car q of env e, env order */
} rx_match_io;
int rx_match_steps(rx_env* h, const rx_io* io, const rx_match_io* m, int32_t n_steps, void* stream);

/* ABI v25, additive: league TRAINING -- every env of a self-play rollout races
 * its own opponent from a bank of frozen snapshots, drawn and tallied on the
 * device (agent/self_play_ppo.py:40-50 draws ONE opponent per update on the host;
 * rx.league_train).  The arithmetic lives in csrc/rx_league.h, shared by the
 * kernels (csrc/rx_league.hip) and the *_host twins; DESIGN.md §4.
 *
 * Slots 0 .. n_live - 1 of the bank are live.  tally[k] = (games, learner wins,
 * opponent wins) against slot k.
 *
 * rx_league_weights: tallies -> sampling table (one wave, a lane per slot; all
 * float64, every operation separately rounded, sums in slot order):
 *   p_k    = (w + 0.5 * (g - w - l) + prior) / (g + 2 * prior)
 *   f_k    = (1 - p_k) multiplied `power` times into 1.0     (power 0: uniform)
 *   F      = f_0 + f_1 + ...;  prob_k = (1 - mix) * (f_k / F) + mix / n_live
 *            (F == 0: prob_k = 1 / n_live)
 *   cdf_k  = cdf_{k-1} + prob_k;  cdf_k = 1.0 for n_live - 1 <= k < n_slots.
 *
 * rx_league_draw over n envs.  With `done` (float [n]): every env e with
 * done[e] != 0 is first tallied with k = opp_id[e] from the RX_INFO_PLACEMENT
 * column of `info` (f64 [n][2][RX_INFO_W], the terminal step's rx_io.info):
 * tally[k][0] += 1, tally[k][1] += (car `agent`'s placement == 1), tally[k][2] +=
 * (the other car's placement == 1), as int64 atomic adds (a k outside
 * [0, n_slots) is not counted), and then redrawn; every other env is left alone.
 * With done == NULL every env is redrawn and nothing is tallied (info is unused).
 * The draw:
 *   h = splitmix64(seed ^ splitmix64(((uint64)draw_count[e] << 32) ^ (uint64)e))
 *   u = (double)(h >> 11) * 2^-53;  opp_id[e] = the smallest k with u < cdf_k
 *   draw_count[e] += 1
 * cdf is 1.0 from n_live - 1 on, so an id is always a live slot and the draw needs
 * no n_live: a captured graph stays valid while the pool fills.
 *
 * All pointers are DEVICE pointers; the *_host twins take the same arguments as
 * HOST pointers, ignore `stream`, make no HIP call and give the same bits.
 *
 * rx_league_rollout_steps: rx_selfplay_rollout_steps' contract and outputs with a
 * per-env opponent (sp->opp_params, opp_log_std and opp_precision are ignored):
 * per step t ONE policy launch (k_league_act, csrc/rx_ppo.hip: the learner's actor
 * and critic as in k_selfplay_act, the opponent's actor through the bank forward
 * with env e on member opp_id[e]), rx_step, then rx_league_draw's tally and redraw
 * of that step's done row and io->info, so step t + 1 sees the new ids: done by
 * step t + 1's opponent waves before they read the ids, and by one launch after
 * the last step.  io->info is required (io->reward64 is not read).
 * With every id = k the outputs equal rx_selfplay_rollout_steps' with bank member
 * k as the opponent bit for bit.
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): null
 * pointers, n_slots outside 1..64, n_live outside 1..n_slots, power outside 0..4,
 * mix outside [0, 1] or NaN, prior <= 0 or NaN, agent not 0 or 1, n <= 0, the
 * precisions, params_stride < rx_ppo_n_params(19), a handle that is not an
 * assigned, bound two-car handle with obs_dim 19. */
typedef struct rx_league_io {
  int32_t n_slots;        /* bank capacity, 1..64 */
  int32_t agent;          /* the learner's car, 0 or 1 */
  const float* params;    /* bank [n_slots][params_stride], rx_policy_act layout (rollout only) */
  const float* log_std;   /* [n_slots][2] (rollout only) */
  int64_t params_stride;  /* floats, >= rx_ppo_n_params(19) (rollout only) */
  int32_t* opp_id;        /* [N] */
  int32_t* draw_count;    /* [N] */
  int64_t* tally;         /* [n_slots][3] */
  double* cdf;            /* [n_slots] */
  uint64_t seed;
  int32_t opp_precision;  /* RX_PREC_* of the opponents' forward (rollout only) */
} rx_league_io;
int rx_league_weights(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior, void* stream);
int rx_league_weights_host(const rx_league_io* lg, int32_t n_live, int32_t power, double mix, double prior,
                           void* stream);
int rx_league_draw(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* stream);
int rx_league_draw_host(const rx_league_io* lg, int64_t n, const float* done, const double* info, void* stream);
int rx_league_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                            const rx_league_io* lg, int32_t precision, void* stream);

/* ABI v25, additive: the TRACK CURRICULUM -- every finished episode of a
 * single-agent rollout is tallied against its track slot on the device, and the
 * envs are redrawn over the slots weighted towards the tracks the learner still
 * fails (a pool-level prioritised level replay; train.py:78,94-99 draws the pool
 * once and every env keeps its track; rx.curriculum).  The arithmetic lives in
 * csrc/rx_curriculum.h, shared by the kernels (csrc/rx_curriculum.hip) and the
 * *_host twins; DESIGN.md §4.
 *
 * tally[k] = (episodes, finishes, crashes, progress_q) of slot k, int64.
 *
 * rx_track_tally over n envs: every env e with done[e] != 0 (float [n]) and
 * 0 <= track[e] < n_tracks adds to row track[e]: episodes += 1; finishes += (info
 * [e][RX_INFO_PROGRESS] == 1.0, which the env reports for a finished lap only,
 * racing_env.py:158-159); crashes += (terminated[e] != 0 and not finished);
 * progress_q += (int64)(progress * 1048576.0).  `info` is f64 [n][RX_INFO_W], the
 * terminal step's rx_io.info of a single-agent handle.  A slot outside the table is
 * not counted.  A wave whose envs are all running returns after one ballot; the
 * envs that ended are summed per slot inside the wave, and one lane per slot
 * issues the int64 atomic adds: integer sums, so the result does not depend on the
 * order of arrival.  cdf, p, track_of_env and seed are not read.
 *
 * rx_track_scores: tallies -> p and the integer sampling table (one workgroup
 * walks the table in chunks; float64, every operation separately rounded):
 *   p_k   = (finishes + prior) / (episodes + 2 * prior)        (unseen slot: 0.5)
 *   q_k   = 1 - p_k (score 0, "fail")  or  4 * p_k * (1 - p_k) (score 1, "potential")
 *   f_k   = q_k multiplied `power` times into 1.0               (power 0: uniform)
 *   W_k   = (uint64)(f_k * 4294967296.0)
 *   cdf_k = W_0 + ... + W_k, an exact integer (non-negative int64);  F = cdf_{n-1}.
 * track and track_of_env are not read.
 *
 * rx_track_draw: track_of_env[e] for e < n at `generation` g:
 *   h1 = splitmix64(seed ^ splitmix64(((uint64)g << 32) ^ (uint64)e));  h2 = splitmix64(h1)
 *   u  = (double)(h1 >> 11) * 2^-53
 *   F == 0 or u < mix:  slot = mulhi64(h2, n_tracks)           (the uniform part)
 *   otherwise:          r = mulhi64(h2, F);  slot = the smallest k with r < cdf_k
 * (binary search), so a slot with W_k == 0 is drawn by the uniform part only.
 * track, tally and p are not read.
 *
 * All pointers are DEVICE pointers; the *_host twins take the same arguments as
 * HOST pointers, ignore `stream`, make no HIP call and give the same bits.
 *
 * rx_track_rollout_steps: rx_rollout_steps' contract and outputs bit for bit, plus
 * after every step's launches ONE rx_track_tally of that step's done row,
 * io->terminated and io->info (both required), ordered after the step on `stream`.
 * No host wait and no allocation: a stream capture records it.
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): null
 * pointers, n_tracks <= 0, score not 0 or 1, power outside 0..4, prior <= 0 or
 * NaN, mix outside [0, 1] or NaN, n <= 0, the precision, a handle that is not an
 * assigned, bound single-agent handle. */
typedef struct rx_track_io {
  int32_t n_tracks;        /* track slots, > 0 */
  int32_t score;           /* 0 = fail, 1 = potential (scores only); rx_track_duel_scores: also 2 = lose, 3 = contested */
  const int32_t* track;    /* [N] the slot of env e, env order: rx_state.track (tally only) */
  int64_t* tally;          /* [n_tracks][4] */
  int64_t* cdf;            /* [n_tracks] */
  double* p;               /* [n_tracks] p_k (scores only) */
  int32_t* track_of_env;   /* [N] out (draw only) */
  uint64_t seed;
} rx_track_io;
int rx_track_tally(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated, const double* info,
                   void* stream);
int rx_track_tally_host(const rx_track_io* tc, int64_t n, const float* done, const uint8_t* terminated,
                        const double* info, void* stream);
int rx_track_scores(const rx_track_io* tc, int32_t power, double prior, void* stream);
int rx_track_scores_host(const rx_track_io* tc, int32_t power, double prior, void* stream);
int rx_track_draw(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* stream);
int rx_track_draw_host(const rx_track_io* tc, int64_t n, uint32_t generation, double mix, void* stream);
int rx_track_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                           int32_t precision, void* stream);

/* ABI v25, additive: the TRACK CURRICULUM FOR SELF-PLAY -- the per-slot tallies of
 * TWO-CAR episodes, so a self-play or league run can answer "on which tracks does the
 * learner lose" and be redrawn over its slots (rx.track_selfplay).  rx_track_io and its
 * entry points above are unchanged; the two-car columns live in rx_track_duel_io.  The
 * arithmetic is csrc/rx_track_duel.h, shared by the kernels (csrc/rx_curriculum.hip)
 * and the *_host twins; DESIGN.md §4.
 *
 * rx_track_tally2 over n two-car envs: a = td->agent is the learner's car, o = 1 - a;
 * `info` is f64 [n][2][RX_INFO_W], the terminal step's rx_io.info.  Every env e with
 * done[e] != 0 and 0 <= track[e] < n_tracks is tallied (an env outside that range is
 * not counted), with pa = info[e][a][RX_INFO_PROGRESS], po = info[e][o][RX_INFO_PROGRESS]
 * and la = info[e][a][RX_INFO_PLACEMENT]:
 *   tally[track[e]] (rx_track_io.tally, the single-agent columns for the learner's car):
 *     episodes += 1;  finishes += (pa == 1.0);
 *     crashes += (terminated[e] != 0 and pa != 1.0 and po != 1.0): both cars left the
 *       track, the only way a two-car episode terminates without a finish (a lost race
 *       is not a crash);
 *     progress_q += (int64)(pa * 1048576.0)
 *   duel[track[e]], int64 [n_tracks][RX_TRACK_DUEL_W = 4]:
 *     wins += (la == 1.0);  opp_finishes += (po == 1.0);
 *     opp_progress_q += (int64)(po * 1048576.0);  timeouts += (terminated[e] == 0)
 * Placement 1 is always awarded when an episode ends, so losses = episodes - wins and
 * are not stored.  The kernel is rx_track_tally's: a wave whose envs all run leaves
 * after one ballot, the envs that ended are folded per slot inside the wave and one lane
 * per slot issues at most 8 int64 atomic adds; integer sums, any order of arrival.
 *
 * rx_track_duel_scores: rx_track_scores with rx_track_io.score in 0..3 (rx_track_scores
 * itself keeps accepting 0 and 1):
 *   0 "fail", 1 "potential":  rx_track_scores' arithmetic on (episodes, finishes), the same bits
 *   2 "lose":       p_k = (wins + prior) / (episodes + 2 * prior);  q_k = 1 - p_k
 *   3 "contested":  the same p_k;  q_k = 4 * p_k * (1 - p_k)
 * f_k, W_k and the exact integer cdf as in rx_track_scores; p[k] receives the p_k used.
 * rx_track_draw reads cdf only and serves these tables unchanged.
 *
 * rx_track_duel_rollout_steps: with lg == NULL rx_selfplay_rollout_steps' contract and
 * outputs bit for bit; with lg rx_league_rollout_steps', opp_id, draw_count and the
 * league tally included (the fold of the league draw into the next policy launch stays).
 * In both cases ONE rx_track_tally2 follows every step's rx_step on `stream`, before the
 * next step's policy launch, reading that step's done row, io->terminated and io->info
 * (both required, also with lg == NULL).  No host wait and no allocation: a stream
 * capture records it.
 *
 * All pointers are DEVICE pointers; the *_host twins take HOST pointers, ignore `stream`,
 * make no HIP call and give the same bits.  Checked before any HIP call (RX_EINVAL, the
 * message names the field): null pointers, n_tracks <= 0, score outside 0..3 (scores),
 * agent not 0 or 1, n <= 0, power, prior and precision as above, a handle that is not an
 * assigned, bound two-car handle with obs_dim 19, td->agent != sp->agent, lg->agent !=
 * td->agent. */
#define RX_TRACK_DUEL_W 4
typedef struct rx_track_duel_io {
  int32_t agent;  /* the learner's car, 0 or 1 */
  int64_t* duel;  /* [n_tracks][RX_TRACK_DUEL_W]: wins, opp_finishes, opp_progress_q, timeouts */
} rx_track_duel_io;
int rx_track_tally2(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                    const uint8_t* terminated, const double* info, void* stream);
int rx_track_tally2_host(const rx_track_io* tc, const rx_track_duel_io* td, int64_t n, const float* done,
                         const uint8_t* terminated, const double* info, void* stream);
int rx_track_duel_scores(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                         void* stream);
int rx_track_duel_scores_host(const rx_track_io* tc, const rx_track_duel_io* td, int32_t power, double prior,
                              void* stream);
int rx_track_duel_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_selfplay_io* sp,
                                const rx_league_io* lg, const rx_track_io* tc, const rx_track_duel_io* td,
                                int32_t precision, void* stream);

/* ABI v25, additive: EPISODIC TRACK DRAWS -- an env takes a new track slot when its own
 * episode ends, as prioritised level replay does, instead of every env being reset at a
 * pool-level redraw (rx.track_episodic).  No episode is dropped and no env is reset by
 * the curriculum.  For handles on the lane-varying schedule (rx_config.lane_tracks) with
 * next-step autoreset: their wave order does not depend on the assignment and the kernels
 * read an env's slot from one array, so rewriting that entry between the terminal step and
 * the step that resets the env moves the env to another track.  The step, ray and policy
 * kernels are the ones every other rollout runs.
 *
 * rx_track_episode over n envs: rx_track_tally, and every env it tallies (done[e] != 0,
 * 0 <= track[e] < n_tracks) then draws its next slot, in this order:
 *   tally row track[e] (rx_track_tally's rule);
 *   g = draws[e];  k' = rx_track_draw's slot of env e at generation g under
 *   seed ^ RX_TRACK_EPISODE_SALT (csrc/rx_curriculum.h: the keys (draws[e], e) stay apart
 *   from rx_track_draw's (generation, e));  draws[e] = g + 1;  track[e] = k';
 *   pos_slot[env_pos[e]] = k' when the two arrays are given (an env_pos outside [0, n)
 *   is not written).
 * slot_out[e], when given, receives the slot env e was on during this step, for every
 * e < n, ended or not.  An env whose slot lies outside the table is neither tallied nor
 * redrawn.  rx_track_io.track is WRITTEN here (and only here): it must be writable device
 * memory although the field is declared const.  cdf is read as it stands (rx_track_scores
 * fills it); p and track_of_env are not read.  The draw counters live in device memory,
 * so a captured graph keeps advancing them on replay.  rx_track_episode_host: the same
 * arguments as host pointers, no HIP call, the same bits.
 *
 * rx_track_episode_step: rx_track_episode on the handle's own wave-order arrays (the
 * caller's env_pos / pos_slot are ignored) and the rows of `io` (terminated, info; `done`
 * NULL = io->done_f32), after a step the caller enqueued on `stream`: eager loops and tests.
 * rx_track_episodic_rollout_steps: rx_track_rollout_steps with rx_track_episode in the
 * place of rx_track_tally: one launch per step, no host wait and no allocation; with
 * `slots` (device int32 [T][N]) row t is step t's slot_out (ep->slot_out is ignored).
 * In both, tc->track must be the handle's bound rx_state.track.
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): everything
 * rx_track_tally and rx_track_draw check, null draws, exactly one of env_pos / pos_slot,
 * a handle that is not an assigned, bound single-agent handle, a handle whose schedule is
 * not lane-varying (set rx_config.lane_tracks = 1; that needs one lane per env, which
 * handles of at most 2,048 envs take only with dyn_lpe = 1), an autoreset mode other than
 * RX_AUTORESET_NEXT_STEP (same-step autoreset resets inside the step on the old slot;
 * without autoreset nothing resets the env). */
typedef struct rx_track_episode_io {
  uint32_t* draws;        /* [N] draws taken so far by env e (zero-filled by the caller) */
  const int32_t* env_pos; /* [N] position of env e in the wave order, or NULL */
  int32_t* pos_slot;      /* [N] slot at each position, or NULL (both or neither) */
  int32_t* slot_out;      /* [N] out, or NULL: the slot of env e during this step */
  double mix;             /* rx_track_draw's mix, in [0, 1] */
} rx_track_episode_io;
int rx_track_episode(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                     const uint8_t* terminated, const double* info, void* stream);
int rx_track_episode_host(const rx_track_io* tc, const rx_track_episode_io* ep, int64_t n, const float* done,
                          const uint8_t* terminated, const double* info, void* stream);
int rx_track_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_episode_io* ep, const rx_io* io,
                          const float* done, void* stream);
int rx_track_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                    const rx_track_episode_io* ep, int32_t* slots, int32_t precision, void* stream);

/* ABI v25, additive: the track curriculum's REPLAY SCORES -- the learning-potential
 * score, rank prioritisation and staleness of prioritised level replay (Jiang et
 * al. 2021) over the track slots, from the advantages of the rollout just
 * collected (rx.track_replay).  rx_track_io and its entry points above are
 * untouched; this block stands beside them.  The arithmetic lives in
 * csrc/rx_track_replay.h, shared by the kernels (csrc/rx_track_replay.hip) and the
 * *_host twins; DESIGN.md §4.  Floating point is float64, every operation
 * separately rounded; every sum is an integer.
 *
 * learn[k] = (samples, mag_q) of slot k, int64.
 *
 * rx_track_learn_tally over adv, f32 [T][n]: every a = adv[t][e] that is finite, of
 * an env with 0 <= track[e] < n_tracks, adds to row track[e]: samples += 1;
 * mag_q += (int64)((double)m * 1048576.0) with m = |a| (kind 0, the L1 value loss)
 * or max(a, 0) (kind 1, the positive value loss), at most 1048576.0f.  Non-finite
 * values and slots outside the table add nothing.  A lane per env column sums a
 * chunk of rows in registers, the wave folds its lanes per slot, and one lane per
 * slot issues the two int64 atomic adds: integer sums, so the result does not
 * depend on the grid or on the order of arrival.  Only track and learn are read.
 *
 * rx_track_learn_fold(update u, alpha), per slot with samples > 0:
 *   mean  = ((double)mag_q / 1048576.0) / (double)samples
 *   score = seen < 0 ? mean : score + alpha * (mean - score);  seen = u;  learn row = 0
 * Slots without samples are untouched.  Reads and writes learn, score, seen.
 *
 * rx_track_learn_tables(power, now): the rank, then the two integer tables.
 *   key_k  = seen_k < 0 ? +inf : score_k        (a score is never negative)
 *   rank_k = 1 + #{ j : key_j > key_k or (key_j == key_k and j < k) }   (1-based)
 *   h = 1.0 / (double)rank_k;  f = h multiplied `power` times into 1.0   (beta = 1 / power)
 *   W_k = (uint64)(f * 4294967296.0);  cdf_score_k = W_0 + ... + W_k   (exact)
 *   S_k = seen_k < 0 ? 0 : max(now - seen_k, 0);  cdf_stale_k = S_0 + ... + S_k
 * Reads score and seen, writes rank, cdf_score, cdf_stale.  F_stale may be 0.
 *
 * rx_track_learn_draw: track_of_env[e] for e < n at `generation` g, with h1, h2 and
 * u of rx_track_draw:
 *   u < mix:                              slot = mulhi64(h2, n_tracks)
 *   u < mix + stale_mix and F_stale > 0:  r = mulhi64(h2, F_stale), the smallest k with r < cdf_stale_k
 *   otherwise:                            rx_track_draw's search of cdf_score (uniform when F == 0)
 * With stale_mix == 0 it is rx_track_draw on cdf_score bit for bit (cdf_stale may
 * then be null).
 *
 * All pointers are DEVICE pointers; the *_host twins take the same arguments as
 * HOST pointers, ignore `stream`, make no HIP call and give the same bits.  No
 * host wait and no allocation: a stream capture records every one of them.
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): null
 * pointers among the ones the entry point reads, n_tracks <= 0, T <= 0, n <= 0,
 * kind not 0 or 1, alpha outside (0, 1] or NaN, power outside 0..10, now < 0,
 * mix or stale_mix outside [0, 1] or NaN, mix + stale_mix > 1. */
typedef struct rx_track_learn_io {
  int32_t n_tracks;        /* track slots, > 0 */
  int32_t kind;            /* 0 = |A|, 1 = max(A, 0) (tally only) */
  const int32_t* track;    /* [N] the slot of env e, env order: rx_state.track (tally only) */
  int64_t* learn;          /* [n_tracks][2] = (samples, mag_q) */
  double* score;           /* [n_tracks] */
  int32_t* seen;           /* [n_tracks] update index of the last fold with samples; -1 = never */
  int32_t* rank;           /* [n_tracks] 1-based */
  int64_t* cdf_score;      /* [n_tracks] */
  int64_t* cdf_stale;      /* [n_tracks] */
  int32_t* track_of_env;   /* [N] out (draw only) */
  uint64_t seed;
} rx_track_learn_io;
int rx_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* stream);
int rx_track_learn_tally_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv, void* stream);
int rx_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha, void* stream);
int rx_track_learn_fold_host(const rx_track_learn_io* lt, int32_t update, double alpha, void* stream);
int rx_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now, void* stream);
int rx_track_learn_tables_host(const rx_track_learn_io* lt, int32_t power, int32_t now, void* stream);
int rx_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix, double stale_mix,
                        void* stream);
int rx_track_learn_draw_host(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                             double stale_mix, void* stream);

/* ABI v25, additive: the REPLAY SCORES ON EPISODIC DRAWS -- prioritised level replay per
 * episode: an env whose episode ends draws its next slot from the score / staleness /
 * uniform mix, and the advantages are tallied by the slot every step ran on
 * (rx.track_replay_episodic).  The two blocks above are untouched.
 *
 * rx_track_learn_tally_slots over adv f32 [T][n], slots int32 [T][n] and dones f32 [T][n]
 * (or NULL): element (t, e) is counted iff adv[t][e] is finite, 0 <= slots[t][e] <
 * n_tracks, and dones is NULL or dones[t][e] == 0; a counted element adds samples += 1,
 * mag_q += q (rx_track_learn_tally's q and kind) to row slots[t][e] of learn.  A rollout
 * row entered with dones[t][e] != 0 is the autoreset step (next-step autoreset): its
 * observation is the old track's terminal one, its action is ignored, its successor is the
 * new track's first observation and the recorded slot is already the new one, so its
 * advantage belongs to neither slot.  Integer sums: the result does not depend on the grid,
 * the chunking or the order of arrival and equals the serial host loop bit for bit; with
 * slots[t][e] == track[e] for every t and dones NULL it is rx_track_learn_tally's.  Only
 * n_tracks, kind and learn of the io are read (track may be NULL).
 *
 * rx_track_learn_episode: rx_track_episode with the next slot drawn from the replay tables:
 *   k' = rx_track_learn_draw's slot of env e at generation g = draws[e] under
 *   lt->seed ^ RX_TRACK_EPISODE_SALT, with ep->mix and stale_mix.
 * The tally into tc->tally, slot_out (written before the draw), draws, track and pos_slot are
 * rx_track_episode's; a slot outside the table is neither tallied nor redrawn.  tc supplies
 * n_tracks, track and tally (cdf and p are not read); lt supplies cdf_score, cdf_stale
 * (may be NULL when stale_mix == 0) and seed.  With lt->cdf_score == tc->cdf, lt->seed ==
 * tc->seed and stale_mix == 0 every output equals rx_track_episode's bit for bit.
 * rx_track_learn_episode_step and rx_track_learn_episodic_rollout_steps are the
 * counterparts of rx_track_episode_step and rx_track_episodic_rollout_steps (the same
 * handle rules, the same launches but for the draw's kernel).
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): what
 * rx_track_learn_tally checks but for track, null slots; everything rx_track_episode checks
 * but for tc->cdf, lt->n_tracks != tc->n_tracks, null cdf_score, stale_mix or mix +
 * stale_mix outside [0, 1] or NaN, null cdf_stale with stale_mix > 0; the handle rules of
 * rx_track_episode_step. */
int rx_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                               const int32_t* slots, const float* dones, void* stream);
int rx_track_learn_tally_slots_host(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                    const int32_t* slots, const float* dones, void* stream);
int rx_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                           double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                           const double* info, void* stream);
int rx_track_learn_episode_host(const rx_track_io* tc, const rx_track_learn_io* lt, const rx_track_episode_io* ep,
                                double stale_mix, int64_t n, const float* done, const uint8_t* terminated,
                                const double* info, void* stream);
int rx_track_learn_episode_step(rx_env* h, const rx_track_io* tc, const rx_track_learn_io* lt,
                                const rx_track_episode_io* ep, double stale_mix, const rx_io* io, const float* done,
                                void* stream);
int rx_track_learn_episodic_rollout_steps(rx_env* h, const rx_io* io, const rx_rollout_io* r, const rx_track_io* tc,
                                          const rx_track_learn_io* lt, const rx_track_episode_io* ep, double stale_mix,
                                          int32_t* slots, int32_t precision, void* stream);

/* ABI v25, additive: TRACK EVOLUTION -- what fills the track slots the curriculum
 * retires, written by a kernel into a device-resident control-point buffer
 * (rx.track_evolve): a fresh track of the host generator's distribution, or a small
 * edit of a track the replay scores still rank high (ACCEL, Parker-Holder et al.
 * 2022).  Handle-free, as rx_build_tracks, which takes the new buffer as it is.  The
 * arithmetic lives in csrc/rx_track_evolve.h, shared by the kernels
 * (csrc/rx_track_evolve.hip) and the *_host twins; the rules are written out there
 * and in DESIGN.md §4.  Floating point is float64, every operation separately
 * rounded; the only transcendental is rx_sincos.
 *
 * The hash stream of spawned slot k at `generation` g is
 *   h0 = splitmix64(seed ^ splitmix64(((uint64)g << 32) ^ k)),  h_{i+1} = splitmix64(h_i)
 * and its first draw decides the kind: an EDIT (1) when u < edit_frac and
 * cdf_score[n_tracks - 1] > 0, else FRESH (0).
 *
 * rx_track_evolve_plan(generation, edit_frac): for j < n_spawn,
 *   plan[j] = (kind, parent or -1, P, 0)
 * with parent drawn from cdf_score (rx_track_learn_tables' table as it stands) and P
 * the parent's point count, or the 10..14 a fresh track draws.  Reads slots, cp_off,
 * cdf_score; writes plan.  The caller downloads the plan (16 bytes per spawned slot)
 * and forms the new offsets from its P column.
 *
 * rx_track_evolve(generation): slot k of the new pool, for every k < n_tracks: a slot
 * not in `slots` is copied (points and width, bit for bit) from cp_off / cp / width to
 * its place in cp_off_new / cp_new / width_new; a spawned slot is written there by its
 * plan row, and plan[j][3] = the edits applied.  A slot whose span in cp_off_new is
 * not the P its rule gives is not written, and its width_new becomes NaN (a bad track
 * to rx_build_tracks): nothing is ever written outside [cp_off_new[k], cp_off_new[k+1]).
 * Reads slots, cp_off, cp, width, plan, cp_off_new; writes cp_new, width_new, plan[.][3].
 * cp_new and width_new must not overlap cp and width.
 *
 * All pointers are DEVICE pointers, the offsets included; the *_host twins take the
 * same arguments as HOST pointers, ignore `stream`, make no HIP call and give the same
 * bits.  No host wait and no allocation.  With n_spawn == 0 the plan call does nothing
 * and the evolve call copies the pool (slots and plan may then be null).
 *
 * Checked before any HIP call (RX_EINVAL, the message names the field): a null io,
 * n_tracks <= 0, n_spawn outside 0..n_tracks, null pointers among the ones the entry
 * point reads, edit_frac outside [0, 1] or NaN. */
typedef struct rx_track_evolve_io {
  int32_t n_tracks;            /* slots of the pool, > 0 */
  int32_t n_spawn;             /* slots to replace, 0..n_tracks */
  const int32_t* slots;        /* [n_spawn] ascending, distinct */
  const int32_t* cp_off;       /* [n_tracks + 1] the pool as it stands: offsets in points */
  const double* cp;            /* [cp_off[n_tracks]][2] */
  const double* width;         /* [n_tracks] */
  const int64_t* cdf_score;    /* [n_tracks] rx_track_learn_tables' rank table (plan only) */
  int32_t* plan;               /* [n_spawn][4] = (kind, parent or -1, P, edits applied) */
  const int32_t* cp_off_new;   /* [n_tracks + 1] (evolve only) */
  double* cp_new;              /* [cp_off_new[n_tracks]][2] out (evolve only) */
  double* width_new;           /* [n_tracks] out (evolve only) */
  uint64_t seed;
} rx_track_evolve_io;
int rx_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* stream);
int rx_track_evolve_plan_host(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac, void* stream);
int rx_track_evolve(const rx_track_evolve_io* ev, uint32_t generation, void* stream);
int rx_track_evolve_host(const rx_track_evolve_io* ev, uint32_t generation, void* stream);

/* ABI v25, additive: TRACK EVOLUTION IN PLACE -- the same fresh tracks and edited
 * children for a pool whose slots keep their point counts (the episodic trainers'
 * partial resample, rx.track_evolve_episodic): no offset moves, so the pool buffer,
 * the resident track table and the captured rollout graphs all stay.  An edited
 * child must have its slot's point count, so the parent is drawn among the slots of
 * that point count only: the rank table is regrouped by point count on the device.
 * Since the host knows every spawned slot's P beforehand, nothing is downloaded
 * between the three calls.  Rules: csrc/rx_track_evolve.h, DESIGN.md §4.
 *
 * rx_track_evolve_classes(): with P_k = cp_off[k+1] - cp_off[k] and w_k = cdf_score[k] -
 * cdf_score[k-1] (w_0 = cdf_score[0]):
 *   order[n_tracks]      the slots sorted by (P_k, k) ascending (a stable counting sort);
 *                        a slot with P_k outside [1, 64] belongs to no class, weighs 0
 *                        and follows the last class in slot order;
 *   cdf_class[n_tracks]  the inclusive integer scan of w[order[i]], through the classes
 *                        without restarting;
 *   class_end[65]        class_end[p] = the number of slots with 1 <= P <= p, class_end[0] = 0.
 * Reads cp_off, cdf_score; writes order, cdf_class, class_end.  It does not look at the
 * spawn set (n_spawn only has to be in range; slots may be null).
 *
 * rx_track_evolve_inplace(generation, edit_frac): for j < n_spawn, k = slots[j], c = P_k:
 *   lo = class_end[c-1], hi = class_end[c], base = lo ? cdf_class[lo-1] : 0,
 *   F = cdf_class[hi-1] - base;  draw 0: an EDIT when u < edit_frac and F > 0, else FRESH;
 *   EDIT:  t = base + mulhi(h, F), parent = order[i] for the smallest i in [lo, hi) with
 *          t < cdf_class[i] (the slot itself and slots being replaced included: the OLD
 *          points are read); the child is rx_track_evolve's edit of it;
 *   FRESH: draw 1 is consumed and discarded; rx_track_evolve's fresh track of P_k points.
 *   plan[j] = (kind, parent or -1, P_k, edits applied); the track goes to
 *   cp_out[out_off[j] .. out_off[j+1]) and width_out[j], a compact staging buffer.
 * A slot whose span in out_off is not P_k, or whose P_k lies outside [1, 64], is not
 * written at all: width_out[j] = NaN (a bad track to rx_build_tracks), plan[j] =
 * (FRESH, -1, P_k, 0).  Reads slots, cp_off, cp, width, order, cdf_class, class_end, out_off;
 * writes plan, cp_out, width_out.  The pool is not written.
 *
 * rx_track_evolve_commit(): the staging rows copied over the spawned slots' spans of cp
 * and over width[slots[j]]; every other byte of the pool stays.  A slot inplace did
 * not write takes the NaN width and keeps its points.  Reads slots, cp_off, out_off,
 * cp_out, width_out; writes cp, width.  To be queued after rx_track_evolve_inplace on
 * the same stream.
 *
 * Pointers, twins, waits and allocation as above.  With n_spawn == 0 inplace and
 * commit do nothing.  Checked before any HIP call (RX_EINVAL, the message names the
 * field): a null io, n_tracks <= 0, n_spawn outside 0..n_tracks, null pointers among
 * the ones the entry point reads or writes, edit_frac outside [0, 1] or NaN. */
typedef struct rx_track_evolve_inplace_io {
  int32_t n_tracks;            /* slots of the pool, > 0 */
  int32_t n_spawn;             /* slots to replace, 0..n_tracks */
  const int32_t* slots;        /* [n_spawn] ascending, distinct */
  const int32_t* cp_off;       /* [n_tracks + 1] offsets in points; they never change */
  double* cp;                  /* [cp_off[n_tracks]][2] the pool: read by inplace, written by commit */
  double* width;               /* [n_tracks] likewise */
  const int64_t* cdf_score;    /* [n_tracks] rx_track_learn_tables' rank table (classes only) */
  int32_t* order;              /* [n_tracks] slots by (P, slot) */
  int64_t* cdf_class;          /* [n_tracks] the rank weights scanned in that order */
  int32_t* class_end;          /* [65] slots with 1 <= P <= p */
  int32_t* plan;               /* [n_spawn][4] = (kind, parent or -1, P, edits applied) */
  const int32_t* out_off;      /* [n_spawn + 1] staging offsets in points */
  double* cp_out;              /* [out_off[n_spawn]][2] staging */
  double* width_out;           /* [n_spawn] staging */
  uint64_t seed;
} rx_track_evolve_inplace_io;
int rx_track_evolve_classes(const rx_track_evolve_inplace_io* ev, void* stream);
int rx_track_evolve_classes_host(const rx_track_evolve_inplace_io* ev, void* stream);
int rx_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac, void* stream);
int rx_track_evolve_inplace_host(const rx_track_evolve_inplace_io* ev, uint32_t generation, double edit_frac,
                                 void* stream);
int rx_track_evolve_commit(const rx_track_evolve_inplace_io* ev, void* stream);
int rx_track_evolve_commit_host(const rx_track_evolve_inplace_io* ev, void* stream);

/* ABI v25, additive: POSITIONS REGROUPED BY SLOT -- on the lane-varying schedule a wave holds 64
 * consecutive positions of any slots, rx_assign orders the positions by slot, and every episodic
 * draw (rx_track_episode_step) sends one env to another slot and leaves it where it sits.  The
 * regroup puts the positions back in slot order on the device: it resets nothing and leaves
 * every env-order output as it would have been (DESIGN.md §3 "Positions regrouped by slot").
 *
 * The plan.  New position j holds what old position src[j] held, where src is the old
 * positions ordered by (pos_slot[p], p) ascending -- a STABLE sort, so the layout is a function
 * of its inputs alone (unlike the spatial re-sort's, whose order inside a bin follows the
 * arrival of atomics), and
 *   perm_out[j] = perm[src[j]],  pos_slot_out[j] = pos_slot[src[j]],  env_pos_out[perm_out[j]] = j.
 * rx_regroup_plan_host: HOST pointers, plain C++, no HIP call; it takes no stream and is not one
 * of the (device, host) pairs that share a body and a refusal table.  RX_EINVAL, each with its own
 * message and nothing written: n < 0, n_tracks <= 0, a null pointer, a slot outside
 * [0, n_tracks), a perm entry outside [0, n).  The outputs must not overlap the inputs.
 * rx_regroup_plan: the same arrays as DEVICE pointers, a scratch buffer of at least
 * rx_regroup_scratch_bytes(n, n_tracks) bytes (4-byte aligned; -1 for n < 0 or n_tracks <= 0)
 * and a stream.  Launches only: no allocation, no host wait, no transfer.  It equals the
 * twin element for element on every input the twin accepts; on others it writes some
 * permutation and never outside its buffers.  Checked before any launch (RX_EINVAL): n,
 * n_tracks, null pointers, scratch_bytes too small, scratch misaligned.
 *
 * rx_regroup_slots: the move on a live handle -- the plan from the handle's env order and
 * position slots, the working-state rows gathered by src into the shadow copy, and state,
 * env order and position slots copied back; the env's position array becomes the inverse of
 * the new order.  Every buffer keeps its address and the scratch was reserved by rx_assign,
 * so the call is stream-ordered and may be captured.  To be called between two calls that
 * step the env (never inside one: rx_steps' snapshots are indexed by position within a call).
 * Refused before any launch: null handle RX_EINVAL; no track table, no assignment or no
 * bound state RX_ESTATE; a two-car handle RX_EINVAL; a schedule that is not lane-varying
 * RX_EINVAL (the grouped and wide schedules bind waves to slots: rx_assign is their regroup).
 *
 * rx_lane_layout: a blocking download of the env order, the slot at each position and the
 * position of each env (int32 [n_envs] each, HOST pointers), for tests and tools; the same
 * refusals, and RX_EINVAL for a null output. */
int32_t rx_regroup_plan_host(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot,
                             int32_t* src_out, int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out);
int64_t rx_regroup_scratch_bytes(int32_t n, int32_t n_tracks);
int rx_regroup_plan(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot, int32_t* src_out,
                    int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out, void* scratch,
                    int64_t scratch_bytes, void* stream);
int rx_regroup_slots(rx_env* h, void* stream);
int rx_lane_layout(rx_env* h, int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out);

#ifdef __cplusplus
}
#endif
#endif /* RX_H_ */
