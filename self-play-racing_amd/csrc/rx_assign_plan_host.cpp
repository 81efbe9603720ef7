// rx_assign_plan_host.cpp -- the assignment planner (rx_assign_plan.h): rx_config's range
// checks, the launch schedule, the env order, the dynamics- and ray-wave tables with their
// XCD placement, and the spatial sort's bins.  Pure functions of a few integers: compiled
// as plain C++, no HIP call and no handle, so the tables that decide which lane casts
// which ray are tested on the CPU (tests/test_assign_plan_cpu.py).  rx_assign (rx_api.cpp)
// uploads what rx_plan_assignment returns.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "rx_assign_plan.h"

namespace {

int fail(std::string* err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return code;
}

// The launch schedule (rx_config ABI v17 fields; 0 = the measured default for N) of N envs of A
// cars over slots of slot_n envs and at least min_w waypoints.  ray_tail is the request: the
// placement clips it to the classes there are.
rx_sched resolve_schedule(const rx_config& c, int min_w, const std::vector<int32_t>& slot_n, int32_t lane_cars) {
  const int N = c.n_envs, A = c.n_agents;
  rx_sched s;
  s.dyn_lpe = (A == 1 && N <= RX_DYN1_SMALL_N) ? RX_DYN1_LPE_SMALL : 1;
  const int wide_n = c.wide_n == 0 ? RX_WIDE_N : c.wide_n;  // -1: never
  if (A == 1 && N <= wide_n) s.dyn_lpe = 64;
  if (A == 1 && c.dyn_lpe != 0) s.dyn_lpe = c.dyn_lpe;
  s.argmin_window = c.argmin_window == 0 ? 2 : (c.argmin_window < 0 ? 0 : c.argmin_window);
  // the window [prev - H, prev + H] is wrapped into [0, W) by one +-W: needs H <= W of every slot
  s.argmin_window = std::min(s.argmin_window, min_w);
  // few envs: the culled raycast is a latency chain over too few waves to
  // fill the chip, so 2 or 4 lanes share one ray and split its leaves
  s.ray_lpr = 1;
  if (c.ray_order == 2 && s.dyn_lpe != 64) {
    const long long pairs = (long long)N * A, lpr2_n = A == 2 ? RX_RAY2_LPR2_N : RX_RAY_LPR2_N;
    s.ray_lpr = pairs <= RX_RAY_LPR4_N ? 4 : (pairs <= lpr2_n ? 2 : 1);
    if (c.ray_lpr != 0) s.ray_lpr = c.ray_lpr;
  }
  // few single-agent envs: REWARD (a latency chain of argmins) outlasts the
  // raycast beside it in k_step2 unless 2 lanes share an env's five points
  s.reward_lpe = (A == 1 && N <= RX_REWARD_LPE2_N) || (A == 2 && N <= RX_REWARD2_LPE2_N) ? 2 : 1;
  if (c.reward_lpe != 0) s.reward_lpe = c.reward_lpe;
  s.split = c.split >= 0;
  // ray-wave class order and the tail split (ABI v19; scheduling only)
  s.ray_dispatch = c.ray_dispatch == 0 ? RX_RAY_DISPATCH : (c.ray_dispatch < 0 ? 0 : c.ray_dispatch);
  s.ray_tail_lpr = c.ray_tail_lpr == 0 ? RX_RAY_TAIL_LPR : c.ray_tail_lpr;
  // few (env, car) pairs: the ray waves are short and the sort is up to 40 % of
  // k_kin's wave, so every other launch keeps the previous task order
  s.task_sort = c.task_sort != 0 ? c.task_sort : ((long long)N * A <= RX_TASK_SORT2_PAIRS ? 2 : 1);
  s.ray_tail = c.ray_tail == 0 ? RX_RAY_TAIL : (c.ray_tail < 0 ? 0 : c.ray_tail);
  if (c.ray_order != 2 || s.ray_lpr != 1 || s.ray_dispatch == 0 || s.dyn_lpe == 64) s.ray_tail = 0;
  s.ray_tail_from = -1;
  // Lane-varying track slots (ABI v23): grouping envs by slot gives every slot
  // ceil(n_k / 64) dynamics waves; with many distinct slots (gen_tracks(N, seed=None): one env
  // each) those waves hold a lane or two.  Auto rule: take waves of 64 consecutive positions of
  // ANY slots (per-lane track loads) when the grouping would need more than twice ceil(N / 64)
  // waves.  Single-agent envs at one lane per env (the split step or the one-kernel k_dyn1<1>);
  // it implies one lane per ray and per REWARD env and no ray-task sort or spatial re-sort.
  // Two-car envs (k_kin2 / k_dyn2 at a lane per env) take the same schedule by the same rule, but
  // from the handle's option (rx_set_lane_cars), not from rx_config.lane_tracks: off unless asked.
  {
    long long grouped = 0;
    for (const int32_t n : slot_n) grouped += (n + 63) / 64;
    const long long full = (N + 63) / 64;
    const bool can = s.dyn_lpe == 1;  // (two-car envs: always)
    const int32_t mode = A == 2 ? lane_cars : c.lane_tracks;
    s.lane_tracks = can && mode >= 0 && (mode == 1 || grouped > 2 * full) ? 1 : 0;
  }
  if (s.lane_tracks) {
    s.ray_lpr = 1;
    s.reward_lpe = 1;
    s.ray_dispatch = 0;
    s.ray_tail = 0;
  }
  return s;
}

// The wave tables before placement.  group_end: the end index (in ray) of each 64-env block's
// waves, for the layouts that are placed (every one but ray_order 0 grouped by slot).
struct wave_tables {
  std::vector<rx_wave> dyn, ray;
  std::vector<int> group_end;
};

// lane-varying: 64 consecutive positions of any slots, (env, agent, ray) tasks
wave_tables lane_varying_waves(int N, int A, int R) {
  wave_tables t;
  for (int ps = 0; ps < N; ps += 64) {
    const int cnt = std::min(64, N - ps), nt = cnt * A * R;
    t.dyn.push_back(rx_wave{-1, ps, 0, cnt});
    for (int j = 0; j < nt; j += 64) t.ray.push_back(rx_wave{-1, ps, j, std::min(64, nt - j)});
    t.group_end.push_back((int)t.ray.size());
  }
  return t;
}

// grouped by slot: every wave holds envs of one slot, the ray waves in the layout of ray_order
wave_tables grouped_waves(const rx_config& c, const rx_sched& s, const int32_t* track_of_env,
                          const std::vector<int32_t>& perm) {
  const int N = c.n_envs, A = c.n_agents, R = c.n_sensors;
  const int tpw = 64 / s.ray_lpr;  // ray tasks per wave
  wave_tables t;
  std::vector<rx_wave>&dyn = t.dyn, &ray = t.ray;
  int g0 = 0;
  while (g0 < N) {
    const int k = track_of_env[perm[g0]];
    int g1 = g0;
    while (g1 < N && track_of_env[perm[g1]] == k) ++g1;
    const int ng = g1 - g0;
    const int epw = A == 1 ? 64 / s.dyn_lpe : 64;  // envs per dynamics wave
    for (int st = 0; st < ng; st += epw) dyn.push_back(rx_wave{k, g0 + st, 0, std::min(epw, ng - st)});
    if (c.ray_order == 2) {  // per dynamics wave: its envs' A*R tasks (direction-sorted by k_dyn), tpw a wave
      for (int st = 0; st < ng; st += epw) {
        const int cnt = std::min(epw, ng - st), nt = cnt * A * R, ps = g0 + st;
        for (int j = 0; j < nt; j += tpw) ray.push_back(rx_wave{k, ps, ps * A * R + j, std::min(tpw, nt - j)});
        t.group_end.push_back((int)ray.size());
      }
    } else if (c.ray_order == 0) {
      const long long tasks = (long long)ng * A * R;
      for (long long st = 0; st < tasks; st += 64)
        ray.push_back(rx_wave{k, g0, (int32_t)st, (int32_t)std::min<long long>(64, tasks - st)});
    } else {  // ray-major: one (agent, ray) x one 64-env block per wave, grouped by block
      for (int b = 0; 64 * b < ng; ++b) {
        for (int qr = 0; qr < A * R; ++qr)
          ray.push_back(rx_wave{k, g0, qr * ng + 64 * b, std::min(64, ng - 64 * b)});
        t.group_end.push_back((int)ray.size());
      }
    }
    g0 = g1;
  }
  return t;
}

// ray_dispatch (rx_config, ABI v19): the rank at which each of a group's maxw classes is
// dispatched.  0 = group-octet-major (ranks unused); 1..3 = class-major, every group's class-j
// wave in one run, the classes in the order 1 centre first (|2j - (maxw - 1)| ascending),
// 2 ascending j, 3 edge classes first (|2j - (maxw - 1)| descending, the default).
int class_ranks(int mode, int maxw, std::vector<int>* out, std::string* err) {
  std::vector<int> rank(maxw);
  std::iota(rank.begin(), rank.end(), 0);
  if (mode == 1 || mode == 3) {
    std::vector<int> cls(maxw);
    std::iota(cls.begin(), cls.end(), 0);
    auto off = [&](int j) { return std::abs(2 * j - (maxw - 1)); };
    std::stable_sort(cls.begin(), cls.end(), [&](int x, int y) { return mode == 1 ? off(x) < off(y) : off(x) > off(y); });
    for (int r = 0; r < maxw; ++r) rank[cls[r]] = r;
  }
#ifdef RX_RAY_ORDER_LIST
  {  // A/B builds: an explicit class order for 11-class groups (ray_dispatch >= 1)
    const int lst[] = RX_RAY_ORDER_LIST;
    if (mode >= 1 && maxw == (int)(sizeof(lst) / sizeof(lst[0]))) {
      // the list must be a permutation of 0..maxw-1: a repeated class would give two
      // ray waves one placed slot (one silently overwritten, its rays never cast)
      std::vector<bool> seen(maxw, false);
      for (int r = 0; r < maxw; ++r) {
        if (lst[r] < 0 || lst[r] >= maxw || seen[lst[r]])
          return fail(err, RX_EINVAL, "RX_RAY_ORDER_LIST is not a permutation of 0..%d", maxw - 1);
        seen[lst[r]] = true;
        rank[lst[r]] = r;
      }
    }
  }
#endif
  (void)err;
  out->swap(rank);
  return RX_OK;
}

// XCD-aware placement: workgroups are dealt round-robin over the 8 XCDs
// (MI355X_MICROARCH.md, workgroup dispatch), and every wave of one 64-env
// block writes into the same obs rows, so the (up to) A*R waves of block g
// go to physical indices p = ((g / 8) * maxw + j) * 8 + g % 8 -- one XCD,
// one L2 to merge their partial-line writes.  Padding waves have count 0.
// That is mode 0; in the class-major modes (class_ranks) the XCD of a group's
// waves is g % 8 as well (padded is a multiple of 8).  Dispatch order is scheduling only.
//
// The tail split (ray_tail, class-major modes only): the waves of the last ray_tail
// ranks run as the chip drains, where a wave's latency chain -- not the shared VALU --
// sets its duration.  Each of their 64-task records becomes m = ray_tail_lpr records of
// 64 / m tasks, cast at m lanes per ray (the lanes split each scanned leaf: a shorter
// chain, the same result, DESIGN.md §3 "Lanes per ray").  Rank r occupies mult[r]
// consecutive runs of `padded` slots; sub-record s of group g's rank-r wave goes to
// base[r] + (s * (padded / 8) + g / 8) * 8 + g % 8, so it keeps the group's XCD.  All
// tail waves sit at the end of the table: *tail_from is the first of them (-1 = none),
// and *tail comes back clipped to the classes there are.
std::vector<rx_wave> place_ray_waves(const std::vector<rx_wave>& ray, const std::vector<int>& group_end,
                                     const std::vector<int>& rank, int mode, int tpw, int tail_lpr, int32_t* tail,
                                     int32_t* tail_from) {
  const size_t n_groups = group_end.size();
  const int maxw = (int)rank.size();
  const size_t padded = (n_groups + 7) / 8 * 8;
  *tail = mode == 0 ? 0 : std::min(*tail, maxw);
  std::vector<size_t> mult(maxw, 1), base(maxw + 1, 0);
  for (int r = maxw - *tail; r < maxw; ++r) mult[r] = (size_t)tail_lpr;
  for (int r = 0; r < maxw; ++r) base[r + 1] = base[r] + mult[r] * padded;
  std::vector<rx_wave> placed(base[maxw], rx_wave{0, 0, 0, 0});
  for (size_t g = 0; g < n_groups; ++g) {
    const int w0 = g ? group_end[g - 1] : 0;
    for (int j = 0; w0 + j < group_end[g]; ++j) {
      const rx_wave w = ray[w0 + j];
      if (mode == 0) {
        placed[((g / 8) * maxw + j) * 8 + g % 8] = w;
        continue;
      }
      const int r = rank[j];
      const int m = (int)mult[r], per = tpw / m;
      for (int sub = 0; sub < m; ++sub) {
        const size_t slot = base[r] + ((size_t)sub * (padded / 8) + g / 8) * 8 + g % 8;
        placed[slot] = rx_wave{w.track, w.perm_start, w.task_start + sub * per,
                               std::max(0, std::min(per, w.count - sub * per))};
      }
    }
  }
  *tail_from = *tail > 0 ? (int32_t)base[maxw - *tail] : -1;
  return placed;
}

// spatial sort bins: slot k owns (W_k >> shift) + 1 consecutive bins from
// sort_base[k]; the smallest shift that keeps all bins <= RX_SORT_MAX_BINS.
// More slots than that (at most ~1 env per slot): nothing to regroup, no sort.
void sort_bins(int32_t n_tracks, const int32_t* wp_off, rx_sched* s, std::vector<int32_t>* sort_base) {
  int shift = 0;
  long long total = 0;
  for (;; ++shift) {
    total = 0;
    for (int k = 0; k < n_tracks; ++k) total += ((wp_off[k + 1] - wp_off[k]) >> shift) + 1;
    if (total <= RX_SORT_MAX_BINS || shift >= 30) break;
  }
  if (total > RX_SORT_MAX_BINS) return;
  std::vector<int32_t> base(n_tracks);
  int32_t run = 0;
  for (int k = 0; k < n_tracks; ++k) {
    base[k] = run;
    run += ((wp_off[k + 1] - wp_off[k]) >> shift) + 1;
  }
  sort_base->swap(base);
  s->sort_bins = (int32_t)total;
  s->sort_shift = shift;
  s->sort_on = true;
}

}  // namespace

int rx_config_check(const rx_config* cfg, std::string* err) {
  if (cfg->n_envs <= 0) return fail(err, RX_EINVAL, "n_envs must be > 0 (got %d)", cfg->n_envs);
  if (cfg->n_agents != 1 && cfg->n_agents != 2)
    return fail(err, RX_EINVAL, "n_agents must be 1 or 2 (got %d)", cfg->n_agents);
  if (cfg->n_sensors <= 0 || cfg->n_sensors > 256)
    return fail(err, RX_EINVAL, "n_sensors out of range (%d)", cfg->n_sensors);
  if (cfg->max_steps <= 0) return fail(err, RX_EINVAL, "max_steps must be > 0");
  if (cfg->ray_order < 0 || cfg->ray_order > 2)
    return fail(err, RX_EINVAL, "ray_order must be 0, 1 or 2 (got %d)", cfg->ray_order);
  if (cfg->cull_super < 0 || cfg->cull_super > 64)
    return fail(err, RX_EINVAL, "cull_super out of range (%d)", cfg->cull_super);
  if (cfg->autoreset < RX_AUTORESET_NEXT_STEP || cfg->autoreset > RX_AUTORESET_DISABLED)
    return fail(err, RX_EINVAL, "bad autoreset mode %d", cfg->autoreset);
  // launch schedule (ABI v17): 0 = auto, -1 = off where there is an off state
  auto tri = [](int32_t v) { return v == 0 || v == 1 || v == -1; };
  auto lanes = [](int32_t v, bool wide) { return v == 0 || v == 1 || v == 2 || v == 4 || (wide && v == 64); };
  if (!tri(cfg->split)) return fail(err, RX_EINVAL, "split must be 0 (auto), 1 or -1 (got %d)", cfg->split);
  if (!tri(cfg->seg_filter))
    return fail(err, RX_EINVAL, "seg_filter must be 0 (auto), 1 or -1 (got %d)", cfg->seg_filter);
  if (!tri(cfg->box_quadrants))
    return fail(err, RX_EINVAL, "box_quadrants must be 0 (auto), 1 or -1 (got %d)", cfg->box_quadrants);
  if (cfg->wide_n < -1) return fail(err, RX_EINVAL, "wide_n must be >= -1 (got %d)", cfg->wide_n);
  if (!lanes(cfg->dyn_lpe, true))
    return fail(err, RX_EINVAL, "dyn_lpe must be 0 (auto), 1, 2, 4 or 64 (got %d)", cfg->dyn_lpe);
  if (!lanes(cfg->ray_lpr, false))
    return fail(err, RX_EINVAL, "ray_lpr must be 0 (auto), 1, 2 or 4 (got %d)", cfg->ray_lpr);
  if (!lanes(cfg->reward_lpe, false))
    return fail(err, RX_EINVAL, "reward_lpe must be 0 (auto), 1, 2 or 4 (got %d)", cfg->reward_lpe);
  if (cfg->argmin_window < -1 || cfg->argmin_window > 32)
    return fail(err, RX_EINVAL, "argmin_window must be 0 (auto), -1 (none) or 1 .. 32 (got %d)", cfg->argmin_window);
  if (cfg->ray_dispatch < -1 || cfg->ray_dispatch > 3)
    return fail(err, RX_EINVAL, "ray_dispatch must be 0 (auto), -1, 1, 2 or 3 (got %d)", cfg->ray_dispatch);
  if (cfg->ray_tail < -1 || cfg->ray_tail > 16)
    return fail(err, RX_EINVAL, "ray_tail must be 0 (auto), -1 (none) or 1 .. 16 (got %d)", cfg->ray_tail);
  if (cfg->ray_tail_lpr != 0 && cfg->ray_tail_lpr != 2 && cfg->ray_tail_lpr != 4)
    return fail(err, RX_EINVAL, "ray_tail_lpr must be 0 (auto), 2 or 4 (got %d)", cfg->ray_tail_lpr);
  if (cfg->lane_tracks < -1 || cfg->lane_tracks > 1)
    return fail(err, RX_EINVAL, "lane_tracks must be 0 (auto), 1 or -1 (got %d)", cfg->lane_tracks);
  if (cfg->reserved0 != 0)
    return fail(err, RX_EINVAL, "reserved0 must be 0 (ABI v23 dropped the kin_sort schedule; got %d)", cfg->reserved0);
  if (cfg->task_sort < 0 || cfg->task_sort > 16)
    return fail(err, RX_EINVAL, "task_sort must be 0 (auto) or 1 .. 16 (got %d)", cfg->task_sort);
  if (cfg->n_agents == 2 && (cfg->dyn_lpe > 1 || cfg->reward_lpe > 2))
    return fail(err, RX_EINVAL, "n_agents = 2: dyn_lpe > 1 is a single-agent schedule, and reward_lpe is 1 or 2 "
                                "(a lane per car)");
  if ((long long)cfg->n_envs * cfg->n_agents * cfg->n_sensors > 0x7fffffffLL)
    return fail(err, RX_EINVAL, "n_envs * n_agents * n_sensors overflows int32");
  return RX_OK;
}

int rx_plan_assignment(const rx_config& c, int32_t n_tracks, const int32_t* wp_off, const int32_t* track_of_env,
                       rx_assignment* out, std::string* err, int32_t lane_cars) {
  int rc = rx_config_check(&c, err);
  if (rc != RX_OK) return rc;
  if (lane_cars < -1 || lane_cars > 1)
    return fail(err, RX_EINVAL, "lane_cars must be 0 (auto), 1 or -1 (got %d)", lane_cars);
  const int N = c.n_envs, A = c.n_agents, R = c.n_sensors;
  for (int e = 0; e < N; ++e)
    if (track_of_env[e] < 0 || track_of_env[e] >= n_tracks)
      return fail(err, RX_EINVAL, "env %d assigned to track %d (have %d)", e, track_of_env[e], n_tracks);
  if (c.ray_order == 2 && A * R > 16 * A)
    return fail(err, RX_EINVAL, "ray_order 2 supports at most 16 sensors (got %d)", R);
  rx_assignment a;
  // group envs by slot (stable: env order inside a slot is preserved)
  a.perm.resize(N);
  std::iota(a.perm.begin(), a.perm.end(), 0);
  std::stable_sort(a.perm.begin(), a.perm.end(),
                   [&](int32_t x, int32_t y) { return track_of_env[x] < track_of_env[y]; });
  a.slot_n.assign(n_tracks, 0);
  for (int e = 0; e < N; ++e) ++a.slot_n[track_of_env[e]];
  int min_w = 1 << 30;
  for (int k = 0; k < n_tracks; ++k) min_w = std::min(min_w, wp_off[k + 1] - wp_off[k]);
  rx_sched& s = a.sched;
  s = resolve_schedule(c, min_w, a.slot_n, lane_cars);
  wave_tables t = s.lane_tracks ? lane_varying_waves(N, A, R) : grouped_waves(c, s, track_of_env, a.perm);
  // Two-car lane-varying tables stay as built, block-major with no padding records: a block's
  // 2 R rays per env fill up to 2 R waves, so padding the block count to 8 would add up to
  // 14 R empty workgroups, and with a slot per lane the waves of a block share no table lines
  // for one XCD's L2 to keep.
  if (s.lane_tracks ? A == 1 : c.ray_order >= 1) {
    int maxw = 0;
    for (size_t g = 0; g < t.group_end.size(); ++g)
      maxw = std::max(maxw, t.group_end[g] - (g ? t.group_end[g - 1] : 0));
    std::vector<int> rank;
    if ((rc = class_ranks(s.ray_dispatch, maxw, &rank, err)) != RX_OK) return rc;
    t.ray = place_ray_waves(t.ray, t.group_end, rank, s.ray_dispatch, 64 / s.ray_lpr, s.ray_tail_lpr, &s.ray_tail,
                            &s.ray_tail_from);
  }
  if (s.lane_tracks) {  // the kernels read each position's slot: the order stays fixed
    a.pos_slot.resize(N);
    a.env_pos.resize(N);
    for (int p = 0; p < N; ++p) a.pos_slot[p] = track_of_env[a.perm[p]];
    for (int p = 0; p < N; ++p) a.env_pos[a.perm[p]] = p;
  } else if (c.sort_interval > 0) {
    sort_bins(n_tracks, wp_off, &s, &a.sort_base);
  }
  a.dyn.swap(t.dyn);
  a.ray.swap(t.ray);
  s.n_dyn_waves = (int32_t)a.dyn.size();
  s.n_ray_waves = (int32_t)a.ray.size();
  *out = std::move(a);
  return RX_OK;
}

void rx_sched_row(const rx_config& cfg, const rx_sched& s, int32_t dyn_calls, int32_t* out) {
  const int32_t v[RX_SCHEDULE_W] = {s.split ? 1 : 0, s.dyn_lpe == 64 ? 1 : 0, s.dyn_lpe, s.ray_lpr, s.reward_lpe,
                                    s.argmin_window, cfg.seg_filter >= 0 ? 1 : 0,
                                    cfg.box_quadrants >= 0 ? 1 : 0, s.n_dyn_waves, s.n_ray_waves,
                                    s.ray_dispatch, s.ray_tail, s.ray_tail_lpr, s.ray_tail_from,
                                    s.task_sort, s.lane_tracks, dyn_calls, 0};
  std::copy(v, v + RX_SCHEDULE_W, out);
}
