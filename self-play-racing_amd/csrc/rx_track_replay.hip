// rx_track_replay.hip -- the replay scores of the track curriculum (ABI v25
// additive; rules in rx_track_replay.h, DESIGN.md §4 "Replay scores"):
//   k_track_adv_tally     once per update over the [T][n] advantages: a lane per env
//                         column walks a chunk of rows (coalesced 4-byte row loads),
//                         keeps (samples, mag_q) in registers, the wave folds its
//                         lanes per slot and one lane per slot issues the two int64
//                         atomic adds;
//   k_track_adv_tally_slots  the same walk with the slot read PER STEP from slots[T][n]
//                         (and the autoreset rows of dones left out): a lane flushes its
//                         registers through the same fold when its slot changes;
//   k_track_learn_fold    once per update, a lane per slot: learn -> score, seen;
//   k_track_rank          once per resample: a counting rank, a workgroup owns 64
//                         slots and streams every key through LDS in tiles, four
//                         waves sharing the comparisons of each slot;
//   k_track_learn_tables  once per resample, ONE workgroup: the two weights and the
//                         two inclusive integer scans in one pass
//                         (k_track_scores' chunked scan);
//   k_track_learn_draw    once per resample, a lane per env;
//   k_track_learn_episode once per rollout step: k_track_episode (rx_curriculum.hip) with
//                         the draw from the replay tables.
// Arguments are checked by rx_api.cpp.
#include <hip/hip_runtime.h>

#include "rx.h"
#include "rx_curriculum.h"  // rx_tc_wave_episode_tally
#include "rx_track_replay.h"

namespace {

constexpr int kTallyThreads = 256;
constexpr int kTallyMinRows = 32;     // rows a lane walks at least (but for T below it)
constexpr int kTallyBlocks = 256;     // workgroups the (env blocks x row chunks) grid aims for
constexpr int kTallyBatch = 4;        // rows k_track_adv_tally_slots loads before it takes them

// The fold of a wave's pending (slot, samples, mag) registers into learn: k_track_tally's leader
// loop (a leader slot read from the lowest pending lane, its lanes balloted, the two columns summed
// by a butterfly over the wave, ONE lane adds).  A slot held by a single lane of the wave skips the
// butterfly (`same` is wave-uniform).  EVERY lane of the wave must call it, pending or not.
__device__ __forceinline__ void wave_learn_flush(int64_t* __restrict__ learn, bool live, int32_t slot,
                                                 long long samples, long long mag) {
  unsigned long long todo = __ballot(live);
  const int lane = (int)(threadIdx.x & 63);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int32_t s = __builtin_amdgcn_readlane(slot, leader);  // wave-uniform: in [0, n_tracks)
    const bool mine = live && slot == s;
    const unsigned long long same = __ballot(mine);
    long long ns = mine ? samples : 0, nm = mine ? mag : 0;
    if (__popcll(same) > 1) {
      for (int o = 32; o > 0; o >>= 1) {
        ns += __shfl_xor(ns, o, 64);
        nm += __shfl_xor(nm, o, 64);
      }
    }
    if (lane == leader) {
      unsigned long long* row = reinterpret_cast<unsigned long long*>(learn + (size_t)s * RX_TRACK_LEARN_W);
      atomicAdd(row, (unsigned long long)ns);
      if (nm) atomicAdd(row + 1, (unsigned long long)nm);
    }
    todo &= ~same;
  }
}

// Grid (env blocks, row chunks).  A lane's slot is the same in every row, so the
// per-slot fold (wave_learn_flush) runs once per chunk, after the row loop.  Integer
// adds only: the sums do not depend on the chunking or on the order of arrival.
__global__ __launch_bounds__(kTallyThreads) void k_track_adv_tally(const int32_t* __restrict__ track,
                                                                   int64_t* __restrict__ learn,
                                                                   const float* __restrict__ adv, int32_t T, int64_t n,
                                                                   int32_t rows, int32_t n_tracks, int32_t kind) {
  const int64_t e = (int64_t)blockIdx.x * kTallyThreads + threadIdx.x;
  int32_t slot = -1;
  long long samples = 0, mag = 0;
  if (e < n) {
    const int32_t k = track[e];
    if (k >= 0 && k < n_tracks) {  // a slot outside the table is not counted
      const int32_t t0 = (int32_t)blockIdx.y * rows;
      const int32_t t1 = t0 + rows < T ? t0 + rows : T;
      const float* col = adv + e;
      for (int32_t t = t0; t < t1; ++t) {
        int64_t q;
        if (rx_tl_mag_q(col[(int64_t)t * n], kind, &q)) {
          samples += 1;
          mag += (long long)q;
        }
      }
      if (samples > 0) slot = k;
    }
  }
  wave_learn_flush(learn, slot >= 0, slot, samples, mag);
}

// k_track_adv_tally with the slot of every element read from slots[t][e].  A lane keeps
// (cur, samples, mag) of the slot its counted rows are on; the row loop is wave-uniform (its bounds
// come from blockIdx and the arguments), and when a ballot says that some lane's next counted row
// is on another slot, those lanes flush through wave_learn_flush and start again -- once per
// episode end, the other lanes of the wave only take part in the ballots.  Lanes past n, lanes
// with nothing counted and lanes on slots outside the table run every ballot and shuffle with
// nothing pending.  kDones: whether the autoreset rows (dones[t][e] != 0) are left out.
template <bool kDones>
__global__ __launch_bounds__(kTallyThreads) void k_track_adv_tally_slots(int64_t* __restrict__ learn,
                                                                         const float* __restrict__ adv,
                                                                         const int32_t* __restrict__ slots,
                                                                         const float* __restrict__ dones, int32_t T,
                                                                         int64_t n, int32_t rows, int32_t n_tracks,
                                                                         int32_t kind) {
  const int64_t e = (int64_t)blockIdx.x * kTallyThreads + threadIdx.x;
  const bool in = e < n;
  const int64_t col = in ? e : n - 1;  // a lane past n loads the last column and counts nothing
  const int32_t t0 = (int32_t)blockIdx.y * rows;
  const int32_t t1 = t0 + rows < T ? t0 + rows : T;
  int32_t cur = -1;  // >= 0: the slot of the pending sums, which then hold at least one sample
  long long samples = 0, mag = 0;
  // kTallyBatch rows are loaded at once (a row past the chunk loads the chunk's last row again and
  // counts nothing: every load is unconditional and inside the arrays), then taken one by one.
  for (int32_t t = t0; t < t1; t += kTallyBatch) {
    int32_t s[kTallyBatch];
    float a[kTallyBatch], d[kTallyBatch];
#pragma unroll
    for (int j = 0; j < kTallyBatch; ++j) {
      const int32_t tj = t + j < t1 ? t + j : t1 - 1;
      const int64_t i = (int64_t)tj * n + col;
      s[j] = slots[i];
      a[j] = adv[i];
      d[j] = kDones ? dones[i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kTallyBatch; ++j) {
      int64_t q = 0;
      const bool counted = in && t + j < t1 && rx_tl_counts(s[j], n_tracks, d[j], a[j], kind, &q);
      const bool moves = counted && cur >= 0 && s[j] != cur;
      if (__ballot(moves) != 0ull) {  // wave-uniform
        wave_learn_flush(learn, moves, cur, samples, mag);
        if (moves) {
          samples = 0;
          mag = 0;
        }
      }
      if (counted) {
        cur = s[j];
        samples += 1;
        mag += (long long)q;
      }
    }
  }
  wave_learn_flush(learn, cur >= 0, cur, samples, mag);
}

__global__ __launch_bounds__(256) void k_track_learn_fold(int64_t* __restrict__ learn, double* __restrict__ score,
                                                          int32_t* __restrict__ seen, int32_t n_tracks, int32_t update,
                                                          double alpha) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n_tracks) return;
  rx_tl_fold(learn + (size_t)k * RX_TRACK_LEARN_W, score + k, seen + k, update, alpha);
}

constexpr int kRankThreads = 256;
constexpr int kRankSlots = 64;  // slots per workgroup: a lane of EVERY wave per slot
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankTile = RX_TRACK_RANK_TILE;
constexpr int kRankPart = kRankTile / kRankWaves;  // keys of a tile each wave compares
static_assert(kRankTile % kRankThreads == 0, "every lane stages the same number of keys");

// A workgroup owns slots [k0, k0 + 64) and every key goes through LDS once per
// workgroup, kRankTile at a time.  Lane l of each of the four waves holds the key of
// slot k0 + l and counts, over its wave's quarter of the tile, the slots that stand
// before its own; the four partial counts meet in LDS at the end.  (A lane per slot
// alone leaves 65,536 slots at one wave per SIMD; four waves per slot give the
// scheduler something to issue while a wave waits.)  The tie rule (j < k) is
// wave-uniform for a tile that lies wholly below or above the workgroup's slots:
// >= there, > here; only the tile that overlaps them takes the full comparison.
__global__ __launch_bounds__(kRankThreads) void k_track_rank(const double* __restrict__ score,
                                                             const int32_t* __restrict__ seen,
                                                             int32_t* __restrict__ rank, int32_t n_tracks) {
  __shared__ unsigned long long tile[kRankTile];
  __shared__ int32_t part[kRankWaves][kRankSlots];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int32_t k0 = (int32_t)blockIdx.x * kRankSlots;
  const int32_t k = k0 + lane;
  const unsigned long long mine = k < n_tracks ? rx_tl_key(score[k], seen[k]) : 0ull;
  int32_t before = 0;
  for (int32_t base = 0; base < n_tracks; base += kRankTile) {
    const int32_t len = n_tracks - base < kRankTile ? n_tracks - base : kRankTile;
    for (int32_t i = (int32_t)threadIdx.x; i < len; i += kRankThreads)
      tile[i] = rx_tl_key(score[base + i], seen[base + i]);
    __syncthreads();
    const int32_t i0 = wave * kRankPart;
    const int32_t i1 = i0 + kRankPart < len ? i0 + kRankPart : len;  // the last tile is walked to its length only
    if (base + len <= k0) {  // every j < every k of this workgroup
#pragma unroll 16
      for (int32_t i = i0; i < i1; ++i) before += tile[i] >= mine ? 1 : 0;
    } else if (base >= k0 + kRankSlots) {  // every j > every k
#pragma unroll 16
      for (int32_t i = i0; i < i1; ++i) before += tile[i] > mine ? 1 : 0;
    } else {
#pragma unroll 4
      for (int32_t i = i0; i < i1; ++i) before += rx_tl_before(tile[i], base + i, mine, k);
    }
    __syncthreads();  // the next pass overwrites the tile
  }
  part[wave][lane] = before;
  __syncthreads();
  if (wave == 0 && k < n_tracks) {
    int32_t r = 1;
    for (int w = 0; w < kRankWaves; ++w) r += part[w][lane];
    rank[k] = r;
  }
}

constexpr int kTableThreads = RX_TRACK_LEARN_CHUNK;
constexpr int kTableWaves = kTableThreads / 64;

// k_track_scores' structure with two columns: per pass lane i takes slot base + i,
// an inclusive wave scan by shuffles, the wave totals through LDS, and the running
// totals of the passes before (every lane keeps its own copy: the same integers).
__global__ __launch_bounds__(kTableThreads) void k_track_learn_tables(const int32_t* __restrict__ rank,
                                                                      const int32_t* __restrict__ seen,
                                                                      int64_t* __restrict__ cdf_score,
                                                                      int64_t* __restrict__ cdf_stale, int32_t n_tracks,
                                                                      int32_t power, int32_t now) {
  __shared__ unsigned long long wave_total[2][kTableWaves];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  unsigned long long carry_w = 0, carry_s = 0;
  for (int base = 0; base < n_tracks; base += kTableThreads) {
    const int k = base + (int)threadIdx.x;
    unsigned long long w = 0, s = 0;
    if (k < n_tracks) {
      w = rx_tl_weight(rank[k], power);
      s = rx_tl_stale(seen[k], now);
    }
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long yw = __shfl_up(w, o, 64), ys = __shfl_up(s, o, 64);
      if (lane >= o) {
        w += yw;
        s += ys;
      }
    }
    if (lane == 63) {
      wave_total[0][wave] = w;
      wave_total[1][wave] = s;
    }
    __syncthreads();
    unsigned long long before_w = 0, total_w = 0, before_s = 0, total_s = 0;
    for (int j = 0; j < kTableWaves; ++j) {
      const unsigned long long tw = wave_total[0][j], ts = wave_total[1][j];
      if (j < wave) {
        before_w += tw;
        before_s += ts;
      }
      total_w += tw;
      total_s += ts;
    }
    if (k < n_tracks) {
      cdf_score[k] = (int64_t)(carry_w + before_w + w);
      cdf_stale[k] = (int64_t)(carry_s + before_s + s);
    }
    carry_w += total_w;
    carry_s += total_s;
    __syncthreads();  // the next pass overwrites wave_total
  }
}

__global__ __launch_bounds__(256) void k_track_learn_draw(const int64_t* __restrict__ cdf_score,
                                                          const int64_t* __restrict__ cdf_stale,
                                                          int32_t* __restrict__ track_of_env, int64_t n,
                                                          int32_t n_tracks, uint64_t seed, uint32_t generation,
                                                          double mix, double stale_mix) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  track_of_env[e] = rx_tl_draw(cdf_score, cdf_stale, n_tracks, seed, generation, (uint32_t)e, mix, stale_mix);
}

struct track_learn_episode_args {
  rx_track_io tc;  // n_tracks, track, tally
  rx_track_episode_io ep;
  const int64_t* cdf_score;
  const int64_t* cdf_stale;  // may be null when stale_mix == 0
  uint64_t seed;
  double stale_mix;
  const float* done;
  const uint8_t* terminated;
  const double* info;  // [n][RX_INFO_W]
  int64_t n;
};

// k_track_episode (rx_curriculum.hip) with the next slot from the replay tables: slot_out, the
// tally of the wave (rx_tc_wave_episode_tally, every lane), then every tallied lane draws for its
// own env (rx_tl_episode_draw) and touches only its own track / draws / pos_slot entries.
__global__ __launch_bounds__(256) void k_track_learn_episode(track_learn_episode_args a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e < a.n;
  const bool ended = in && a.done[e] != 0.0f;
  const bool any = __ballot(ended) != 0ull;
  int32_t k = -1;
  if (in && (ended || a.ep.slot_out)) k = a.tc.track[e];
  if (in && a.ep.slot_out) a.ep.slot_out[e] = k;
  if (!any) return;  // wave-uniform
  const bool live = rx_tc_wave_episode_tally(a.tc.tally, a.tc.n_tracks, ended, k, a.terminated, a.info, e);
  if (live) rx_tl_episode_draw(&a.tc, &a.ep, a.cdf_score, a.cdf_stale, a.seed, a.stale_mix, a.n, e);
}

// the rows a lane walks: enough chunks for kTallyBlocks workgroups, at least kTallyMinRows rows each
int tally_rows(int32_t T, int64_t n) {
  const int64_t env_blocks = (n + kTallyThreads - 1) / kTallyThreads;
  int64_t chunks = (kTallyBlocks + env_blocks - 1) / env_blocks;
  const int64_t most = ((int64_t)T + kTallyMinRows - 1) / kTallyMinRows;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  return (int)((T + chunks - 1) / chunks);
}

}  // namespace

extern "C" int rx_launch_track_learn_tally(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                           hipStream_t s) {
  const int rows = tally_rows(T, n);
  const dim3 grid((unsigned)((n + kTallyThreads - 1) / kTallyThreads), (unsigned)((T + rows - 1) / rows));
  hipLaunchKernelGGL(k_track_adv_tally, grid, dim3(kTallyThreads), 0, s, lt->track, lt->learn, adv, T, n, rows,
                     lt->n_tracks, lt->kind);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_learn_tally_slots(const rx_track_learn_io* lt, int32_t T, int64_t n, const float* adv,
                                                 const int32_t* slots, const float* dones, hipStream_t s) {
  const int rows = tally_rows(T, n);
  const dim3 grid((unsigned)((n + kTallyThreads - 1) / kTallyThreads), (unsigned)((T + rows - 1) / rows));
  if (dones)
    hipLaunchKernelGGL(k_track_adv_tally_slots<true>, grid, dim3(kTallyThreads), 0, s, lt->learn, adv, slots, dones, T,
                       n, rows, lt->n_tracks, lt->kind);
  else
    hipLaunchKernelGGL(k_track_adv_tally_slots<false>, grid, dim3(kTallyThreads), 0, s, lt->learn, adv, slots, dones,
                       T, n, rows, lt->n_tracks, lt->kind);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_learn_fold(const rx_track_learn_io* lt, int32_t update, double alpha, hipStream_t s) {
  hipLaunchKernelGGL(k_track_learn_fold, dim3((unsigned)((lt->n_tracks + 255) / 256)), dim3(256), 0, s, lt->learn,
                     lt->score, lt->seen, lt->n_tracks, update, alpha);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_learn_tables(const rx_track_learn_io* lt, int32_t power, int32_t now, hipStream_t s) {
  hipLaunchKernelGGL(k_track_rank, dim3((unsigned)((lt->n_tracks + kRankSlots - 1) / kRankSlots)),
                     dim3(kRankThreads), 0, s, lt->score, lt->seen, lt->rank, lt->n_tracks);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(k_track_learn_tables, dim3(1), dim3(kTableThreads), 0, s, lt->rank, lt->seen, lt->cdf_score,
                     lt->cdf_stale, lt->n_tracks, power, now);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_learn_draw(const rx_track_learn_io* lt, int64_t n, uint32_t generation, double mix,
                                          double stale_mix, hipStream_t s) {
  hipLaunchKernelGGL(k_track_learn_draw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lt->cdf_score,
                     lt->cdf_stale, lt->track_of_env, n, lt->n_tracks, lt->seed, generation, mix, stale_mix);
  return (int)hipGetLastError();
}

extern "C" int rx_launch_track_learn_episode(const rx_track_io* tc, const rx_track_learn_io* lt,
                                             const rx_track_episode_io* ep, double stale_mix, int64_t n,
                                             const float* done, const uint8_t* terminated, const double* info,
                                             hipStream_t s) {
  const track_learn_episode_args a{*tc, *ep, lt->cdf_score, lt->cdf_stale, lt->seed, stale_mix, done, terminated,
                                   info, n};
  hipLaunchKernelGGL(k_track_learn_episode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
