// rx_eval.hip -- the per-step metric accumulation of an evaluation
// (rx_eval_steps, ABI v25): utils/metrics.py:55-67 (single agent) and :108-125
// (two cars) for every episode of the protocol at once.
//
// k_eval_acc<A>: one lane per env POSITION p, launched once after every step.
// The post-step x, y and flags come from the engine's working state, which is
// in position order (element A * p + q; env e = perm[p]); the step's reward,
// info and done come from the rx_io buffers and the record lives in the
// caller's acc / active arrays, all three in env order.  The launch follows
// the step's spatial re-sort on the same stream, and the re-sort writes the
// moved rows back into the same perm / state buffers, so perm and the state
// rows read here are consistent with each other.
//
// Arithmetic: the float64 operations of rx.evaluate's eager loop, in its order
// (dx * dx + dy * dy with a separate multiply and add under -ffp-contract=off,
// the correctly rounded sqrt, one add per step into each sum), so the record
// is bit-equal to the eager one.
//
// The active count drops once per wave: ballot of the lanes whose episode
// ended, popcount, one vector atomic by lane 0.  With *n_active == 0 on entry
// nothing is left to do.  A wave that reads 0 while the launch's other waves
// are still counting down holds no active env either (its own envs are counted
// until it subtracts them), so the early return is safe at any time.
//
// 10 doubles read and written per active (env, car) and step: a few KB per
// launch at the protocol's 200 episodes -- latency, not bandwidth.
#include <hip/hip_runtime.h>

#include "rx_internal.h"

namespace {

constexpr int kEvalBlock = 256;

template <int A>
__global__ __launch_bounds__(kEvalBlock) void k_eval_acc(int n, const int32_t* __restrict__ perm,
                                                          const double* __restrict__ x, const double* __restrict__ y,
                                                          const uint8_t* __restrict__ flags,
                                                          const double* __restrict__ reward64,
                                                          const double* __restrict__ info,
                                                          const float* __restrict__ done, double* __restrict__ acc,
                                                          uint8_t* __restrict__ active, int32_t* n_active) {
  if (*n_active == 0) return;
  const int p = blockIdx.x * kEvalBlock + threadIdx.x;
  bool ended = false;
  if (p < n) {
    const int e = perm[p];
    if (active[e]) {
      const double steps = acc[(int64_t)e * A * RX_EVAL_W + 2];  // per env: car 0's copy
#pragma unroll
      for (int q = 0; q < A; ++q) {
        const int64_t eq = (int64_t)e * A + q;
        double* r = acc + eq * RX_EVAL_W;
        const int i = A * p + q;
        const double cx = x[i], cy = y[i];
        r[0] = r[0] + reward64[eq];
        if (steps > 0.0) {  // utils/metrics.py:59-64: the first step has no previous position
          const double dx = cx - r[7], dy = cy - r[8];
          r[1] = r[1] + sqrt(dx * dx + dy * dy);
        }
        r[7] = cx;
        r[8] = cy;
        r[2] = steps + 1.0;
        r[3] = info[eq * RX_INFO_W + RX_INFO_PROGRESS];
        r[4] = info[eq * RX_INFO_W + RX_INFO_SPEED];
        r[5] = info[eq * RX_INFO_W + RX_INFO_PLACEMENT];
        r[6] = (double)flags[i];
      }
      if (done[e] != 0.0f) {
        active[e] = 0;
        ended = true;
      }
    }
  }
  const unsigned long long m = __ballot(ended);
  if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(n_active, -(int)__builtin_popcountll(m));
}

}  // namespace

extern "C" int rx_launch_eval_acc(int n, int A, const int32_t* perm, const rx_state* work, const rx_io* io,
                                  double* acc, uint8_t* active, int32_t* n_active, hipStream_t s) {
  if (n <= 0) return 0;
  if (A != 1 && A != 2) return (int)hipErrorInvalidValue;
  const int grid = (n + kEvalBlock - 1) / kEvalBlock;
  if (A == 1)
    hipLaunchKernelGGL(k_eval_acc<1>, dim3(grid), dim3(kEvalBlock), 0, s, n, perm, work->x, work->y, work->flags,
                       io->reward64, io->info, io->done_f32, acc, active, n_active);
  else
    hipLaunchKernelGGL(k_eval_acc<2>, dim3(grid), dim3(kEvalBlock), 0, s, n, perm, work->x, work->y, work->flags,
                       io->reward64, io->info, io->done_f32, acc, active, n_active);
  return (int)hipGetLastError();
}
