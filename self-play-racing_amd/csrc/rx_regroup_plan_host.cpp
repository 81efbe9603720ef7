// rx_regroup_plan_host.cpp -- the regroup of a lane-varying env's positions by slot as a pure
// function (include/rx.h rx_regroup_plan_host; the kernels are in rx_sort.hip): new position j
// holds what old position src[j] held, src being the old positions ordered by (pos_slot[p], p).
// A stable counting sort; plain C++, no HIP call.
#include <stdarg.h>
#include <stdio.h>

#include "rx_assign_plan.h"

namespace {

int fail(std::string* err, int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return code;
}

}  // namespace

int rx_plan_regroup(int32_t n, int32_t n_tracks, const int32_t* perm, const int32_t* pos_slot, int32_t* src_out,
                    int32_t* perm_out, int32_t* pos_slot_out, int32_t* env_pos_out, std::string* err) {
  const char* fn = "rx_regroup_plan_host";
  if (n < 0) return fail(err, RX_EINVAL, "%s: n must be >= 0 (got %d)", fn, n);
  if (n_tracks <= 0) return fail(err, RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n_tracks);
  const void* ptrs[] = {perm, pos_slot, src_out, perm_out, pos_slot_out, env_pos_out};
  const char* names[] = {"perm", "pos_slot", "src_out", "perm_out", "pos_slot_out", "env_pos_out"};
  for (int i = 0; i < 6; ++i)
    if (!ptrs[i]) return fail(err, RX_EINVAL, "%s: null %s", fn, names[i]);
  for (int32_t p = 0; p < n; ++p) {
    if (pos_slot[p] < 0 || pos_slot[p] >= n_tracks)
      return fail(err, RX_EINVAL, "%s: pos_slot[%d] = %d outside [0, %d)", fn, p, pos_slot[p], n_tracks);
    if (perm[p] < 0 || perm[p] >= n)
      return fail(err, RX_EINVAL, "%s: perm[%d] = %d is no env id in [0, %d)", fn, p, perm[p], n);
  }
  std::vector<int32_t> cursor((size_t)n_tracks + 1, 0);
  for (int32_t p = 0; p < n; ++p) ++cursor[(size_t)pos_slot[p] + 1];
  for (int32_t k = 0; k < n_tracks; ++k) cursor[(size_t)k + 1] += cursor[k];
  for (int32_t p = 0; p < n; ++p) src_out[cursor[pos_slot[p]]++] = p;  // ascending p inside a slot
  for (int32_t j = 0; j < n; ++j) {
    const int32_t s = src_out[j];
    perm_out[j] = perm[s];
    pos_slot_out[j] = pos_slot[s];
    env_pos_out[perm[s]] = j;
  }
  return RX_OK;
}
