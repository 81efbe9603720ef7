// rx_track_evolve_host.cpp -- the host twins of the track-evolution kernels
// (rx_track_evolve_plan_host / rx_track_evolve_host and the in-place form's
// rx_track_evolve_classes_host / _inplace_host / _commit_host, ABI v25 additive): the loops of
// rx_track_evolve.hip one slot at a time over the same rx_track_evolve.h functions.
// Compiled as plain C++ (not as HIP); rx_api_curriculum.cpp checks the arguments before it
// calls in here.  No HIP call.
#include "rx.h"
#include "rx_track_evolve.h"

extern "C" void rx_host_track_evolve_plan(const rx_track_evolve_io* ev, uint32_t generation, double edit_frac) {
  for (int32_t j = 0; j < ev->n_spawn; ++j) rx_te_plan_row(ev, generation, edit_frac, j);
}

extern "C" void rx_host_track_evolve(const rx_track_evolve_io* ev, uint32_t generation) {
  for (int32_t k = 0; k < ev->n_tracks; ++k) rx_te_slot(ev, generation, k);
}

// the in-place form: the class table, the staging buffer, the commit
extern "C" void rx_host_track_evolve_classes(const rx_track_evolve_inplace_io* ev) { rx_te_classes_serial(ev); }

extern "C" void rx_host_track_evolve_inplace(const rx_track_evolve_inplace_io* ev, uint32_t generation,
                                             double edit_frac) {
  for (int32_t j = 0; j < ev->n_spawn; ++j) rx_te_inplace_slot(ev, generation, edit_frac, j);
}

extern "C" void rx_host_track_evolve_commit(const rx_track_evolve_inplace_io* ev) {
  for (int32_t j = 0; j < ev->n_spawn; ++j) rx_te_commit_slot(ev, j);
}
