// PST_<X>_TIMES=1: stream events around the N phases of a call, read by tools/bench_*.py through pst_<x>_phase_times.  Every API file keeps
// its own thread_local double[N], its entry point and its own `static const bool ... = env_nonzero("PST_<X>_TIMES")` (env.hpp: read once per
// process, at that algorithm's first call); this is the create / mark / read / destroy around them.
#pragma once
#include "core.hpp"

namespace pst {

template <int N>
struct PhaseEvents {
  hipEvent_t e[N + 1] = {};
  const bool on;
  double* const ms;  // the caller's thread_local array: N entries
  PhaseEvents(bool wanted, double (&times)[N]) : on(wanted), ms(times) {
    if (on)
      for (auto& ev : e) PST_HIP_CHECK(hipEventCreate(&ev));
  }
  PhaseEvents(const PhaseEvents&) = delete;
  ~PhaseEvents() {
    for (auto ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
  void mark(int i, hipStream_t s) {
    if (on) PST_HIP_CHECK(hipEventRecord(e[i], s));
  }
  // event i for a launcher that records it itself (cluster_components' `gathered`); null when off
  hipEvent_t event(int i) const { return on ? e[i] : nullptr; }
  void read() {  // after the stream has been synchronised: the N differences, or N zeros when off
    for (int i = 0; i < N; ++i) {
      float t = 0.f;
      if (on) PST_HIP_CHECK(hipEventElapsedTime(&t, e[i], e[i + 1]));
      ms[i] = t;
    }
  }
};

}  // namespace pst
