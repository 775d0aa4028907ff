// The one place that reads environment switches (host only: plain C++, no HIP, never part of the run-time-compiled headers).
// A call site keeps its value in a `static const`, so a switch is read once per process; std::getenv is not thread-safe against setenv.
#pragma once
#include <cstdlib>

namespace pst {

inline const char* env_str(const char* name) { return std::getenv(name); }  // null when unset: for the few switches that are not one of the forms below

// on unless the value starts with '0' (unset and empty: on) -- the form of the A/B switches
inline bool env_on(const char* name) {
  const char* v = env_str(name);
  return !(v && *v == '0');
}
// set, not empty, and not starting with '0'
inline bool env_nonzero(const char* name) {
  const char* v = env_str(name);
  return v && *v && *v != '0';
}
// the value as a decimal number; `dflt` when unset or empty
inline long env_long(const char* name, long dflt) {
  const char* v = env_str(name);
  return v && *v ? std::strtol(v, nullptr, 10) : dflt;
}

}  // namespace pst
