// The one place that reads the environment: every SRHIP_* switch of the host
// code (api.cpp, jit.cpp, jit_grad.cpp, jit64.cpp) goes through these helpers.
// DESIGN.md "Environment switches" lists the switches. A helper reads the
// environment each time it is called; when a switch is read (once per process
// behind a `static const`, per program build, per call or launch) is decided
// where it is used.
#pragma once

#include <algorithm>
#include <cstdlib>

namespace srhip {

// the raw value, nullptr when unset (string- and list-valued switches)
inline const char* env_str(const char* name) { return std::getenv(name); }
// set to anything, the empty string included (the debug prints)
inline bool env_set(const char* name) { return env_str(name) != nullptr; }
// 0 or 1 as the value starts, else -1 (unset, empty, anything else)
inline int env_01(const char* name) {
  const char* e = env_str(name);
  return (e && e[0] == '0') ? 0 : (e && e[0] == '1') ? 1 : -1;
}
inline bool env_on(const char* name) { return env_01(name) != 0; }   // on unless it starts with 0
inline bool env_is1(const char* name) { return env_01(name) == 1; }  // on only if it starts with 1
// atoi of the value (0 for text that is no number), dflt when unset
inline int env_int(const char* name, int dflt) {
  const char* e = env_str(name);
  return e ? std::atoi(e) : dflt;
}
// the same clamped to [lo, hi]; dflt is returned as it is
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = env_str(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : dflt;
}
// atof of the value, dflt when unset
inline double env_double(const char* name, double dflt) {
  const char* e = env_str(name);
  return e ? std::atof(e) : dflt;
}

}  // namespace srhip
