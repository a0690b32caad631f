// Environment knobs of the kernel launchers, read one way.  Host-only, plain C++.  What a value
// MEANS (which values switch a path, clamps, ignored values) stays at the knob's call site.
#pragma once
#include <cstdlib>

namespace dtfx {

// integer value of the environment variable, `dflt` when it is unset
inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

// A knob that Python can force through a *_set_* binding: get() is the forced value when one is
// set (>= 0), otherwise the environment's.  The environment is read ONCE, at the first get() that
// needs it, also after a set(-1) (reset() is the exception): no test or tool changes a DTFX_*
// variable that C++ reads inside a running process (the ones they change are read in Python).
struct Knob {
  const char* name;
  int dflt;
  int forced = -1;  // < 0: none
  int env = 0;
  bool env_read = false;
  void set(int v) { forced = v; }
  // no forced value, and `v` in place of the environment's from now on (a setter whose -1 means
  // "the default", not "whatever the variable says")
  void reset(int v) {
    forced = -1;
    env = v;
    env_read = true;
  }
  int get() {
    if (forced >= 0) return forced;
    if (!env_read) {
      env = env_int(name, dflt);
      env_read = true;
    }
    return env;
  }
};

}  // namespace dtfx
