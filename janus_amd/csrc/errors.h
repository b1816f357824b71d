// The error model's host side, free of HIP headers (common.h includes it): the exception
// type, JANUS_CHECK, the entry-point wrapper and the A/B environment switch.
#pragma once

#include <cstdlib>
#include <stdexcept>
#include <string>

namespace janus {

void set_error(const std::string& msg);

// Kernel-geometry A/B switches (JANUS_* environment variables) are read only by builds made
// with -DJANUS_AB_KNOBS (the A/B libraries the tools build beside the product); the product
// library takes no tuning from the environment and always runs the measured defaults.
inline const char* ab_env(const char* name) {
#ifdef JANUS_AB_KNOBS
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define JANUS_CHECK(cond, msg)                                                   \
  do {                                                                           \
    if (!(cond)) throw ::janus::Error(std::string(msg));                         \
  } while (0)

// Wrap an entry-point body: map exceptions to status codes.
template <class F>
inline int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    set_error(e.what());
    return 1;
  } catch (...) {
    set_error("unknown C++ exception");
    return 1;
  }
}

}  // namespace janus
