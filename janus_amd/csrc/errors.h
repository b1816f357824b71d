// The error model's host side, free of HIP headers (common.h includes it): the exception
// type, JANUS_CHECK and the entry-point wrapper.
#pragma once

#include <stdexcept>
#include <string>

namespace janus {

void set_error(const std::string& msg);

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
