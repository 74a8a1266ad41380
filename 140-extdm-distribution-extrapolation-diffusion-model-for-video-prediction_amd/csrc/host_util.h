// Host-side pieces every runtime (runtime.cpp, fvd.cpp) and launcher shares: the error type and
// its checks, the C ABI's exception guard, and the environment switch rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <stdexcept>
#include <string>

namespace extdm {

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      throw ::extdm::Error(std::string(#x) + " failed: " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
  } while (0)

#define REQUIRE(c, msg) \
  do { if (!(c)) throw ::extdm::Error(msg); } while (0)

// the thread's extdm_last_error message (runtime.cpp)
void set_last_error(const std::string& msg);

// A C ABI entry point's body: 0, or -1 with the exception's message as extdm_last_error
template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

// An environment switch is on when it is set, non-empty and does not start with '0'
inline bool env_flag(const char* name) {
  const char* v = getenv(name);
  return v && v[0] && v[0] != '0';
}

}  // namespace extdm
