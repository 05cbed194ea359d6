// launch_util.hpp -- what the host side of a kernel file needs around its launches: the check behind a launch, the
// grid arithmetic, and the cursor that lays a caller's workspace out.  A layout is written once, as a function over a
// Workspace: on a null base it only counts (the *_work_bytes functions), on d_work it hands the pointers out.
#ifndef ATR_LAUNCH_UTIL_HPP
#define ATR_LAUNCH_UTIL_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "atropos_hip.h"

namespace atr {

int hip_fail(hipError_t e, const char *what);             // api.hip

inline int launched(const char *what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ATR_OK : hip_fail(e, what);
}

inline long long blocks(long long n, long long per) { return (n + per - 1) / per; }
inline unsigned grid256(long long n) { return (unsigned)blocks(n, 256); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// arrays one behind the other, each on a 256-byte boundary of the base
class Workspace {
  public:
    explicit Workspace(const void *base) : base_((char *)base) {}
    template <typename T>
    T *take(size_t count) {
        T *p = base_ ? (T *)(base_ + used_) : nullptr;
        used_ += align256(count * sizeof(T));
        return p;
    }
    size_t bytes() const { return used_ + 256; }          // (256 spare bytes behind the last array, as ever)

  private:
    char *base_;
    size_t used_ = 0;
};

}  // namespace atr
#endif
