// common.h -- shared host-side helpers for liblic360_hip (error reporting, owners of HIP resources, launch geometry).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdarg>
#include <algorithm>
#include <utility>
#include "../../include/lic360_hip.h"

#define LIC360_API extern "C" __attribute__((visibility("default")))

void lic360_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            lic360_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

#define LAUNCH_CHECK()                                                                       \
    do {                                                                                     \
        hipError_t _e = hipGetLastError();                                                   \
        if (_e != hipSuccess) {                                                              \
            lic360_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

#define ARG_CHECK(cond)                                                                      \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            lic360_set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__);         \
            return 2;                                                                        \
        }                                                                                    \
    } while (0)

// Move-only owners of one HIP resource each: DevBuf (hipMalloc), PinnedBuf (mapped, host-coherent hipHostMalloc), HipEvent.  alloc / create
// report a failure as HIP_TRY does and replace what the owner held only on success; the implicit conversion keeps launch sites and pointer
// arithmetic as they were on raw pointers.
template <class T, bool PINNED>
class HipBuf {
  public:
    HipBuf() = default;
    HipBuf(HipBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    HipBuf &operator=(HipBuf o) noexcept { std::swap(p_, o.p_); return *this; }
    ~HipBuf() {
        if (!p_) return;
        if constexpr (PINNED) (void)hipHostFree(p_);
        else (void)hipFree(p_);
    }
    int alloc(size_t n) {                      // at least one element
        HipBuf b;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if constexpr (PINNED) HIP_TRY(hipHostMalloc((void **)&b.p_, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        else HIP_TRY(hipMalloc((void **)&b.p_, bytes));
        *this = std::move(b);
        return 0;
    }
    operator T *() const { return p_; }
  private:
    T *p_ = nullptr;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

class HipEvent {
  public:
    HipEvent() = default;
    HipEvent(HipEvent &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    HipEvent &operator=(HipEvent o) noexcept { std::swap(e_, o.e_); return *this; }
    ~HipEvent() { if (e_) (void)hipEventDestroy(e_); }
    int create(unsigned flags) {
        HipEvent e;
        HIP_TRY(hipEventCreateWithFlags(&e.e_, flags));
        *this = std::move(e);
        return 0;
    }
    operator hipEvent_t() const { return e_; }
  private:
    hipEvent_t e_ = nullptr;
};

// 1-D streaming launches: 256 threads/block; enough blocks to cover `n` items at `per_thread`
// each, capped so that grid-stride loops keep >= 8 waves per CU resident (256 CUs).
static inline unsigned lic360_blocks(long n, int per_thread = 1) {
    long b = (n + 256L * per_thread - 1) / (256L * per_thread);
    if (b < 1) b = 1;
    if (b > 256L * 32) b = 256L * 32;
    return (unsigned)b;
}
