// rt_hip_host.hpp -- host-side HIP helpers of the runtime: the failure type, HIP_CHECK, and owning handles of
// device memory, pinned host memory, events and streams.  The handles are move-only; their destructors release
// what they hold and never throw (a failure there has nobody to report to).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>

namespace rtr {

inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

struct HipFail { std::string what; };
// an argument the library refuses before it touches the device: RT_ERR_INVALID where HipFail is RT_ERR_HIP (guarded());
// every other handler takes it for the HipFail it derives from and keeps its text
struct BadArgument : HipFail { explicit BadArgument(std::string w) : HipFail{std::move(w)} {} };
#define HIP_CHECK(expr)                                                                                     \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) throw ::rtr::HipFail{::rtr::fmt("%s failed: %s", #expr, hipGetErrorString(e_))}; \
  } while (0)

// n elements of T in device memory (kPinned: page-locked host memory), grow-only
template <class T, bool kPinned = false>
class HipArray {
 public:
  HipArray() = default;
  explicit HipArray(size_t n) { ensure(n ? n : 1); }                   // (a zero-length request still gets a valid pointer)
  HipArray(HipArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  HipArray& operator=(HipArray&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
  ~HipArray() { reset(); }
  // room for at least n elements; growing frees the old buffer first (hipFree waits for the device) and drops its
  // contents.  true = (re)allocated
  bool ensure(size_t n) {
    if (n <= n_) return false;
    reset();
    if (kPinned) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), hipHostMallocDefault));
    else HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)));
    n_ = n;
    return true;
  }
  void reset() {
    if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <class T> using DevArray = HipArray<T, false>;
template <class T> using PinnedArray = HipArray<T, true>;

// an event or a stream; converts to the raw handle for the HIP calls
template <class H, hipError_t (*Release)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  HipHandle& operator=(HipHandle&& o) noexcept { std::swap(h_, o.h_); return *this; }
  ~HipHandle() { if (h_) (void)Release(h_); }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};

struct Event : HipHandle<hipEvent_t, hipEventDestroy> {
  Event() = default;
  explicit Event(unsigned flags) { HIP_CHECK(hipEventCreateWithFlags(&h_, flags)); }
  static Event timing() { Event e; HIP_CHECK(hipEventCreate(&e.h_)); return e; }
};

struct Stream : HipHandle<hipStream_t, hipStreamDestroy> {
  Stream() = default;
  explicit Stream(unsigned flags) { HIP_CHECK(hipStreamCreateWithFlags(&h_, flags)); }
  Stream(unsigned flags, int priority) { HIP_CHECK(hipStreamCreateWithPriority(&h_, flags, priority)); }
};

}  // namespace rtr
