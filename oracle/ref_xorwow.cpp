// ref_xorwow.cpp -- the XORWOW step and skips behind oracle/ref_shim/curand_kernel.h, taken from rocRAND's host-callable
// rocrand_device::xorwow_engine of the ROCm installation, as tests/golden/make_rocrand_kats.cpp does.  TEST INFRASTRUCTURE.
// A translation unit of its own: rocRAND's headers include the HIP runtime's, whose float4, dim3 and blockIdx would
// collide with the stand-ins that the reference's text is compiled against.  State words: {d, x0..x4}.
#include <rocrand/rocrand_xorwow.h>

#include <cstdint>

namespace {
struct Engine : rocrand_device::xorwow_engine {
  explicit Engine(const uint32_t s[6]) {
    m_state.d = s[0];
    for (int i = 0; i < 5; ++i) m_state.x[i] = s[1 + i];
  }
  void store(uint32_t s[6]) const {
    s[0] = m_state.d;
    for (int i = 0; i < 5; ++i) s[1 + i] = m_state.x[i];
  }
};
}  // namespace

extern "C" uint32_t ref_xorwow_next(uint32_t s[6]) {
  Engine e(s);
  const uint32_t out = e.next();
  e.store(s);
  return out;
}

extern "C" void ref_xorwow_skip_subsequences(uint32_t s[6], uint64_t n) {
  Engine e(s);
  e.discard_subsequence(n);
  e.store(s);
}

extern "C" void ref_xorwow_skip(uint32_t s[6], uint64_t n) {
  Engine e(s);
  e.discard(n);
  e.store(s);
}
