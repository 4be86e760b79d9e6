/* curand_kernel.h -- stand-in for the three cuRAND device functions the reference calls (Random.cu:24-27,
 * Random.cuh:15-16,23): curand_init, curand_uniform on a curandState_t (XORWOW, cuRAND's default generator).
 *
 * TEST INFRASTRUCTURE (see oracle/ref_driver.cpp).  Where each piece comes from:
 *   - the xorshift + Weyl step and the skip by subsequences of 2^67 outputs: rocRAND's host-callable
 *     rocrand_device::xorwow_engine, with AMD's precomputed jump matrices (oracle/ref_xorwow.cpp, a translation unit of
 *     its own because rocRAND's headers pull in the HIP runtime's float4, dim3 and blockIdx);
 *   - the seeding and the uint -> float mapping, which rocRAND does differently: stated below from the published
 *     curand_kernel.h of the CUDA Toolkit (11.7 is what the reference builds with, RayTracer/RayTracer.vcxproj:32).
 */
#pragma once

#include <cstdint>

/* {d, v[0..4]}: the words of curandStateXORWOW that the three functions read or write (the Box-Muller leftovers that
 * follow them in cuRAND's struct are never touched by curand_uniform).  The same layout as the project's RNG states. */
struct curandState_t {
  uint32_t d;
  uint32_t v[5];
};

extern "C" {
uint32_t ref_xorwow_next(uint32_t s[6]);                          /* rocRAND: xorwow_engine::next()                 */
void ref_xorwow_skip_subsequences(uint32_t s[6], uint64_t n);     /* rocRAND: xorwow_engine::discard_subsequence(n) */
void ref_xorwow_skip(uint32_t s[6], uint64_t n);                  /* rocRAND: xorwow_engine::discard(n)             */
}

/* curand_init(seed, subsequence, offset, state), curand_kernel.h (_curand_init_scratch + skipahead_sequence +
 * skipahead): the seed's two halves are salted with 0xaad26b49 and 0xf7dcefdd, multiplied by 1099087573 and 2591861531,
 * and added / xor-ed onto Marsaglia's xorwow constants 123456789, 362436069, 521288629, 88675123, 5783321 and 6615241;
 * then the state skips `subsequence` times 2^67 outputs and `offset` outputs. */
inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandState_t* state) {
  const uint32_t s0 = static_cast<uint32_t>(seed) ^ 0xaad26b49u;
  const uint32_t s1 = static_cast<uint32_t>(seed >> 32) ^ 0xf7dcefddu;
  const uint32_t t0 = 1099087573u * s0;
  const uint32_t t1 = 2591861531u * s1;
  state->d = 6615241u + t1 + t0;
  state->v[0] = 123456789u + t0;
  state->v[1] = 362436069u ^ t0;
  state->v[2] = 521288629u + t1;
  state->v[3] = 88675123u ^ t1;
  state->v[4] = 5783321u + t0;
  uint32_t* w = &state->d;
  static_assert(sizeof(curandState_t) == 6 * sizeof(uint32_t), "state words are contiguous");
  ref_xorwow_skip_subsequences(w, subsequence);
  ref_xorwow_skip(w, offset);
}

inline unsigned int curand(curandState_t* state) { return ref_xorwow_next(&state->d); }

/* curand_uniform, curand_uniform.h: _curand_uniform(x) = x * CURAND_2POW32_INV + (CURAND_2POW32_INV / 2.0f) with
 * CURAND_2POW32_INV = 2.3283064e-10f: x converted to float, one product and one sum, a value in (0, 1]. */
inline float curand_uniform(curandState_t* state) {
  const unsigned int x = curand(state);
  return x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}
