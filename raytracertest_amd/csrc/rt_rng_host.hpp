// rt_rng_host.hpp -- host side of the XORWOW state creation.
//
// curand_init(seed, subsequence, 0) (call site RayTracer/Random.cu:22-27) = seed scramble
// + a jump of subsequence * 2^67 steps of the xorshift part.  The xorshift step is linear
// over GF(2) on 160 bits, so the jump is the matrix J = T^(2^67); we build J by 67
// squarings of the one-step matrix T and then J^(2^k), k = 0..31, which the device kernel
// multiplies together according to the bits of the pixel index.  Nothing is copied from
// cuRAND's precomputed tables (they are not available here); the matrices follow from the
// recurrence alone.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace rth {

struct Gf2Mat { uint32_t col[160][5]; };   // column i = image of basis vector e_i

inline void xorshift_step(uint32_t v[5]) {
  const uint32_t t = v[0] ^ (v[0] >> 2);
  v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = v[4];
  v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
}

inline void mat_vec(const Gf2Mat& A, const uint32_t x[5], uint32_t out[5]) {
  uint32_t r[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 160; ++i)
    if ((x[i >> 5] >> (i & 31)) & 1u)
      for (int w = 0; w < 5; ++w) r[w] ^= A.col[i][w];
  memcpy(out, r, sizeof r);
}

inline void mat_mul(const Gf2Mat& A, const Gf2Mat& B, Gf2Mat& out) {   // out = A * B
  Gf2Mat tmp;
  for (int i = 0; i < 160; ++i) mat_vec(A, B.col[i], tmp.col[i]);
  out = tmp;
}

// jump[k] = (T^(2^67))^(2^k), k = 0..31, as 160 columns padded to 8 words (device layout)
inline std::vector<uint32_t> build_jump_table() {
  Gf2Mat m;
  for (int i = 0; i < 160; ++i) {
    uint32_t v[5] = {0, 0, 0, 0, 0};
    v[i >> 5] = 1u << (i & 31);
    xorshift_step(v);
    memcpy(m.col[i], v, sizeof v);
  }
  for (int i = 0; i < 67; ++i) mat_mul(m, m, m);
  std::vector<uint32_t> table(32u * 160u * 8u, 0u);
  for (int k = 0; k < 32; ++k) {
    for (int i = 0; i < 160; ++i)
      memcpy(&table[(static_cast<size_t>(k) * 160u + i) * 8u], m.col[i], 5 * sizeof(uint32_t));
    mat_mul(m, m, m);
  }
  return table;
}

// 4-bit window tables of `matrices` matrices whose column i of matrix m starts at cols[(m * 160 + i) * col_stride] (5 words
// used): entry [m][g][n] = XOR of the columns g*4 + j of matrix m over the set bits j of the nibble n, so that a
// matrix-vector product is 40 table look-ups instead of 160 masked column XORs (the kernels keep the tables in LDS).
// Device layout: matrices*40*16 entries of words 0..3 (16 bytes each), then the same entries' word 4.
// rng_init_kernel: the six lowest jump powers J^(2^m), m = 0..5 (what distinguishes the 64 pixels of a wave);
// rng_settle_kernel: the one matrix T^n of the draws a tracer owes.
constexpr uint32_t kWindowMatrices = 6, kWindowGroups = 40, kWindowEntries = kWindowMatrices * kWindowGroups * 16u;
constexpr uint32_t kWindowEntriesOne = kWindowGroups * 16u;
inline std::vector<uint32_t> build_window_tables(const uint32_t* cols, size_t col_stride, uint32_t matrices) {
  const size_t entries = static_cast<size_t>(matrices) * kWindowGroups * 16u;
  std::vector<uint32_t> t(entries * 5u, 0u);
  for (uint32_t m = 0; m < matrices; ++m)
    for (uint32_t g = 0; g < kWindowGroups; ++g)
      for (uint32_t n = 0; n < 16u; ++n) {
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (uint32_t j = 0; j < 4u; ++j)
          if ((n >> j) & 1u)
            for (int w = 0; w < 5; ++w) r[w] ^= cols[(static_cast<size_t>(m) * 160u + g * 4u + j) * col_stride + w];
        const size_t e = (static_cast<size_t>(m) * kWindowGroups + g) * 16u + n;
        memcpy(&t[e * 4u], r, 4 * sizeof(uint32_t));
        t[entries * 4u + e] = r[4];
      }
  return t;
}
inline std::vector<uint32_t> build_window_tables(const std::vector<uint32_t>& jump) { return build_window_tables(jump.data(), 8u, kWindowMatrices); }
inline std::vector<uint32_t> build_window_table(const Gf2Mat& m) { return build_window_tables(&m.col[0][0], 5u, 1u); }

// out = M x through the window table of the one matrix M (what rng_settle_kernel does per lane)
inline void window_product(const std::vector<uint32_t>& table, const uint32_t x[5], uint32_t out[5]) {
  uint32_t r[5] = {0, 0, 0, 0, 0};
  for (uint32_t g = 0; g < kWindowGroups; ++g) {
    const uint32_t n = (x[g >> 3] >> ((g & 7u) * 4u)) & 15u;
    const size_t e = static_cast<size_t>(g) * 16u + n;
    for (int w = 0; w < 4; ++w) r[w] ^= table[e * 4u + w];
    r[4] ^= table[static_cast<size_t>(kWindowEntriesOne) * 4u + e];
  }
  memcpy(out, r, sizeof r);
}

// Advancing the xorshift words by n draws is the product by T^n (T: the one-step matrix).  T^(2^j), j < 32, are built once
// per process; T^n comes from them by square-and-multiply (all powers of T commute).
inline Gf2Mat identity_matrix() {
  Gf2Mat m;
  memset(&m, 0, sizeof m);
  for (int i = 0; i < 160; ++i) m.col[i][i >> 5] = 1u << (i & 31);
  return m;
}
inline const std::vector<Gf2Mat>& step_powers() {
  static const std::vector<Gf2Mat> powers = [] {
    std::vector<Gf2Mat> p(32);
    p[0] = identity_matrix();
    for (int i = 0; i < 160; ++i) xorshift_step(p[0].col[i]);
    for (int j = 1; j < 32; ++j) mat_mul(p[j - 1], p[j - 1], p[j]);
    return p;
  }();
  return powers;
}
inline Gf2Mat step_power(uint32_t n) {                          // T^n
  const std::vector<Gf2Mat>& p = step_powers();
  Gf2Mat r = identity_matrix();
  bool first = true;
  for (int j = 0; j < 32; ++j) {
    if (!((n >> j) & 1u)) continue;
    if (first) { r = p[j]; first = false; }
    else mat_mul(p[j], r, r);
  }
  return r;
}

// seed scramble of curand_init: state = {d, v0..v4}
inline void seed_state(uint64_t seed, uint32_t s[6]) {
  const uint32_t lo = static_cast<uint32_t>(seed) ^ 0xaad26b49u;
  const uint32_t hi = static_cast<uint32_t>(seed >> 32) ^ 0xf7dcefddu;
  const uint32_t t0 = 1099087573u * lo;
  const uint32_t t1 = 2591861531u * hi;
  s[0] = 6615241u + t1 + t0;
  s[1] = 123456789u + t0;
  s[2] = 362436069u ^ t0;
  s[3] = 521288629u + t1;
  s[4] = 88675123u ^ t1;
  s[5] = 5783321u + t0;
}

// host evaluation of curand_init(seed, subsequence, 0) from the same table (debug/tests)
inline void init_state(const std::vector<uint32_t>& table, uint64_t seed, uint64_t subsequence,
                       uint32_t s[6]) {
  seed_state(seed, s);
  for (int k = 0; k < 32; ++k) {
    if (!((subsequence >> k) & 1u)) continue;
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 160; ++i)
      if ((s[1 + (i >> 5)] >> (i & 31)) & 1u)
        for (int w = 0; w < 5; ++w) r[w] ^= table[(static_cast<size_t>(k) * 160u + i) * 8u + w];
    memcpy(s + 1, r, sizeof r);
  }
}

}  // namespace rth
