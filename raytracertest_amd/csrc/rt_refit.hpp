// rt_refit.hpp -- refit of the ray queries' BVH on the device (RT_ACCEL_REFIT): a re-uploaded scene of the
// same size keeps the tree's topology and gets new boxes.  Three kernels, launched on one stream in this order; the order of
// the launches is the only synchronisation (no atomics, no device-scope fences):
//
//   refit_gather_kernel   one lane per record slot: the slot's upload index picks the triangle's 36 bytes out of the scene's
//                         arrays (tri_a[2i], tri_a[2i+1], tri_b[i]); a slot whose triangle changed its class -- a leaf's
//                         became non-finite, an always-tested one finite -- raises the flag (the host then builds instead)
//   refit_level_kernel    one launch per level, deepest first; lane = (node of the level, child), four lanes per node.  A leaf
//                         child: the union of its 1..4 triangles' boxes, each from corners in double rounded outward; an inner
//                         child: the union of the referenced node's four child boxes, which the launch before wrote
//   refit_cost_kernel     one block: the tree's cost, in a fixed summation order
//
// The arithmetic is rtb::refit's (rt_bvh_host.hpp) operation by operation, selects included, so that the device tree equals
// the host's refit bit for bit: min and max are compare-and-select in the host's operand order (they differ from v_min_f32 /
// v_max_f32 in the sign of a zero), the double additions are IEEE, the roundings to fp32 are round-to-nearest followed by one
// integer step outward.  Every reference read from the tree is checked against the tree's sizes before it is followed.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

constexpr uint32_t kRefitEmpty = 0xFFFFFFFFu;
constexpr uint32_t kRefitLeaf = 0x80000000u;
constexpr uint32_t kRefitCostThreads = 1024u;

// std::min(a, b) and std::max(a, b): the first operand unless the second is strictly better
template <class T> __device__ __forceinline__ T refit_min(T a, T b) { return b < a ? b : a; }
template <class T> __device__ __forceinline__ T refit_max(T a, T b) { return a < b ? b : a; }

__device__ __forceinline__ bool refit_finite(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7F800000u) != 0x7F800000u; }

// the next float below / above f (f is no NaN, and not the infinity of that direction)
__device__ __forceinline__ float refit_step_down(float f) {
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  return __builtin_bit_cast(float, (b << 1) == 0u ? 0x80000001u : (b >> 31) ? b + 1u : b - 1u);
}
__device__ __forceinline__ float refit_step_up(float f) {
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  return __builtin_bit_cast(float, (b << 1) == 0u ? 0x00000001u : (b >> 31) ? b - 1u : b + 1u);
}
// rtb::detail::round_down / round_up
__device__ __forceinline__ float refit_round_down(double x) {
  const float f = static_cast<float>(x);
  return static_cast<double>(f) > x ? refit_step_down(f) : f;
}
__device__ __forceinline__ float refit_round_up(double x) {
  const float f = static_cast<float>(x);
  return static_cast<double>(f) < x ? refit_step_up(f) : f;
}

struct RefitBox { float lox, loy, loz, hix, hiy, hiz; };

// one axis of rtb::detail::tri_box: the corners v0, v0 + e1, v0 + e2 in double, rounded outward
__device__ __forceinline__ void refit_axis(float v0f, float e1, float e2, float& lo, float& hi) {
  const double v0 = v0f, c1 = v0 + static_cast<double>(e1), c2 = v0 + static_cast<double>(e2);
  lo = refit_round_down(refit_min(v0, refit_min(c1, c2)));
  hi = refit_round_up(refit_max(v0, refit_max(c1, c2)));
}

// rtb::detail::tri_box of the record (e2.xyz, e1.x), (e1.yz, v0.xy), v0.z: its box, and whether the triangle is finite
__device__ __forceinline__ bool refit_tri_box(float4 a0, float4 a1, float v0z, RefitBox& b) {
  refit_axis(a1.z, a0.w, a0.x, b.lox, b.hix);
  refit_axis(a1.w, a1.x, a0.y, b.loy, b.hiy);
  refit_axis(v0z, a1.y, a0.z, b.loz, b.hiz);
  return refit_finite(a0.x) && refit_finite(a0.y) && refit_finite(a0.z) && refit_finite(a0.w) && refit_finite(a1.x) &&
         refit_finite(a1.y) && refit_finite(a1.z) && refit_finite(a1.w) && refit_finite(v0z) && refit_finite(b.lox) &&
         refit_finite(b.hix) && refit_finite(b.loy) && refit_finite(b.hiy) && refit_finite(b.loz) && refit_finite(b.hiz);
}

__device__ __forceinline__ void refit_grow(RefitBox& acc, const RefitBox& b) {
  acc.lox = refit_min(acc.lox, b.lox); acc.loy = refit_min(acc.loy, b.loy); acc.loz = refit_min(acc.loz, b.loz);
  acc.hix = refit_max(acc.hix, b.hix); acc.hiy = refit_max(acc.hiy, b.hiy); acc.hiz = refit_max(acc.hiz, b.hiz);
}

// rtb::detail::Box::half_area
__device__ __forceinline__ double refit_half_area(const RefitBox& b) {
  const double x = static_cast<double>(b.hix) - b.lox, y = static_cast<double>(b.hiy) - b.loy, z = static_cast<double>(b.hiz) - b.loz;
  return x * y + y * z + z * x;
}

// records: 3 float4 per slot, (e2.xyz, e1.x), (e1.yz, v0.xy), (v0.z, upload index, 0, 0).  The index and the pad stay.
__global__ __launch_bounds__(256) void refit_gather_kernel(const float4* __restrict__ tri_a, const float* __restrict__ tri_b, uint32_t n_tris,
                                                            float4* __restrict__ records, uint32_t n_leaf_records, uint32_t n_records,
                                                            uint32_t* __restrict__ flag) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_records) return;
  const uint32_t i = __builtin_bit_cast(uint32_t, records[3u * static_cast<size_t>(s) + 2u].y);
  if (i >= n_tris) { *flag = 1u; return; }                            // (not a tree of this scene: build instead)
  const float4 a0 = tri_a[2u * static_cast<size_t>(i)], a1 = tri_a[2u * static_cast<size_t>(i) + 1u];
  const float v0z = tri_b[i];
  records[3u * static_cast<size_t>(s)] = a0;
  records[3u * static_cast<size_t>(s) + 1u] = a1;
  records[3u * static_cast<size_t>(s) + 2u].x = v0z;
  RefitBox b;
  if (refit_tri_box(a0, a1, v0z, b) != (s < n_leaf_records)) *flag = 1u;
}

// nodes as floats, 32 per node: lo[axis][child] at 4 axis + child, hi at 12 + 4 axis + child, child[] (bits) at 24, cmax[] at 28
__global__ __launch_bounds__(256) void refit_level_kernel(float* __restrict__ nodes, uint32_t n_nodes, const float4* __restrict__ records,
                                                           uint32_t n_leaf_records, const uint32_t* __restrict__ level_nodes, uint32_t count) {
  const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
  if ((lane >> 2) >= count) return;
  const uint32_t node = level_nodes[lane >> 2], c = lane & 3u;
  if (node >= n_nodes) return;
  float* const nd = nodes + 32u * static_cast<size_t>(node);
  const uint32_t ref = __builtin_bit_cast(uint32_t, nd[24u + c]);
  if (ref == kRefitEmpty) return;                                     // keeps +inf, -inf, 0
  RefitBox acc = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (ref & kRefitLeaf) {
    const uint32_t first = ref & 0x0FFFFFFFu, n = ((ref >> 28) & 3u) + 1u;
    if (first + n > n_leaf_records) return;
    for (uint32_t j = first; j < first + n; ++j) {
      const float4 a0 = records[3u * static_cast<size_t>(j)], a1 = records[3u * static_cast<size_t>(j) + 1u];
      const float v0z = records[3u * static_cast<size_t>(j) + 2u].x;
      RefitBox b;
      (void)refit_tri_box(a0, a1, v0z, b);
      refit_grow(acc, b);
    }
  } else {
    if (ref >= n_nodes || ref <= node) return;                        // (children lie behind their parents)
    const float4* const ch = reinterpret_cast<const float4*>(nodes + 32u * static_cast<size_t>(ref));
    const float4 lx = ch[0], ly = ch[1], lz = ch[2], hx = ch[3], hy = ch[4], hz = ch[5];
    refit_grow(acc, {lx.x, ly.x, lz.x, hx.x, hy.x, hz.x});
    refit_grow(acc, {lx.y, ly.y, lz.y, hx.y, hy.y, hz.y});
    refit_grow(acc, {lx.z, ly.z, lz.z, hx.z, hy.z, hz.z});
    refit_grow(acc, {lx.w, ly.w, lz.w, hx.w, hy.w, hz.w});
  }
  float m = 0.0f;
  m = refit_max(m, refit_max(__builtin_fabsf(acc.lox), __builtin_fabsf(acc.hix)));
  m = refit_max(m, refit_max(__builtin_fabsf(acc.loy), __builtin_fabsf(acc.hiy)));
  m = refit_max(m, refit_max(__builtin_fabsf(acc.loz), __builtin_fabsf(acc.hiz)));
  nd[c] = acc.lox; nd[4u + c] = acc.loy; nd[8u + c] = acc.loz;
  nd[12u + c] = acc.hix; nd[16u + c] = acc.hiy; nd[20u + c] = acc.hiz;
  nd[28u + c] = m;
}

// rtb::tree_cost, one block of kRefitCostThreads lanes: lane = (node, child) strided over the tree, each lane's terms added in
// node order, the partial sums by a tree in LDS -- the value depends on the tree alone.  out[0] = the cost (0 when the union
// of the root's child boxes has no area).
__global__ __launch_bounds__(kRefitCostThreads) void refit_cost_kernel(const float* __restrict__ nodes, uint32_t n_nodes, double* __restrict__ out) {
  __shared__ double part[kRefitCostThreads];
  const uint32_t c = threadIdx.x & 3u;
  double sum = 0.0;
  for (uint32_t node = threadIdx.x >> 2; node < n_nodes; node += kRefitCostThreads / 4u) {
    const float* const nd = nodes + 32u * static_cast<size_t>(node);
    if (__builtin_bit_cast(uint32_t, nd[24u + c]) == kRefitEmpty) continue;
    sum += refit_half_area({nd[c], nd[4u + c], nd[8u + c], nd[12u + c], nd[16u + c], nd[20u + c]});
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t w = kRefitCostThreads / 2u; w != 0u; w >>= 1) {
    if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0u) return;
  double cost = 0.0;
  if (n_nodes != 0u) {
    RefitBox root = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const float4* const ch = reinterpret_cast<const float4*>(nodes);
    const float4 lx = ch[0], ly = ch[1], lz = ch[2], hx = ch[3], hy = ch[4], hz = ch[5];
    refit_grow(root, {lx.x, ly.x, lz.x, hx.x, hy.x, hz.x});
    refit_grow(root, {lx.y, ly.y, lz.y, hx.y, hy.y, hz.y});
    refit_grow(root, {lx.z, ly.z, lz.z, hx.z, hy.z, hz.z});
    refit_grow(root, {lx.w, ly.w, lz.w, hx.w, hy.w, hz.w});
    const double area = refit_half_area(root);
    if (area > 0.0) cost = part[0] / area;
  }
  out[0] = cost;
}

hipError_t launch_refit_gather(const float4* tri_a, const float* tri_b, uint32_t n_tris, float4* records, uint32_t n_leaf_records,
                               uint32_t n_records, uint32_t* flag, hipStream_t st) {
  if (n_records == 0u) return hipSuccess;
  if (tri_a == nullptr || tri_b == nullptr || records == nullptr || flag == nullptr || n_leaf_records > n_records) return hipErrorInvalidValue;
  hipLaunchKernelGGL(refit_gather_kernel, dim3((n_records + 255u) / 256u), dim3(256), 0, st, tri_a, tri_b, n_tris, records, n_leaf_records,
                     n_records, flag);
  return hipGetLastError();
}

hipError_t launch_refit_level(float4* nodes, uint32_t n_nodes, const float4* records, uint32_t n_leaf_records, const uint32_t* level_nodes,
                              uint32_t count, hipStream_t st) {
  if (count == 0u) return hipSuccess;
  if (nodes == nullptr || records == nullptr || level_nodes == nullptr || count > n_nodes) return hipErrorInvalidValue;
  const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(count) * 4u + 255u) / 256u);
  hipLaunchKernelGGL(refit_level_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<float*>(nodes), n_nodes, records, n_leaf_records,
                     level_nodes, count);
  return hipGetLastError();
}

hipError_t launch_refit_cost(const float4* nodes, uint32_t n_nodes, double* out, hipStream_t st) {
  if (out == nullptr || (n_nodes != 0u && nodes == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(refit_cost_kernel, dim3(1), dim3(kRefitCostThreads), 0, st, reinterpret_cast<const float*>(nodes), n_nodes, out);
  return hipGetLastError();
}

}  // namespace rtk
