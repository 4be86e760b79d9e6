// rt_sides.hpp -- the side of the nearest surface (rt_tracer_signed_distance*, rt_tracer_closest_sides*): a
// post-pass over the records rt_tracer_closest_point or rt_tracer_closest_all wrote.  Included by rt_kernels.hip only, behind
// rt_nearest.hpp.  The eight search kernels are not touched: the hit half of a signed answer IS the point query's answer.
//
// sides_kernel: 256-thread blocks, lane = record.  Record j belongs to point i = j / per_point.  The lane loads the point and
// the record (one 16-byte load each, the records coalesced), recomputes closest_triangle_feature on the triangle's record --
// the function the searches ran, on the same operands, so the same u, v, residual r = p - c and region -- gathers the ONE
// float4 at table[7 * prim + feature] (rt_features_host.hpp) and stores {s, feature} as one 8-byte store, with
//   s = (r.x*N.x + r.y*N.y) + r.z*N.z      (Math<false>::dot, every operation rounded separately)
// A sphere record (n_tris <= prim < n_tris + n_spheres): feature = 7, s = sqrt(w.w) - radius with closest_finish's operands.
// RT_PRIM_NONE -- the rows beyond a point's count hold it -- and any prim outside the scene: {0, -1}, nothing is read.
// s > 0: the front side; s < 0: the back side; s == 0: on the surface, or undecided.  No epsilon is applied.
#pragma once
#include "rt_nearest.hpp"

namespace rtk {

constexpr int kSideSphere = 7, kSideNone = -1;

__global__ __launch_bounds__(256) void sides_kernel(const TraceParams p, const float4* __restrict__ table, uint64_t n_records,
                                                     uint32_t per_point, const float4* __restrict__ pts,
                                                     const float4* __restrict__ hits, uint2* __restrict__ sides) {
  using M = Math<false>;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (j >= n_records) return;
  const float4 h = hits[j];
  const int prim = __float_as_int(h.w);
  float s = 0.0f;
  int feature = kSideNone;
  const uint32_t up = static_cast<uint32_t>(prim);                       // (a negative prim is beyond every scene)
  if (up < p.n_tris) {
    const float4 q = pts[per_point == 1u ? j : j / per_point];
    const float4 A0 = p.tri_a[2u * static_cast<size_t>(up)], A1 = p.tri_a[2u * static_cast<size_t>(up) + 1u];
    float t, u, v;
    V3 r;
    closest_triangle_feature({q.x, q.y, q.z}, {A1.z, A1.w, p.tri_b[up]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v, r, feature);
    const float4 N = table[7u * static_cast<size_t>(up) + static_cast<uint32_t>(feature)];
    s = M::dot(r, {N.x, N.y, N.z});
  } else if (prim >= 0 && up - p.n_tris < p.n_spheres) {
    const float4 q = pts[per_point == 1u ? j : j / per_point];
    const float4 sph = p.spheres[up - p.n_tris];
    const V3 w = rtd::sub({q.x, q.y, q.z}, {sph.x, sph.y, sph.z});
    s = __builtin_sqrtf(M::dot(w, w)) - sph.w;
    feature = kSideSphere;
  }
  sides[j] = make_uint2(__float_as_uint(s), static_cast<uint32_t>(feature));
}

// table: 7 float4 per triangle (may be nullptr for a scene without triangles); pts n x {x, y, z, d2max}; hits and sides
// n * per_point records; all 16-byte aligned but sides (8)
hipError_t launch_sides(const TraceParams& p, const float4* table, uint32_t n, uint32_t per_point, const float* pts, const float4* hits,
                        void* sides, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (per_point == 0u || per_point > kAllHitsMax || pts == nullptr || hits == nullptr || sides == nullptr) return hipErrorInvalidValue;
  if (p.n_tris != 0u && table == nullptr) return hipErrorInvalidValue;
  const uint64_t total = static_cast<uint64_t>(n) * per_point;
  const dim3 grid(static_cast<uint32_t>((total + 255u) / 256u));         // (at most 2^28 blocks)
  hipLaunchKernelGGL(sides_kernel, grid, dim3(256), 0, st, p, table, total, per_point, reinterpret_cast<const float4*>(pts), hits,
                     static_cast<uint2*>(sides));
  return hipGetLastError();
}

}  // namespace rtk
