// rt_trioverlap.hpp -- the triangle-shaped region query (rt_tracer_overlap_triangles*): the primitives of the
// tracer's scene that touch query triangle i, the max_hits lowest of them in ascending prim order behind an optional cursor, and
// the total number of them.  Included by rt_kernels.hip only, behind rt_overlap.hpp, whose list (OverlapList<CAP>), cursor
// (overlap_cursor, overlap_behind), box-axis comparison (overlap_axis1) and kernels (region_kernel, region_bvh_kernel) are used as
// they are: this file states the rule, as the shape TriRegion.
//
// Acceptance is a pure function of (query, record, cursor), the text of include/rt_mi355x.h operation by operation: ONE
// arithmetic, every operation rounded separately (the library is compiled with -ffp-contract=off).  On the record the renderer
// intersects, A = v0, B = fl(v0 + e1), C = fl(v0 + e2), against the query P0, P1, P2:
//   step 1 (TriRegion::step1) the query finite, neither B nor C a NaN, per axis min(A, B, C) <= max(P) and max(A, B, C) >= min(P)
//   step 2                   a = A - P0, b = B - P0, c = C - P0, p1 = P1 - P0, p2 = P2 - P0; the query's own corner is 0
//   step 3 (separated)       17 axes: n = e1 x e2, m = p1 x p2, the nine f_i x g_j, the three n x f_i, the three m x g_j of
//                            f = e1, c - b, a - c and g = p1, p2 - p1, p2.  ALL six points are projected on every axis: a
//                            corner shared bit for bit projects identically on both sides, so no axis separates the pair.
// An axis separates when every record projection is > every query projection, or every one is <; a NaN projection makes its
// comparisons false and never separates.  tri_axis takes min3 / max3 of each side and masks the verdict with "no projection
// is a NaN": the same verdicts as the nine plus nine comparisons, since without a NaN min3 / max3 are exact.
// A sphere is its surface (TriRegion::sphere): closest_triangle's t from the centre to the query's own record against r*r, and the
// farthest query corner.
//
// Why the tree prunes exactly, with no slack: the argument of rt_overlap.hpp with the query triangle's bounding box in the place
// of the caller's box.  Step 1's record interval lies inside rtb::detail::tri_box; a child is entered when its box and the
// query's bounding box overlap under the same closed comparisons.  b.rho is not read.
//
// The query is three 16-byte loads.  The axes are evaluated in groups of three (one f against the three g) so that no more than a
// group's projections are live at once: 0 B of scratch in all six kernels.  The tree kernels ask for 4 waves per SIMD
// (kTreeWaves): left alone, the max-ILP scheduler interleaves the seventeen axes of the three inlined record tests up to 242
// VGPRs (2 waves); bounded it stays at 90 - 107 VGPRs with 0 B of scratch (a few SGPRs are kept in VGPR lanes).
#pragma once
#include "rt_overlap.hpp"

namespace rtk {

// the query triangle as the rule reads it (the pads are dropped here)
struct TriQuery {
  V3 P0, P1, P2;      // the corners as given (the sphere rule's farthest corner)
  V3 p1, p2;          // moved by -P0
  V3 lo, hi;          // the bounding box: minNum / maxNum of the corners
  bool valid;         // all nine coordinates finite
};

__device__ __forceinline__ bool tri_finite(float4 v) {
  const float inf = __builtin_inff();
  const bool x = fabsf(v.x) < inf, y = fabsf(v.y) < inf, z = fabsf(v.z) < inf;   // false on a NaN
  return x & y & z;
}

__device__ __forceinline__ TriQuery tri_query(float4 q0, float4 q1, float4 q2) {
  TriQuery q;
  q.P0 = {q0.x, q0.y, q0.z};
  q.P1 = {q1.x, q1.y, q1.z};
  q.P2 = {q2.x, q2.y, q2.z};
  q.p1 = rtd::sub(q.P1, q.P0);
  q.p2 = rtd::sub(q.P2, q.P0);
  q.lo = {fminf(fminf(q0.x, q1.x), q2.x), fminf(fminf(q0.y, q1.y), q2.y), fminf(fminf(q0.z, q1.z), q2.z)};
  q.hi = {fmaxf(fmaxf(q0.x, q1.x), q2.x), fmaxf(fmaxf(q0.y, q1.y), q2.y), fmaxf(fmaxf(q0.z, q1.z), q2.z)};
  const bool f0 = tri_finite(q0), f1 = tri_finite(q1), f2 = tri_finite(q2);
  q.valid = f0 & f1 & f2;
  return q;
}

// one axis x: the record projects to x.a, x.b, x.c, the query to 0, x.p1, x.p2
__device__ __forceinline__ bool tri_axis(V3 x, V3 a, V3 b, V3 c, V3 p1, V3 p2) {
  using M = Math<false>;
  const float ra = M::dot(x, a), rb = M::dot(x, b), rc = M::dot(x, c), q1 = M::dot(x, p1), q2 = M::dot(x, p2);
  const float rmin = fminf(fminf(ra, rb), rc), rmax = fmaxf(fmaxf(ra, rb), rc);
  const float qmin = fminf(fminf(q1, q2), 0.0f), qmax = fmaxf(fmaxf(q1, q2), 0.0f);
  const bool nan0 = __builtin_isunordered(ra, rb), nan1 = __builtin_isunordered(rc, q1), nan2 = __builtin_isunordered(q2, q2);
  const bool above = rmin > qmax, below = rmax < qmin;
  return !(nan0 | nan1 | nan2) & (above | below);
}

// the three axes f x g_j of one record edge vector f
__device__ __forceinline__ bool tri_axes3(V3 f, V3 g0, V3 g1, V3 g2, V3 a, V3 b, V3 c, V3 p1, V3 p2) {
  using M = Math<false>;
  const bool s0 = tri_axis(M::cross(f, g0), a, b, c, p1, p2);
  const bool s1 = tri_axis(M::cross(f, g1), a, b, c, p1, p2);
  const bool s2 = tri_axis(M::cross(f, g2), a, b, c, p1, p2);
  return s0 | s1 | s2;
}

// The triangle as a region shape (rt_overlap.hpp's skeleton).
struct TriRegion {
  static constexpr int kFloat4s = 3;
  static constexpr int kScanWaves = 4, kTreeWaves = 4;
  using Query = TriQuery;
  using SphereCtx = NoSphereCtx;
  static constexpr bool kSphereCtx = false;

  __device__ static __forceinline__ void load(Query& q, const float4* tris, size_t base, uint32_t lane, bool live) {
    const float inf = __builtin_inff();
    float4 q0 = {inf, inf, inf, 0.0f}, q1 = q0, q2 = q0;                  // padding lanes: a non-finite query accepts nothing
    if (live) { q0 = tris[3u * (base + lane)]; q1 = tris[3u * (base + lane) + 1u]; q2 = tris[3u * (base + lane) + 2u]; }
    q = tri_query(q0, q1, q2);
  }
  __device__ static __forceinline__ SphereCtx sphere_ctx(const float4*, size_t, uint32_t) { return {}; }

  // step 1: BoxRegion::step1's comparisons against the query's bounding box
  __device__ static __forceinline__ bool step1(const Query& q, V3 A, V3 B, V3 C) {
    const bool x = overlap_axis1(A.x, B.x, C.x, q.lo.x, q.hi.x), y = overlap_axis1(A.y, B.y, C.y, q.lo.y, q.hi.y);
    const bool z = overlap_axis1(A.z, B.z, C.z, q.lo.z, q.hi.z);
    return q.valid & x & y & z;
  }

  // steps 2 and 3: true when one of the seventeen axes separates the record from the query
  __device__ static __forceinline__ bool separated(const Query& q, V3 A, V3 B, V3 C, V3 e1, V3 e2) {
    using M = Math<false>;
    const V3 a = rtd::sub(A, q.P0), b = rtd::sub(B, q.P0), c = rtd::sub(C, q.P0);
    const V3 f0 = e1, f1 = rtd::sub(c, b), f2 = rtd::sub(a, c);
    const V3 g0 = q.p1, g1 = rtd::sub(q.p2, q.p1), g2 = q.p2;
    const V3 n = M::cross(e1, e2), m = M::cross(q.p1, q.p2);
    const bool sn = tri_axis(n, a, b, c, q.p1, q.p2), sm = tri_axis(m, a, b, c, q.p1, q.p2);
    const bool s0 = tri_axes3(f0, g0, g1, g2, a, b, c, q.p1, q.p2);
    const bool s1 = tri_axes3(f1, g0, g1, g2, a, b, c, q.p1, q.p2);
    const bool s2 = tri_axes3(f2, g0, g1, g2, a, b, c, q.p1, q.p2);
    const bool s3 = tri_axes3(n, f0, f1, f2, a, b, c, q.p1, q.p2);   // the in-plane axes of the record
    const bool s4 = tri_axes3(m, g0, g1, g2, a, b, c, q.p1, q.p2);   // and of the query
    return sn | sm | s0 | s1 | s2 | s3 | s4;
  }

  // the sphere rule: the surface touches the triangle when its nearest point is inside the ball and its farthest corner is not
  __device__ static __forceinline__ bool sphere(const Query& q, SphereCtx, float4 sph) {
    using M = Math<false>;
    const V3 C = {sph.x, sph.y, sph.z};
    float d2min, u, v;
    closest_triangle(C, q.P0, q.p1, q.p2, d2min, u, v);
    const V3 w0 = rtd::sub(q.P0, C), w1 = rtd::sub(q.P1, C), w2 = rtd::sub(q.P2, C);
    const float d2max = fmaxf(fmaxf(M::dot(w0, w0), M::dot(w1, w1)), M::dot(w2, w2));
    const float rr = sph.w * sph.w;
    const bool inside = d2min <= rr, reaches = rr <= d2max;
    return q.valid & inside & reaches;
  }
};

hipError_t launch_overlap_triangles(const TraceParams& p, const BvhParams* b, uint32_t n, const float* tris, const int* after,
                                    uint32_t max_hits, int* prims, uint32_t* counts, hipStream_t st) {
  return launch_region<TriRegion>(p, b, n, tris, after, max_hits, prims, counts, st);
}

}  // namespace rtk
