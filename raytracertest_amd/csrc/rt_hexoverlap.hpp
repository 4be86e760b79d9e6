// rt_hexoverlap.hpp -- the hexahedron-shaped region query (rt_tracer_overlap_hexahedra*): the primitives of the
// tracer's scene that touch the convex hull of eight corners in a box-like order (an oriented or sheared box, a frustum, a
// pyramid, a wedge, a segment), the max_hits lowest of them in ascending prim order behind an optional cursor, and the total
// number of them.  Included by rt_kernels.hip only, behind rt_trioverlap.hpp, whose query check (tri_finite) is used as it is, as
// are rt_overlap.hpp's list (OverlapList<CAP>), cursor (overlap_cursor, overlap_behind), box-axis comparison (overlap_axis1) and
// kernels (region_kernel, region_bvh_kernel): this file states the rule, as the shape HexRegion.
//
// Acceptance is a pure function of (corners, record, cursor), the text of include/rt_mi355x.h operation by operation: ONE
// arithmetic, every operation rounded separately (the library is compiled with -ffp-contract=off).  On the record the renderer
// intersects, A = v0, B = fl(v0 + e1), C = fl(v0 + e2), against the corners C0 .. C7 (bit 0 of k = the side along the region's
// first direction, bit 1 the second, bit 2 the third):
//   step 1 (HexRegion::step1) all 24 coordinates finite, neither B nor C a NaN, per axis min(A, B, C) <= max_k C_k and
//                            max(A, B, C) >= min_k C_k
//   step 2                   a = A - C0, b = B - C0, c = C - C0, h_k = C_k - C0; the region's own corner 0 is the literal 0
//   step 3 (separated)       43 axes: n = e1 x e2; the six face normals (h_d - h_a) x (h_c - h_b), the cross product of a face's
//                            two diagonals; the 36 crosses f_i x g_e of f = e1, c - b, a - c and the twelve edges g_e = h_j - h_i
// On an axis x the record projects to x.a, x.b, x.c and the region to 0, x.h_1 .. x.h_7; it separates when the record's minimum
// is > the region's maximum or its maximum < the region's minimum, and no projection is a NaN (hex_axis masks the verdict as
// tri_axis does).  The region's own projections on its six face normals do not depend on the record: hex_query computes them
// once (HexQuery::fmn, fmx; a NaN among them is kept as the interval [-inf, +inf], which separates nothing: the same verdicts).
// A sphere is its surface (HexRegion::sphere): inside the six face slabs or closest_triangle's t to the twelve face triangles against
// r*r, and the farthest corner.
//
// Why the tree prunes exactly, with no slack: the argument of rt_overlap.hpp with the region's bounding box in the place of the
// caller's box.  Step 1's record interval lies inside rtb::detail::tri_box; a child is entered when its box and the region's
// bounding box overlap under the same closed comparisons.  b.rho is not read.
//
// The query is eight 16-byte loads.  Corners and list slots sit behind compile-time indices only; the edge axes are evaluated in groups of three
// (one g_e against the three f), every axis a block of its own.  The corners as given are needed by the sphere rule alone and
// are loaded again for it, so the triangle loop does not carry them.  All six kernels are bounded to RT_HEX_WAVES = 4 waves per
// SIMD: 128 VGPRs and 52 - 152 B of scratch (12 - 139 registers spilled), which measured 1.2 - 1.6 times faster than the 196 -
// 233 VGPRs and 0 B of scratch of a bound of 2; the macro is there so that the bound can be measured again
// (make EXTRA=-DRT_HEX_WAVES=2).
#pragma once
#include "rt_trioverlap.hpp"

#ifndef RT_HEX_WAVES
#define RT_HEX_WAVES 4
#endif
namespace rtk {

// the region as the triangle rule reads it (the pads are dropped here)
struct HexQuery {
  V3 C0;              // corner 0 as given
  V3 h[8];            // the corners moved by -C0; h[0] is not used (the literal 0)
  V3 lo, hi;          // the bounding box: minNum / maxNum of the corners
  V3 fn[6];           // the face normals
  float fmn[6], fmx[6];   // the region's own projections on them: min and max over 0, fn.h_1 .. fn.h_7
  bool valid;         // all 24 coordinates finite
};

__device__ __forceinline__ float hex_min8(float a, float b, float c, float d, float e, float f, float g, float h) {
  return fminf(fminf(fminf(fminf(fminf(fminf(fminf(a, b), c), d), e), f), g), h);
}
__device__ __forceinline__ float hex_max8(float a, float b, float c, float d, float e, float f, float g, float h) {
  return fmaxf(fmaxf(fmaxf(fmaxf(fmaxf(fmaxf(fmaxf(a, b), c), d), e), f), g), h);
}

// the region's projections on an axis x: min and max over 0, x.h_1 .. x.h_7, and whether one of them is a NaN
__device__ __forceinline__ bool hex_project(const HexQuery& q, V3 x, float& qmin, float& qmax) {
  using M = Math<false>;
  const float q1 = M::dot(x, q.h[1]), q2 = M::dot(x, q.h[2]), q3 = M::dot(x, q.h[3]), q4 = M::dot(x, q.h[4]);
  const float q5 = M::dot(x, q.h[5]), q6 = M::dot(x, q.h[6]), q7 = M::dot(x, q.h[7]);
  qmin = hex_min8(q1, q2, q3, q4, q5, q6, q7, 0.0f);
  qmax = hex_max8(q1, q2, q3, q4, q5, q6, q7, 0.0f);
  const bool n0 = __builtin_isunordered(q1, q2), n1 = __builtin_isunordered(q3, q4), n2 = __builtin_isunordered(q5, q6);
  return n0 | n1 | n2 | __builtin_isunordered(q7, q7);
}

// the normal of the face (a, b, c, d): the cross product of its diagonals a-d and b-c, and the region's projections on it
__device__ __forceinline__ void hex_face(HexQuery& q, int f, V3 da, V3 db) {
  const float inf = __builtin_inff();
  q.fn[f] = Math<false>::cross(da, db);
  float mn, mx;
  const bool nan = hex_project(q, q.fn[f], mn, mx);
  q.fmn[f] = nan ? -inf : mn;
  q.fmx[f] = nan ? inf : mx;
}

__device__ __forceinline__ HexQuery hex_query(float4 c0, float4 c1, float4 c2, float4 c3, float4 c4, float4 c5, float4 c6, float4 c7) {
  HexQuery q;
  q.C0 = {c0.x, c0.y, c0.z};
  q.h[0] = {0.0f, 0.0f, 0.0f};
  q.h[1] = rtd::sub({c1.x, c1.y, c1.z}, q.C0);
  q.h[2] = rtd::sub({c2.x, c2.y, c2.z}, q.C0);
  q.h[3] = rtd::sub({c3.x, c3.y, c3.z}, q.C0);
  q.h[4] = rtd::sub({c4.x, c4.y, c4.z}, q.C0);
  q.h[5] = rtd::sub({c5.x, c5.y, c5.z}, q.C0);
  q.h[6] = rtd::sub({c6.x, c6.y, c6.z}, q.C0);
  q.h[7] = rtd::sub({c7.x, c7.y, c7.z}, q.C0);
  q.lo = {hex_min8(c0.x, c1.x, c2.x, c3.x, c4.x, c5.x, c6.x, c7.x), hex_min8(c0.y, c1.y, c2.y, c3.y, c4.y, c5.y, c6.y, c7.y),
          hex_min8(c0.z, c1.z, c2.z, c3.z, c4.z, c5.z, c6.z, c7.z)};
  q.hi = {hex_max8(c0.x, c1.x, c2.x, c3.x, c4.x, c5.x, c6.x, c7.x), hex_max8(c0.y, c1.y, c2.y, c3.y, c4.y, c5.y, c6.y, c7.y),
          hex_max8(c0.z, c1.z, c2.z, c3.z, c4.z, c5.z, c6.z, c7.z)};
  const bool f0 = tri_finite(c0), f1 = tri_finite(c1), f2 = tri_finite(c2), f3 = tri_finite(c3);
  const bool f4 = tri_finite(c4), f5 = tri_finite(c5), f6 = tri_finite(c6), f7 = tri_finite(c7);
  q.valid = f0 & f1 & f2 & f3 & f4 & f5 & f6 & f7;
  // the faces (a, b, c, d): (0,2,4,6), (1,3,5,7), (0,1,4,5), (2,3,6,7), (0,1,2,3), (4,5,6,7); h_0 is the literal 0
  hex_face(q, 0, q.h[6], rtd::sub(q.h[4], q.h[2]));
  hex_face(q, 1, rtd::sub(q.h[7], q.h[1]), rtd::sub(q.h[5], q.h[3]));
  hex_face(q, 2, q.h[5], rtd::sub(q.h[4], q.h[1]));
  hex_face(q, 3, rtd::sub(q.h[7], q.h[2]), rtd::sub(q.h[6], q.h[3]));
  hex_face(q, 4, q.h[3], rtd::sub(q.h[2], q.h[1]));
  hex_face(q, 5, rtd::sub(q.h[7], q.h[4]), rtd::sub(q.h[6], q.h[5]));
  return q;
}

// the record's side of one axis against a region interval [qmin, qmax] that holds no NaN
__device__ __forceinline__ bool hex_record_axis(V3 x, V3 a, V3 b, V3 c, float qmin, float qmax) {
  using M = Math<false>;
  const float ra = M::dot(x, a), rb = M::dot(x, b), rc = M::dot(x, c);
  const float rmin = fminf(fminf(ra, rb), rc), rmax = fmaxf(fmaxf(ra, rb), rc);
  const bool nan0 = __builtin_isunordered(ra, rb), nan1 = __builtin_isunordered(rc, rc);
  const bool above = rmin > qmax, below = rmax < qmin;
  return !(nan0 | nan1) & (above | below);
}

// one axis x: the record projects to x.a, x.b, x.c, the region to 0, x.h_1 .. x.h_7
__device__ __forceinline__ bool hex_axis(const HexQuery& q, V3 x, V3 a, V3 b, V3 c) {
  float qmin, qmax;
  const bool nan = hex_project(q, x, qmin, qmax);
  return !nan & hex_record_axis(x, a, b, c, qmin, qmax);
}

// the three axes f_i x g of one region edge g; an axis that separates ends the test for its lane
__device__ __forceinline__ bool hex_axes3(const HexQuery& q, V3 g, V3 f0, V3 f1, V3 f2, V3 a, V3 b, V3 c) {
  using M = Math<false>;
  if (hex_axis(q, M::cross(f0, g), a, b, c)) return true;
  if (hex_axis(q, M::cross(f1, g), a, b, c)) return true;
  return hex_axis(q, M::cross(f2, g), a, b, c);
}

// the corners as given, for the sphere rule
struct HexCorners {
  V3 C[8];
};

__device__ __forceinline__ HexCorners hex_corners(const float4* __restrict__ hexa) {
  HexCorners K;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 v = hexa[k];
    K.C[k] = {v.x, v.y, v.z};
  }
  return K;
}

// the point query's t from S to the face triangle (P, Q, R): the record (P, Q - P, R - P)
__device__ __forceinline__ float hex_face_t(V3 S, V3 P, V3 Q, V3 R) {
  float t, u, v;
  closest_triangle(S, P, rtd::sub(Q, P), rtd::sub(R, P), t, u, v);
  return t;
}

// the two triangles (a, b, d) and (a, d, c) of the face (a, b, c, d): true when one of them comes within rr of S
__device__ __forceinline__ bool hex_face_near(V3 S, float rr, V3 Ca, V3 Cb, V3 Cc, V3 Cd) {
  __builtin_amdgcn_sched_barrier(0);                               // (keeps this face a block of its own: see HexRegion::sphere)
  return fminf(hex_face_t(S, Ca, Cb, Cd), hex_face_t(S, Ca, Cd, Cc)) <= rr;
}

// The hexahedron as a region shape (rt_overlap.hpp's skeleton).
struct HexRegion {
  static constexpr int kFloat4s = 8;
  static constexpr int kScanWaves = RT_HEX_WAVES, kTreeWaves = RT_HEX_WAVES;
  using Query = HexQuery;
  using SphereCtx = HexCorners;                                    // loaded once there are spheres and the query is valid
  static constexpr bool kSphereCtx = true;

  __device__ static __forceinline__ void load(Query& q, const float4* hexa, size_t base, uint32_t lane, bool live) {
    const float inf = __builtin_inff();
    float4 c0 = {inf, inf, inf, 0.0f}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0, c6 = c0, c7 = c0;   // padding lanes: a non-finite query accepts nothing
    if (live) {
      const float4* const h = hexa + 8u * (base + lane);
      c0 = h[0]; c1 = h[1]; c2 = h[2]; c3 = h[3]; c4 = h[4]; c5 = h[5]; c6 = h[6]; c7 = h[7];
    }
    q = hex_query(c0, c1, c2, c3, c4, c5, c6, c7);
  }
  __device__ static __forceinline__ SphereCtx sphere_ctx(const float4* hexa, size_t base, uint32_t lane) { return hex_corners(hexa + 8u * (base + lane)); }

  // step 1: BoxRegion::step1's comparisons against the region's bounding box
  __device__ static __forceinline__ bool step1(const Query& q, V3 A, V3 B, V3 C) {
    const bool x = overlap_axis1(A.x, B.x, C.x, q.lo.x, q.hi.x), y = overlap_axis1(A.y, B.y, C.y, q.lo.y, q.hi.y);
    const bool z = overlap_axis1(A.z, B.z, C.z, q.lo.z, q.hi.z);
    return q.valid & x & y & z;
  }

  // steps 2 and 3: true when one of the forty-three axes separates the record from the region
  __device__ static __forceinline__ bool separated(const Query& q, V3 A, V3 B, V3 C, V3 e1, V3 e2) {
    using M = Math<false>;
    const V3 a = rtd::sub(A, q.C0), b = rtd::sub(B, q.C0), c = rtd::sub(C, q.C0);
    const V3 f0 = e1, f1 = rtd::sub(c, b), f2 = rtd::sub(a, c);
    // An axis that separates ends the test for its lane: the verdict is the OR of the same forty-three verdicts, and a wave whose
    // live lanes are all separated skips the rest.  The face normals, whose region side hex_query has ready, go first.
    bool s = false;
  #pragma unroll
    for (int f = 0; f < 6; ++f) s |= hex_record_axis(q.fn[f], a, b, c, q.fmn[f], q.fmx[f]);
    if (s) return true;
    if (hex_axis(q, M::cross(e1, e2), a, b, c)) return true;
    // the twelve edges (0,1), (2,3), (4,5), (6,7), (0,2), (1,3), (4,6), (5,7), (0,4), (1,5), (2,6), (3,7)
    if (hex_axes3(q, q.h[1], f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[3], q.h[2]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[5], q.h[4]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[7], q.h[6]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, q.h[2], f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[3], q.h[1]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[6], q.h[4]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[7], q.h[5]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, q.h[4], f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[5], q.h[1]), f0, f1, f2, a, b, c)) return true;
    if (hex_axes3(q, rtd::sub(q.h[6], q.h[2]), f0, f1, f2, a, b, c)) return true;
    return hex_axes3(q, rtd::sub(q.h[7], q.h[3]), f0, f1, f2, a, b, c);
  }

  // the sphere rule: the surface touches the region when the region's nearest point is inside the ball and its farthest corner
  // is not.  d2min <= r*r is decided face by face -- the smallest t is within r*r exactly when one of the twelve is (minNum drops a
  // NaN, and a NaN compares false) -- and a face that decides ends it.  Left to itself the compiler flattens the six faces into
  // one block (the point query is branchless) and the scheduler interleaves the twelve of them past the register file; the
  // scheduling barrier in hex_face_near cannot be speculated, so every face stays a block of its own.
  __device__ static __forceinline__ bool sphere(const Query& q, const SphereCtx& K, float4 sph) {
    using M = Math<false>;
    const V3 S = {sph.x, sph.y, sph.z};
    const V3 s = rtd::sub(S, q.C0);
    const float rr = sph.w * sph.w;
    float d2max = 0.0f;
  #pragma unroll
    for (int k = 0; k < 8; ++k) {
      const V3 w = rtd::sub(K.C[k], S);
      const float d2 = M::dot(w, w);
      d2max = k == 0 ? d2 : fmaxf(d2max, d2);
    }
    if (!(q.valid & (rr <= d2max))) return false;
    bool out = false;                                                // a face normal separates the centre from the corners
  #pragma unroll
    for (int f = 0; f < 6; ++f) {
      const float ps = M::dot(q.fn[f], s);
      out |= !__builtin_isunordered(ps, ps) & ((ps > q.fmx[f]) | (ps < q.fmn[f]));
    }
    if (!out) return 0.0f <= rr;                                     // inside: d2min = 0 (a NaN radius touches nothing)
    if (hex_face_near(S, rr, K.C[0], K.C[2], K.C[4], K.C[6])) return true;
    if (hex_face_near(S, rr, K.C[1], K.C[3], K.C[5], K.C[7])) return true;
    if (hex_face_near(S, rr, K.C[0], K.C[1], K.C[4], K.C[5])) return true;
    if (hex_face_near(S, rr, K.C[2], K.C[3], K.C[6], K.C[7])) return true;
    if (hex_face_near(S, rr, K.C[0], K.C[1], K.C[2], K.C[3])) return true;
    return hex_face_near(S, rr, K.C[4], K.C[5], K.C[6], K.C[7]);
  }
};

hipError_t launch_overlap_hexahedra(const TraceParams& p, const BvhParams* b, uint32_t n, const float* hexa, const int* after,
                                    uint32_t max_hits, int* prims, uint32_t* counts, hipStream_t st) {
  return launch_region<HexRegion>(p, b, n, hexa, after, max_hits, prims, counts, st);
}

}  // namespace rtk
