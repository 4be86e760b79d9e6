// rt_trioverlap.hpp -- the triangle-shaped region query (rt_tracer_overlap_triangles*): the primitives of the
// tracer's scene that touch query triangle i, the max_hits lowest of them in ascending prim order behind an optional cursor, and
// the total number of them.  Included by rt_kernels.hip only, behind rt_overlap.hpp, whose list (OverlapList<CAP>), cursor
// (overlap_cursor, overlap_behind) and box-axis comparison (overlap_axis1) are used as they are.
//
// Acceptance is a pure function of (query, record, cursor), the text of include/rt_mi355x.h operation by operation: ONE
// arithmetic, every operation rounded separately (the library is compiled with -ffp-contract=off).  On the record the renderer
// intersects, A = v0, B = fl(v0 + e1), C = fl(v0 + e2), against the query P0, P1, P2:
//   step 1 (tri_step1)       the query finite, neither B nor C a NaN, per axis min(A, B, C) <= max(P) and max(A, B, C) >= min(P)
//   step 2                   a = A - P0, b = B - P0, c = C - P0, p1 = P1 - P0, p2 = P2 - P0; the query's own corner is 0
//   step 3 (tri_separated)   17 axes: n = e1 x e2, m = p1 x p2, the nine f_i x g_j, the three n x f_i, the three m x g_j of
//                            f = e1, c - b, a - c and g = p1, p2 - p1, p2.  ALL six points are projected on every axis: a
//                            corner shared bit for bit projects identically on both sides, so no axis separates the pair.
// An axis separates when every record projection is > every query projection, or every one is <; a NaN projection makes its
// comparisons false and never separates.  tri_axis takes min3 / max3 of each side and masks the verdict with "no projection
// is a NaN": the same verdicts as the nine plus nine comparisons, since without a NaN min3 / max3 are exact.
// A sphere is its surface (tri_sphere): closest_triangle's t from the centre to the query's own record against r*r, and the
// farthest query corner.
//
// Why the tree prunes exactly, with no slack: the argument of rt_overlap.hpp with the query triangle's bounding box in the place
// of the caller's box.  Step 1's record interval lies inside rtb::detail::tri_box; a child is entered when its box and the
// query's bounding box overlap under the same closed comparisons.  b.rho is not read.
//
// trioverlap_kernel<CAP> (RT_QUERY_SCAN) and trioverlap_bvh_kernel<CAP> (RT_QUERY_BVH) have the shapes of overlap_kernel and
// overlap_bvh_kernel: 256-thread blocks over LDS chunks of kQueryChunk records with a per-record ballot exit after step 1; one
// wave per block over bvh_walk<64, false>, then the overflow redo, the always-tested list and the spheres.  The query is three
// 16-byte loads.  The axes are evaluated in groups of three (one f against the three g) so that no more than a group's
// projections are live at once: 0 B of scratch in all six kernels.  The tree kernels ask for 4 waves per SIMD: left alone, the
// max-ILP scheduler interleaves the seventeen axes of the three inlined record tests up to 242 VGPRs (2 waves); bounded it
// stays at 90 - 107 VGPRs with 0 B of scratch (a few SGPRs are kept in VGPR lanes).
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

// step 1: overlap_step1's comparisons against the query's bounding box
__device__ __forceinline__ bool tri_step1(const TriQuery& q, V3 A, V3 B, V3 C) {
  const bool x = overlap_axis1(A.x, B.x, C.x, q.lo.x, q.hi.x), y = overlap_axis1(A.y, B.y, C.y, q.lo.y, q.hi.y);
  const bool z = overlap_axis1(A.z, B.z, C.z, q.lo.z, q.hi.z);
  return q.valid & x & y & z;
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

// steps 2 and 3: true when one of the seventeen axes separates the record from the query
__device__ __forceinline__ bool tri_separated(const TriQuery& q, V3 A, V3 B, V3 C, V3 e1, V3 e2) {
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
__device__ __forceinline__ bool tri_sphere(const TriQuery& q, float4 sph) {
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

template <int CAP>
__global__ __launch_bounds__(256, 4) void trioverlap_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ tris,
                                                             const int* __restrict__ after, uint32_t max_hits,
                                                             int* __restrict__ prims, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first query of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  const float inf = __builtin_inff();
  float4 q0 = {inf, inf, inf, 0.0f}, q1 = q0, q2 = q0;                  // padding lanes: a non-finite query accepts nothing
  if (tid < nb) { q0 = tris[3u * (base + tid)]; q1 = tris[3u * (base + tid) + 1u]; q2 = tris[3u * (base + tid) + 2u]; }
  const TriQuery q = tri_query(q0, q1, q2);
  const int cur = overlap_cursor(after, base + tid, tid < nb);

  OverlapList<CAP> L;
  L.init_scan();

  // the triangles, staged into LDS chunk by chunk; every chunk is scanned
  const uint32_t nt = p.n_tris;
  const uint32_t cap = nt < kQueryChunk ? nt : kQueryChunk;
  float4* const sA = s_mem;                                        // 2 float4 per triangle
  float* const sB = reinterpret_cast<float*>(s_mem + 2u * cap);    // v0.z
  for (uint32_t c0 = 0; c0 < nt; c0 += kQueryChunk) {
    const uint32_t cn = (nt - c0 < kQueryChunk) ? nt - c0 : kQueryChunk;
    __syncthreads();                                               // the previous chunk is read
    for (uint32_t i = tid; i < 2u * cn; i += 256u) sA[i] = p.tri_a[2u * c0 + i];
    for (uint32_t i = tid; i < cn; i += 256u) sB[i] = p.tri_b[c0 + i];
    __syncthreads();
    if (__builtin_amdgcn_ballot_w64(q.valid) == 0ull) continue;    // no query of this wave accepts; it still helps staging
    for (uint32_t j = 0; j < cn; ++j) {
      const float4 A0 = sA[2u * j], A1 = sA[2u * j + 1u];
      const V3 e2 = {A0.x, A0.y, A0.z}, e1 = {A0.w, A1.x, A1.y}, A = {A1.z, A1.w, sB[j]};
      const V3 B = rtd::add(A, e1), C = rtd::add(A, e2);
      const int prim = static_cast<int>(c0 + j);
      const bool behind = overlap_behind(prim, cur);
      const bool in1 = tri_step1(q, A, B, C) & behind;
      if (__builtin_amdgcn_ballot_w64(in1) == 0ull) continue;      // step 1 rejects it for every query of the wave
      if (in1 && !tri_separated(q, A, B, C, e1, e2)) L.append(prim, max_hits);
    }
  }
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    const int prim = static_cast<int>(nt + si);
    if (tri_sphere(q, p.spheres[si]) && overlap_behind(prim, cur)) L.append(prim, max_hits);
  }

  if (tid < nb) L.store_scan(max_hits, prims + (base + tid) * max_hits, counts + base + tid);
}

// one 48-byte record against one query
template <int CAP>
__device__ __forceinline__ void trioverlap_test_record(const float4* __restrict__ rec, const TriQuery& q, int cur, OverlapList<CAP>& L) {
  const BvhRecord r = bvh_record(rec);
  const V3 B = rtd::add(r.v0, r.e1), C = rtd::add(r.v0, r.e2);
  if (tri_step1(q, r.v0, B, C) && overlap_behind(r.idx, cur) && !tri_separated(q, r.v0, B, C, r.e1, r.e2)) L.insert(r.idx);
}

template <int CAP>
__global__ __launch_bounds__(64, 4) void trioverlap_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n,
                                                             const float4* __restrict__ tris, const int* __restrict__ after,
                                                             uint32_t max_hits, int* __restrict__ prims, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const TriQuery q = tri_query(tris[3u * i], tris[3u * i + 1u], tris[3u * i + 2u]);
  const int cur = overlap_cursor(after, i, true);

  OverlapList<CAP> L;
  L.init_tree(max_hits);

  const float inf = __builtin_inff();
  // the child's box against the query's bounding box: step 1's comparisons, no inflation; the key is constant
  auto child = [&](const BvhNode& nd, int c) {
    const bool in = (nd.lo[0][c] <= q.hi.x) & (nd.hi[0][c] >= q.lo.x) & (nd.lo[1][c] <= q.hi.y) & (nd.hi[1][c] >= q.lo.y) &
                    (nd.lo[2][c] <= q.hi.z) & (nd.hi[2][c] >= q.lo.z);
    return in ? 0.0f : -inf;
  };
  auto leaf = [&](const float4* rec) { trioverlap_test_record<CAP>(rec, q, cur, L); return false; };
  const bool overflow = bvh_walk<64u, false>(b, s_mem, lane, q.valid, child, leaf, [](float) { return false; });
  if (overflow) {                                                  // an entry was not kept: every leaf record, from an empty list and count
    L.init_tree(max_hits);
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) trioverlap_test_record<CAP>(b.records + 3u * j, q, cur, L);
  }
  if (q.valid) {
    for (uint32_t j = 0; j < b.n_always; ++j) trioverlap_test_record<CAP>(b.records + 3u * (b.n_leaf_records + j), q, cur, L);
    for (uint32_t si = 0; si < p.n_spheres; ++si) {
      const int prim = static_cast<int>(p.n_tris + si);
      if (tri_sphere(q, p.spheres[si]) && overlap_behind(prim, cur)) L.insert(prim);
    }
  }
  L.store_tree(max_hits, prims + i * max_hits, counts + i);
}

// CAP = 0 for max_hits 0, 4 for 1 .. 4, else 16, in both forms
hipError_t launch_overlap_triangles(const TraceParams& p, const BvhParams* b, uint32_t n, const float* tris, const int* after,
                                    uint32_t max_hits, int* prims, uint32_t* counts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (max_hits > kAllHitsMax || tris == nullptr || counts == nullptr || (prims == nullptr && max_hits != 0u)) return hipErrorInvalidValue;
  const float4* const t4 = reinterpret_cast<const float4*>(tris);
  if (b != nullptr) {                                              // one wave per block, lane = query, the reference alone on the stack
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, false);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    const auto walk = max_hits == 0u ? trioverlap_bvh_kernel<0> : max_hits <= 4u ? trioverlap_bvh_kernel<4> : trioverlap_bvh_kernel<16>;
    return launch_blocks(walk, n, 64u, 64u, lds, st, p, *b, n, t4, after, max_hits, prims, counts);
  }
  const auto scan = max_hits == 0u ? trioverlap_kernel<0> : max_hits <= 4u ? trioverlap_kernel<4> : trioverlap_kernel<16>;
  return launch_blocks(scan, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, t4, after, max_hits, prims, counts);
}

}  // namespace rtk
