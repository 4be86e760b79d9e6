// rt_tridistance.hpp -- the triangle-shaped proximity query (rt_tracer_triangle_distance*): the primitive of the
// tracer's scene nearest to query triangle i within that triangle's own squared search radius, where on the primitive, and where
// on the query triangle.  Included by rt_kernels.hip only, behind rt_trioverlap.hpp, whose TriQuery (corners, p1, p2, bounding
// box, validity) and sphere verdict (TriRegion::sphere) are used as they are, as are rt_closest.hpp's closest_triangle and closest_keep.
//
// The rule is the text of include/rt_mi355x.h operation by operation: ONE arithmetic, every operation rounded separately (the
// library is compiled with -ffp-contract=off), division correctly rounded, min and max IEEE minNum / maxNum.  Against a record
// (v0, e1, e2) with corners A = v0, B = fl(v0 + e1), C = fl(v0 + e2) there are 21 candidate points x_k ON THE QUERY triangle:
//   0-2    its corners
//   3-5    the projections of A, B, C onto it (td_project: closest_triangle's (u', v') on the record (P0, p1, p2))
//   6-14   the point of query edge j nearest to record edge i, k = 6 + 3i + j (td_seg_s: Ericson's closest points of two segments)
//   15-17  where query edge j crosses the record's plane (td_plane_s)
//   18-20  where record edge i crosses the query's plane, projected onto the query
// each clamped per axis into the query's bounding box; a candidate that is absent or has a NaN coordinate is not considered.
// t_k = closest_triangle(x_k) on the record, UNCHANGED; the pair's answer is the smallest t_k, equal t to the lowest k.  So
// every distance this query reports is the point query's own for a point inside the query's bounding box, which is what lets
// the tree prune by the point query's bound (4.3f) with the box in the place of the point: no new rounding proof.
// A sphere has four candidates (the corners and the centre's projection) under closest_finish's sphere arithmetic; t = 0 when
// OverlapTriangles' sphere condition (TriRegion::sphere) holds.  Winner: closest_keep's (t, prim) rule, best starting at d2max.
//
// tridistance_kernel (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = query, the query is three 16-byte
// loads; spheres after the triangles.  The scan carries (t, prim) only: the winner's (u, v) and the witness are recomputed
// from the winning record at the end (td_finish).
//
// tridistance_bvh_kernel (RT_QUERY_BVH): one wave per block, lane = query, bvh_walk<64, true> (keyed entries {-lb, reference}).
// Per child, in fp32,
//   pad = rho_c * (qabs + cmax)       g = max(max(lo - qmax, qmin - hi, 0) - pad, 0) per axis
//   lb  = ((gx*gx + gy*gy) + gz*gz) * (1 - 2^-21)
// which, term by term, is at most what closest_bvh_kernel computes for ANY point of [qmin, qmax] (fp32 subtraction,
// multiplication and max are monotone), hence a lower bound of every t_k of every record inside the child.  A child is skipped
// only when lb > best STRICTLY, at the visit and again at the pop; a NaN lb takes no pruning decision.  Then the overflow redo,
// the always-tested list and the spheres.
#pragma once
#include "rt_trioverlap.hpp"

namespace rtk {

// the query as the rule reads it: TriQuery and what else depends on the query alone
struct TdQuery {
  TriQuery q;
  V3 g1, g2;          // the second and third edge vectors P2 - P1, P0 - P2 (the first is q.p1)
  V3 m;               // p1 x p2
  float a0, a1, a2;   // the edges' squared lengths
  float qabs;         // the largest |coordinate| of the corners
  float d2max;
  bool active;        // finite corners and d2max >= 0
};

__device__ __forceinline__ TdQuery td_query(float4 q0, float4 q1, float4 q2) {
  using M = Math<false>;
  TdQuery d;
  d.q = tri_query(q0, q1, q2);
  d.g1 = rtd::sub(d.q.P2, d.q.P1);
  d.g2 = rtd::sub(d.q.P0, d.q.P2);
  d.m = M::cross(d.q.p1, d.q.p2);
  d.a0 = M::dot(d.q.p1, d.q.p1); d.a1 = M::dot(d.g1, d.g1); d.a2 = M::dot(d.g2, d.g2);
  const float m0 = fmaxf(fmaxf(fabsf(q0.x), fabsf(q0.y)), fabsf(q0.z)), m1 = fmaxf(fmaxf(fabsf(q1.x), fabsf(q1.y)), fabsf(q1.z));
  const float m2 = fmaxf(fmaxf(fabsf(q2.x), fabsf(q2.y)), fabsf(q2.z));
  d.qabs = fmaxf(fmaxf(m0, m1), m2);
  d.d2max = q0.w;
  d.active = d.q.valid & (q0.w >= 0.0f);                           // a NaN or negative d2max accepts nothing
  return d;
}

__device__ __forceinline__ float td_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }   // a NaN becomes 0

// G0 + s * d per component (the product, then the sum)
__device__ __forceinline__ V3 td_along(V3 G0, float s, V3 d) { return {G0.x + s * d.x, G0.y + s * d.y, G0.z + s * d.z}; }

// the projection of Y onto the query: closest_triangle's (u', v') on the record (P0, p1, p2), then (P0 + u'*p1) + v'*p2
__device__ __forceinline__ V3 td_project(const TriQuery& q, V3 Y) {
  float t, u, v;
  closest_triangle(Y, q.P0, q.p1, q.p2, t, u, v);
  return {(q.P0.x + u * q.p1.x) + v * q.p2.x, (q.P0.y + u * q.p1.y) + v * q.p2.y, (q.P0.z + u * q.p1.z) + v * q.p2.z};
}

// Ericson's closest points of two segments, the parameter s of the FIRST: G0 + s*d1 (a = d1.d1) against R0 + t*d2 (e = d2.d2).
// The guards are exact comparisons with 0; the t-driven re-clamp is decided on tnom = b*s + f against 0 and e (no division).
__device__ __forceinline__ float td_seg_s(V3 G0, V3 d1, float a, V3 R0, V3 d2, float e) {
  using M = Math<false>;
  const V3 r = rtd::sub(G0, R0);
  const float f = M::dot(d2, r), c = M::dot(d1, r), b = M::dot(d1, d2);
  const float denom = a * e - b * b;
  float s0 = td_clamp01((b * f - c * e) / denom);
  if (denom == 0.0f) s0 = 0.0f;
  const float tnom = b * s0 + f;
  const bool low = (tnom < 0.0f) | (e == 0.0f), redo = low | (tnom > e);
  const float s1 = td_clamp01((low ? -c : b - c) / a);
  return a == 0.0f ? 0.0f : redo ? s1 : s0;
}

// where the segment with signed plane offsets da (start) and db (end) crosses the plane; absent unless da*db <= 0 && da != db
__device__ __forceinline__ float td_plane_s(float da, float db, bool& present) {
  present = (da * db <= 0.0f) & (da != db);
  return td_clamp01(da / (da - db));
}

// the least t_k so far of one pair: k < 0 = none yet
struct TdPair {
  float t, u, v;
  V3 x;
  int k;
};

// candidate k of a record: the NaN check, the clamp into the query's box, the point query's triangle rule, the fold
__device__ __forceinline__ void td_try(const TriQuery& q, V3 x, bool present, int k, V3 v0, V3 e1, V3 e2, TdPair& b) {
  const bool ok = present & !(__builtin_isunordered(x.x, x.y) | __builtin_isunordered(x.z, x.z));
  x = {fminf(fmaxf(x.x, q.lo.x), q.hi.x), fminf(fmaxf(x.y, q.lo.y), q.hi.y), fminf(fmaxf(x.z, q.lo.z), q.hi.z)};
  float t, u, v;
  closest_triangle(x, v0, e1, e2, t, u, v);
  if (ok & ((t < b.t) | ((b.k < 0) & (t <= b.t)))) { b.t = t; b.u = u; b.v = v; b.x = x; b.k = k; }
}

// one record against one query: the 21 candidates in ascending k.  Where only .t is read the rest is dead code.
__device__ __forceinline__ TdPair td_triangle(const TdQuery& d, V3 A, V3 e1, V3 e2) {
  using M = Math<false>;
  const TriQuery& q = d.q;
  TdPair b = {__builtin_inff(), 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}, -1};
  const V3 B = rtd::add(A, e1), C = rtd::add(A, e2);
  td_try(q, q.P0, true, 0, A, e1, e2, b);
  td_try(q, q.P1, true, 1, A, e1, e2, b);
  td_try(q, q.P2, true, 2, A, e1, e2, b);
  td_try(q, td_project(q, A), true, 3, A, e1, e2, b);
  td_try(q, td_project(q, B), true, 4, A, e1, e2, b);
  td_try(q, td_project(q, C), true, 5, A, e1, e2, b);
  const V3 G[3] = {q.P0, q.P1, q.P2}, dg[3] = {q.p1, d.g1, d.g2};
  const float ag[3] = {d.a0, d.a1, d.a2};
  const V3 R[3] = {A, B, C}, dr[3] = {rtd::sub(B, A), rtd::sub(C, B), rtd::sub(A, C)};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float e = M::dot(dr[i], dr[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) td_try(q, td_along(G[j], td_seg_s(G[j], dg[j], ag[j], R[i], dr[i], e), dg[j]), true, 6 + 3 * i + j, A, e1, e2, b);
  }
  const V3 n = M::cross(e1, e2);
  const float dq[3] = {M::dot(n, rtd::sub(q.P0, A)), M::dot(n, rtd::sub(q.P1, A)), M::dot(n, rtd::sub(q.P2, A))};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    bool present;
    const float s = td_plane_s(dq[j], dq[(j + 1) % 3], present);
    td_try(q, td_along(G[j], s, dg[j]), present, 15 + j, A, e1, e2, b);
  }
  const float dp[3] = {M::dot(d.m, rtd::sub(A, q.P0)), M::dot(d.m, rtd::sub(B, q.P0)), M::dot(d.m, rtd::sub(C, q.P0))};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    bool present;
    const float s = td_plane_s(dp[i], dp[(i + 1) % 3], present);
    td_try(q, td_project(q, td_along(R[i], s, dr[i])), present, 18 + i, A, e1, e2, b);
  }
  if (b.k < 0) b.t = __builtin_nanf("");                           // nothing considered: never accepted
  return b;
}

// one sphere against one query: s = |sqrt(w.w) - radius|, t = s*s at the corners and at the centre's projection
__device__ __forceinline__ TdPair td_sphere(const TdQuery& d, float4 sph) {
  using M = Math<false>;
  const TriQuery& q = d.q;
  const V3 ctr = {sph.x, sph.y, sph.z};
  TdPair b = {__builtin_inff(), 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}, -1};
  auto attempt = [&](V3 x, int k) {
    const bool ok = !(__builtin_isunordered(x.x, x.y) | __builtin_isunordered(x.z, x.z));
    x = {fminf(fmaxf(x.x, q.lo.x), q.hi.x), fminf(fmaxf(x.y, q.lo.y), q.hi.y), fminf(fmaxf(x.z, q.lo.z), q.hi.z)};
    const V3 w = rtd::sub(x, ctr);
    const float s = fabsf(__builtin_sqrtf(M::dot(w, w)) - sph.w), t = s * s;
    if (ok & ((t < b.t) | ((b.k < 0) & (t <= b.t)))) { b.t = t; b.x = x; b.k = k; }
  };
  attempt(q.P0, 0); attempt(q.P1, 1); attempt(q.P2, 2); attempt(td_project(q, ctr), 3);
  if (b.k < 0) b.t = __builtin_nanf("");
  else if (TriRegion::sphere(q, {}, sph)) b.t = 0.0f;                         // the surface touches the query: OverlapTriangles' verdict
  return b;
}

// the spheres (prim = n_tris + sphere index), then the query's two records from the winner itself
__device__ __forceinline__ void td_finish(const TraceParams& p, const TdQuery& d, float best, int best_i, float4& hit, float4& wit) {
  const uint32_t nt = p.n_tris;
  for (uint32_t si = 0; si < p.n_spheres; ++si) closest_keep(td_sphere(d, p.spheres[si]).t, static_cast<int>(nt + si), best, best_i);
  hit = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
  wit = hit;
  if (best_i < 0) return;
  TdPair w;
  if (static_cast<uint32_t>(best_i) < nt) {
    const float4 A0 = p.tri_a[2 * best_i], A1 = p.tri_a[2 * best_i + 1];
    w = td_triangle(d, {A1.z, A1.w, p.tri_b[best_i]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z});
  } else {
    w = td_sphere(d, p.spheres[static_cast<uint32_t>(best_i) - nt]);
  }
  hit = make_float4(best, w.u, w.v, __int_as_float(best_i));
  wit = make_float4(w.x.x, w.x.y, w.x.z, __int_as_float(w.k));
}

__global__ __launch_bounds__(256, 2) void tridistance_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ tris,
                                                              float4* __restrict__ hits, float4* __restrict__ witness) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first query of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  float4 q0 = {0.0f, 0.0f, 0.0f, -1.0f}, q1 = q0, q2 = q0;              // padding lanes accept nothing
  if (tid < nb) { q0 = tris[3u * (base + tid)]; q1 = tris[3u * (base + tid) + 1u]; q2 = tris[3u * (base + tid) + 2u]; }
  const TdQuery d = td_query(q0, q1, q2);
  float best = d.d2max;
  int best_i = -1;

  // the triangles; every chunk is scanned, by the waves that hold a query that accepts
  scan_triangles<ScanMode::SkipIdleWaves>(p, s_mem, [&] { return d.active; }, [&](const float4 A0, const float4 A1, auto z, int prim) {
    const float t = td_triangle(d, {A1.z, A1.w, z()}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}).t;
    if (d.active) closest_keep(t, prim, best, best_i);
  });
  if (tid < nb) {
    float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)}, w = h;
    if (d.active) td_finish(p, d, best, best_i, h, w);
    hits[base + tid] = h;
    witness[base + tid] = w;
  }
}

// one 48-byte record against one query
__device__ __forceinline__ void td_test_record(const float4* __restrict__ rec, const TdQuery& d, float& best, int& best_i) {
  const BvhRecord r = bvh_record(rec);
  closest_keep(td_triangle(d, r.v0, r.e1, r.e2).t, r.idx, best, best_i);
}

__global__ __launch_bounds__(64, 2) void tridistance_bvh_kernel(const TraceParams p, const BvhParams b, float rho_c, uint32_t n,
                                                                 const float4* __restrict__ tris, float4* __restrict__ hits,
                                                                 float4* __restrict__ witness) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const TdQuery d = td_query(tris[3u * i], tris[3u * i + 1u], tris[3u * i + 2u]);
  if (!d.active) {
    hits[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    witness[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    return;
  }
  float best = d.d2max;
  int best_i = -1;

  const float inf = __builtin_inff();
  const V3 lo = d.q.lo, hi = d.q.hi;
  auto child = [&](const BvhNode& nd, int c) {
    const float pad = rho_c * (d.qabs + nd.cmax[c]);
    const float gx = fmaxf(fmaxf(fmaxf(nd.lo[0][c] - hi.x, lo.x - nd.hi[0][c]), 0.0f) - pad, 0.0f);
    const float gy = fmaxf(fmaxf(fmaxf(nd.lo[1][c] - hi.y, lo.y - nd.hi[1][c]), 0.0f) - pad, 0.0f);
    const float gz = fmaxf(fmaxf(fmaxf(nd.lo[2][c] - hi.z, lo.z - nd.hi[2][c]), 0.0f) - pad, 0.0f);
    const float lb = ((gx * gx + gy * gy) + gz * gz) * kClosestDeflate;
    return !(lb == lb) ? inf : lb > best ? -inf : fmaxf(-lb, -FLT_MAX);   // a NaN lb takes no pruning decision
  };
  auto leaf = [&](const float4* rec) { td_test_record(rec, d, best, best_i); return false; };
  const bool overflow = bvh_walk<64u, true>(b, s_mem, lane, true, child, leaf, [&](float key) { return key < -best; });
  if (overflow) {                                                  // an entry was not kept: every leaf record, from the start
    best = d.d2max; best_i = -1;
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) td_test_record(b.records + 3u * j, d, best, best_i);
  }
  for (uint32_t j = 0; j < b.n_always; ++j) td_test_record(b.records + 3u * (b.n_leaf_records + j), d, best, best_i);
  float4 h, w;
  td_finish(p, d, best, best_i, h, w);
  hits[i] = h;
  witness[i] = w;
}

hipError_t launch_triangle_distance(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* tris, float4* hits,
                                    float4* witness, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (tris == nullptr || hits == nullptr || witness == nullptr) return hipErrorInvalidValue;
  const float4* const t4 = reinterpret_cast<const float4*>(tris);
  if (b != nullptr) {                                              // one wave per block, lane = query, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(tridistance_bvh_kernel, n, 64u, 64u, lds, st, p, *b, rho_c, n, t4, hits, witness);
  }
  return launch_blocks(tridistance_kernel, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, t4, hits, witness);
}

}  // namespace rtk
