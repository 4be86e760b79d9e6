// rt_closest.hpp -- the point query (rt_tracer_closest_point*): the nearest surface point of the tracer's scene
// to point i, within that point's own squared search radius.  Included by rt_kernels.hip only, behind rt_allhits.hpp.  Nothing
// is shared with the ray-query kernels beyond V3, Math<false>::dot (the separately rounded (x*x' + y*y') + z*z') and the tree.
//
// A candidate is every triangle through the record the renderer intersects (v0, e1, e2) and every sphere through its surface.
// Triangle: Ericson's closest point on a triangle restated on the record (closest_triangle below, the text of
// include/rt_mi355x.h operation by operation); there is no reference arithmetic to be faithful to, so there is ONE arithmetic,
// every operation rounded separately (the library is compiled with -ffp-contract=off), the division correctly rounded.  The
// seven regions are evaluated without branches: each region's one division is selected first and performed once, which is the
// same operation on the same operands and therefore the same bits.  Sphere: s = |sqrt(w.w) - radius|, t = s*s.
// Accepted: t <= d2max in plain fp32 (a NaN t never; a NaN or negative d2max accepts nothing).  Winner: the smallest (t, prim),
// equal t (==) to the lowest prim -- a rule that names no visiting order, so the scan and the traversal cannot disagree.
//
// closest_kernel (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = point, the point is one 16-byte load;
// spheres after the triangles.
//
// closest_bvh_kernel (RT_QUERY_BVH): one wave per block, lane = point, the tree and the LDS stack of rt_bvh.hpp (8-byte entries
// {-lb, reference} at entry * 64 + lane, capacity b.stack_cap, overflow = every leaf record).  Per child, in fp32,
//   pad = rho_c * (max|p| + cmax)          g = max(max(lo - p, p - hi, 0) - pad, 0) per axis
//   lb  = ((gx*gx + gy*gy) + gz*gz) * (1 - 2^-21)
// a lower bound of the t every record inside the child's box computes (DESIGN.md 4.3f derives rho_c).  A child is skipped only
// when lb > best STRICTLY (a tie may hide a lower index); the nearest child is entered first, the others wait on the stack and
// are dropped at the pop when their lb has fallen strictly behind best.  best starts at d2max.  A point with a non-finite
// coordinate, or a child whose lb is a NaN, takes no pruning decision.  The always-tested list and the spheres follow.
//
// closest_bvh_kernel keeps the walk in its own text -- the loop, the node unpack and the ordering network are A SECOND COPY of
// rt_bvh_walk.hpp's bvh_walk: change them together.  On the shared function this kernel measured slower than its
// parent by more than the parent's own run-to-run spread, in every shape of the function that was tried.
#pragma once
#include "rt_allhits.hpp"

namespace rtk {

constexpr float kClosestDeflate = 0.999999523162841796875f;   // 1 - 2^-21

// t = squared distance from p to the triangle (v0, e1, e2), (u, v) = the nearest point's barycentrics; the residual r = p - c
// it forms on the way and the feature of the triangle that holds c, in the order of rt_features_host.hpp's table: 0 the face
// (region 7), 1, 2, 3 the vertices A, B, C (regions 1, 2, 4), 4, 5, 6 the edges AB, AC, BC (regions 3, 5, 6).
__device__ __forceinline__ void closest_triangle_feature(V3 p, V3 v0, V3 e1, V3 e2, float& t, float& u, float& v, V3& r, int& feature) {
  using M = Math<false>;
  const V3 ap = rtd::sub(p, v0);
  const float a = M::dot(e1, e1), b = M::dot(e1, e2), c = M::dot(e2, e2);
  const float d1 = M::dot(e1, ap), d2 = M::dot(e2, ap);
  const float d3 = d1 - a, d4 = d2 - b, d5 = d1 - b, d6 = d2 - c;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float d43 = d4 - d3, d56 = d5 - d6;
  const bool r1 = d1 <= 0.0f && d2 <= 0.0f;
  const bool r2 = d3 >= 0.0f && d4 <= d3;
  const bool r3 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
  const bool r4 = d6 >= 0.0f && d5 <= d6;
  const bool r5 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  const bool r6 = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
  // the division of the first region that holds among 3, 5, 6, 7 (regions 1, 2, 4 divide nothing)
  const float num = r3 ? d1 : r5 ? d2 : r6 ? d43 : 1.0f;
  const float den = r3 ? d1 - d3 : r5 ? d2 - d6 : r6 ? d43 + d56 : (va + vb) + vc;
  const float q = num / den;
  if (r1) { u = 0.0f; v = 0.0f; }
  else if (r2) { u = 1.0f; v = 0.0f; }
  else if (r3) { u = q; v = 0.0f; }
  else if (r4) { u = 0.0f; v = 1.0f; }
  else if (r5) { u = 0.0f; v = q; }
  else if (r6) { u = 1.0f - q; v = q; }
  else { u = vb * q; v = vc * q; }
  feature = r1 ? 1 : r2 ? 2 : r3 ? 4 : r4 ? 3 : r5 ? 5 : r6 ? 6 : 0;
  r = {(ap.x - u * e1.x) - v * e2.x, (ap.y - u * e1.y) - v * e2.y, (ap.z - u * e1.z) - v * e2.z};
  t = M::dot(r, r);
}

// t, u and v alone: what the searches keep
__device__ __forceinline__ void closest_triangle(V3 p, V3 v0, V3 e1, V3 e2, float& t, float& u, float& v) {
  V3 r;
  int feature;
  closest_triangle_feature(p, v0, e1, e2, t, u, v, r, feature);
}

// one accepted candidate under the order-free winner rule (best starts at d2max with best_i = -1: t == d2max is accepted)
__device__ __forceinline__ void closest_keep(float t, int prim, float& best, int& best_i) {
  if ((t < best) | ((t == best) & ((best_i < 0) | (prim < best_i)))) { best = t; best_i = prim; }
}

// the spheres (prim = n_tris + sphere index), then the point's record; u, v of a winning triangle from its record
__device__ __forceinline__ float4 closest_finish(const TraceParams& p, V3 pt, float best, int best_i) {
  using M = Math<false>;
  const uint32_t nt = p.n_tris;
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    const float4 sph = p.spheres[si];
    const V3 w = rtd::sub(pt, {sph.x, sph.y, sph.z});
    const float s = fabsf(__builtin_sqrtf(M::dot(w, w)) - sph.w);
    closest_keep(s * s, static_cast<int>(nt + si), best, best_i);
  }
  float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
  if (best_i >= 0) {
    h.x = best;
    h.w = __int_as_float(best_i);
    if (static_cast<uint32_t>(best_i) < nt) {
      const float4 A0 = p.tri_a[2 * best_i], A1 = p.tri_a[2 * best_i + 1];
      float t = 0.0f, u = 0.0f, v = 0.0f;
      closest_triangle(pt, {A1.z, A1.w, p.tri_b[best_i]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
      h.y = u; h.z = v;
    }
  }
  return h;
}

__global__ __launch_bounds__(256, 4) void closest_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ pts,
                                                          float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first point of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  float4 q = {0.0f, 0.0f, 0.0f, -1.0f};                            // padding lanes accept nothing
  if (tid < nb) q = pts[base + tid];
  const V3 pt = {q.x, q.y, q.z};
  const bool active = q.w >= 0.0f;                                 // a NaN or negative d2max accepts nothing
  float best = q.w;
  int best_i = -1;

  // the triangles; every chunk is scanned, by the waves that hold a point that accepts
  scan_triangles<ScanMode::SkipIdleWaves>(p, s_mem, [&] { return active; }, [&](const float4 A0, const float4 A1, auto z, int prim) {
    float t, u, v;
    closest_triangle(pt, {A1.z, A1.w, z()}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
    if (active) closest_keep(t, prim, best, best_i);
  });
  if (tid < nb) {
    float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
    if (active) h = closest_finish(p, pt, best, best_i);
    hits[base + tid] = h;
  }
}

// one record against one point
__device__ __forceinline__ void closest_test_record(const float4* __restrict__ rec, V3 pt, float& best, int& best_i) {
  const float4 A0 = rec[0], A1 = rec[1], B = rec[2];
  float t, u, v;
  closest_triangle(pt, {A1.z, A1.w, B.x}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
  closest_keep(t, __float_as_int(B.y), best, best_i);
}

__global__ __launch_bounds__(64) void closest_bvh_kernel(const TraceParams p, const BvhParams b, float rho_c, uint32_t n,
                                                          const float4* __restrict__ pts, float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const float4 q = pts[i];
  const V3 pt = {q.x, q.y, q.z};
  if (!(q.w >= 0.0f)) {                                            // a NaN or negative d2max accepts nothing
    hits[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    return;
  }
  float best = q.w;
  int best_i = -1;

  uint2* const stack = reinterpret_cast<uint2*>(s_mem) + lane;     // entry e at stack[e * 64]
  const float inf = __builtin_inff();
  const bool finite = fabsf(pt.x) < inf && fabsf(pt.y) < inf && fabsf(pt.z) < inf;
  const float pmax = fmaxf(fmaxf(fabsf(pt.x), fabsf(pt.y)), fabsf(pt.z));
  uint32_t sp = 0u;
  uint32_t cur = b.n_nodes != 0u ? 0u : kBvhEmpty;
  bool overflow = false;
  for (;;) {
    if (cur == kBvhEmpty) {
      if (sp == 0u) break;
      --sp;
      const uint2 e = stack[sp * 64u];
      if (__uint_as_float(e.x) < -best) continue;                  // -lb fell strictly behind -best meanwhile
      cur = e.y;
    }
    if ((cur & kBvhLeaf) != 0u) {
      const uint32_t first = cur & 0x0FFFFFFFu, count = ((cur >> 28) & 3u) + 1u;
      for (uint32_t j = 0; j < count; ++j) closest_test_record(b.records + 3u * (first + j), pt, best, best_i);
      cur = kBvhEmpty;
      continue;
    }
    const float4* const nd = b.nodes + 8u * static_cast<size_t>(cur);
    const float4 lox = nd[0], loy = nd[1], loz = nd[2], hix = nd[3], hiy = nd[4], hiz = nd[5], refs = nd[6], cm = nd[7];
    const float L[3][4] = {{lox.x, lox.y, lox.z, lox.w}, {loy.x, loy.y, loy.z, loy.w}, {loz.x, loz.y, loz.z, loz.w}};
    const float Hh[3][4] = {{hix.x, hix.y, hix.z, hix.w}, {hiy.x, hiy.y, hiy.z, hiy.w}, {hiz.x, hiz.y, hiz.z, hiz.w}};
    const float cmax[4] = {cm.x, cm.y, cm.z, cm.w};
    uint32_t ref[4] = {__float_as_uint(refs.x), __float_as_uint(refs.y), __float_as_uint(refs.z), __float_as_uint(refs.w)};
    float good[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float pad = rho_c * (pmax + cmax[c]);
      const float gx = fmaxf(fmaxf(fmaxf(L[0][c] - pt.x, pt.x - Hh[0][c]), 0.0f) - pad, 0.0f);
      const float gy = fmaxf(fmaxf(fmaxf(L[1][c] - pt.y, pt.y - Hh[1][c]), 0.0f) - pad, 0.0f);
      const float gz = fmaxf(fmaxf(fmaxf(L[2][c] - pt.z, pt.z - Hh[2][c]), 0.0f) - pad, 0.0f);
      const float lb = ((gx * gx + gy * gy) + gz * gz) * kClosestDeflate;
      const bool decided = finite && lb == lb;
      float g = decided ? fmaxf(-lb, -FLT_MAX) : inf;              // nearest first; an undecided child is never dropped
      if (ref[c] == kBvhEmpty || (decided && lb > best)) { ref[c] = kBvhEmpty; g = -inf; }
      good[c] = g;
    }
    // nearest first (a 5-exchange network); an empty reference carries -inf, a visited one at least -FLT_MAX
#define RT_CP_CSWAP(i, j)                                                                             \
    if (good[i] < good[j]) { const float tg = good[i]; good[i] = good[j]; good[j] = tg;               \
                             const uint32_t tr = ref[i]; ref[i] = ref[j]; ref[j] = tr; }
    RT_CP_CSWAP(0, 1) RT_CP_CSWAP(2, 3) RT_CP_CSWAP(0, 2) RT_CP_CSWAP(1, 3) RT_CP_CSWAP(1, 2)
#undef RT_CP_CSWAP
    cur = ref[0];
    auto push = [&](float g, uint32_t r) {
      if (r == kBvhEmpty) return;
      if (sp < b.stack_cap) { stack[sp * 64u] = make_uint2(__float_as_uint(g), r); ++sp; }
      else overflow = true;                                        // (cannot happen: the capacity is 3 x the tree's depth)
    };
    push(good[3], ref[3]); push(good[2], ref[2]); push(good[1], ref[1]);   // the nearer of them on top
  }
  if (overflow) {                                                  // an entry was not kept: every leaf record, from the start
    best = q.w; best_i = -1;
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) closest_test_record(b.records + 3u * j, pt, best, best_i);
  }
  for (uint32_t j = 0; j < b.n_always; ++j) closest_test_record(b.records + 3u * (b.n_leaf_records + j), pt, best, best_i);
  hits[i] = closest_finish(p, pt, best, best_i);
}

hipError_t launch_closest(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* pts, float4* hits,
                          hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (pts == nullptr || hits == nullptr) return hipErrorInvalidValue;
  const float4* const p4 = reinterpret_cast<const float4*>(pts);
  if (b != nullptr) {                                              // one wave per block, lane = point, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(closest_bvh_kernel, n, 64u, 64u, lds, st, p, *b, rho_c, n, p4, hits);
  }
  return launch_blocks(closest_kernel, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, p4, hits);
}

}  // namespace rtk
