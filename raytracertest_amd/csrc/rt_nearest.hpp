// rt_nearest.hpp -- the k-nearest point query (rt_tracer_closest_all*): the max_hits nearest primitives of the
// tracer's scene to point i within that point's own squared search radius, in ascending (t, prim) order, optionally only those
// that sort strictly behind a caller's cursor.  Included by rt_kernels.hip only, behind rt_closest.hpp.
//
// Candidates, arithmetic and acceptance are rt_closest.hpp's word for word: closest_triangle on the record the renderer
// intersects, s = |sqrt(w.w) - radius|, t = s*s for a sphere; one arithmetic for both math modes; accepted when t <= d2max in
// plain fp32 (a NaN t never; a NaN or negative d2max accepts nothing).  The cursor (after[i], where its prim is not -1) accepts
// a candidate only if  t > after.t  or  t == after.t && prim > after.prim  (int32); a NaN after.t accepts nothing.  It is
// applied before the insert and takes no pruning decision.
//
// The list is rt_allhits.hpp's: CAP pairs (t, prim) in registers behind compile-time indices, the leading CAP - max_hits slots
// pinned at (-inf, -1), the last slot's t the bound the traversal prunes with (+inf while the list is not full).  u and v are
// recomputed from the triangle's record when a row is written out: the same operations on the same operands, the same bits.
//
// nearest_kernel<CAP> (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = point, spheres after the triangles.
//
// nearest_bvh_kernel<CAP> (RT_QUERY_BVH): closest_bvh_kernel's walk -- the same pad, lb, deflation, NaN and non-finite rules,
// five-exchange ordering, LDS stack and overflow fallback -- against  bound = min(d2max, t_last).  A child is skipped only when
// lb > bound STRICTLY (a tie may hide a lower index that displaces the last slot); a popped entry is dropped when its lb has
// fallen strictly behind bound.  The invariant: every record inside a skipped child computes t >= lb > bound, so it is either
// not accepted (t > d2max) or sorts behind a full list's last entry, and the list only ever tightens.
//
// nearest_bvh_kernel keeps the walk in its own text -- the loop, the node unpack and the ordering network are A SECOND COPY of
// rt_bvh_walk.hpp's bvh_walk: change them together.  On the shared function this kernel measured slower than its
// parent by more than the parent's own run-to-run spread, in every shape of the function that was tried.
#pragma once
#include "rt_closest.hpp"

namespace rtk {

// the continuation cursor of one point: has == false accepts every candidate
struct NearestCursor {
  float t;
  int prim;
  bool has;
};

__device__ __forceinline__ NearestCursor nearest_cursor(const float4* __restrict__ after, size_t i, bool valid) {
  NearestCursor c = {0.0f, -1, false};
  if (after != nullptr && valid) {
    const float4 a = after[i];
    c.t = a.x; c.prim = __float_as_int(a.w); c.has = c.prim != -1;
  }
  return c;
}

// one candidate: the radius, the cursor, the list
template <int CAP>
__device__ __forceinline__ void nearest_keep(float t, int prim, float d2max, const NearestCursor& c, float (&lt)[CAP], int (&lp)[CAP]) {
  const bool behind = (!c.has) | (t > c.t) | ((t == c.t) & (prim > c.prim));
  if ((t <= d2max) & behind) allhits_insert<CAP>(lt, lp, t, prim);
}

template <int CAP>
__device__ __forceinline__ void nearest_spheres(const TraceParams& p, V3 pt, float d2max, const NearestCursor& c, float (&lt)[CAP],
                                                int (&lp)[CAP]) {
  using M = Math<false>;
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    const float4 sph = p.spheres[si];
    const V3 w = rtd::sub(pt, {sph.x, sph.y, sph.z});
    const float s = fabsf(__builtin_sqrtf(M::dot(w, w)) - sph.w);
    nearest_keep<CAP>(s * s, static_cast<int>(p.n_tris + si), d2max, c, lt, lp);
  }
}

// The point's row: the last max_hits slots in order, u and v of a triangle from its record, then records {0, 0, 0, -1}; and
// its count.  The list is consumed from the front (slot 0 is taken, the rest moves up: compile-time indices).
template <int CAP>
__device__ __forceinline__ void nearest_store(const TraceParams& p, V3 pt, float (&lt)[CAP], int (&lp)[CAP], uint32_t max_hits,
                                              float4* __restrict__ row, uint32_t* __restrict__ count) {
  const uint32_t nt = p.n_tris;
  uint32_t cnt = 0u;
#pragma unroll 1
  for (uint32_t s = 0; s < static_cast<uint32_t>(CAP); ++s) {
    const float t0 = lt[0];
    const int prim = lp[0];
#pragma unroll
    for (int k = 0; k + 1 < CAP; ++k) { lt[k] = lt[k + 1]; lp[k] = lp[k + 1]; }
    if (s + max_hits < static_cast<uint32_t>(CAP)) continue;       // a leading (-inf, -1) slot (uniform: max_hits is)
    float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
    if (prim != kAllHitsEmpty) {
      ++cnt;
      h.x = t0;
      h.w = __int_as_float(prim);
      if (static_cast<uint32_t>(prim) < nt) {
        const float4 A0 = p.tri_a[2 * prim], A1 = p.tri_a[2 * prim + 1];
        float t = 0.0f, u = 0.0f, v = 0.0f;
        closest_triangle(pt, {A1.z, A1.w, p.tri_b[prim]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
        h.y = u; h.z = v;
      }
    }
    row[s + max_hits - static_cast<uint32_t>(CAP)] = h;
  }
  *count = cnt;
}

template <int CAP>
__global__ __launch_bounds__(256, 4) void nearest_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ pts,
                                                          const float4* __restrict__ after, uint32_t max_hits,
                                                          float4* __restrict__ hits, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first point of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  float4 q = {0.0f, 0.0f, 0.0f, -1.0f};                            // padding lanes accept nothing
  if (tid < nb) q = pts[base + tid];
  const V3 pt = {q.x, q.y, q.z};
  const float d2max = q.w;
  const NearestCursor cur = nearest_cursor(after, base + tid, tid < nb);
  const bool active = (d2max >= 0.0f) & !(cur.has & (cur.t != cur.t));   // a NaN or negative d2max, or a NaN cursor: nothing

  float lt[CAP];
  int lp[CAP];
  allhits_init<CAP>(lt, lp, max_hits);

  // the triangles; every chunk is scanned, by the waves that hold a point that accepts
  scan_triangles<ScanMode::SkipIdleWaves>(p, s_mem, [&] { return active; }, [&](const float4 A0, const float4 A1, auto z, int prim) {
    float t, u, v;
    closest_triangle(pt, {A1.z, A1.w, z()}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
    if (active) nearest_keep<CAP>(t, prim, d2max, cur, lt, lp);
  });
  if (active) nearest_spheres<CAP>(p, pt, d2max, cur, lt, lp);

  if (tid < nb) nearest_store<CAP>(p, pt, lt, lp, max_hits, hits + (base + tid) * max_hits, counts + base + tid);
}

// one record against one point
template <int CAP>
__device__ __forceinline__ void nearest_test_record(const float4* __restrict__ rec, V3 pt, float d2max, const NearestCursor& c,
                                                    float (&lt)[CAP], int (&lp)[CAP]) {
  const float4 A0 = rec[0], A1 = rec[1], B = rec[2];
  float t, u, v;
  closest_triangle(pt, {A1.z, A1.w, B.x}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, t, u, v);
  nearest_keep<CAP>(t, __float_as_int(B.y), d2max, c, lt, lp);
}

template <int CAP>
__global__ __launch_bounds__(64) void nearest_bvh_kernel(const TraceParams p, const BvhParams b, float rho_c, uint32_t n,
                                                          const float4* __restrict__ pts, const float4* __restrict__ after,
                                                          uint32_t max_hits, float4* __restrict__ hits, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const float4 q = pts[i];
  const V3 pt = {q.x, q.y, q.z};
  const float d2max = q.w;
  const NearestCursor cs = nearest_cursor(after, i, true);
  const bool active = (d2max >= 0.0f) & !(cs.has & (cs.t != cs.t));      // a NaN or negative d2max, or a NaN cursor: nothing

  float lt[CAP];
  int lp[CAP];
  allhits_init<CAP>(lt, lp, max_hits);

  uint2* const stack = reinterpret_cast<uint2*>(s_mem) + lane;     // entry e at stack[e * 64]
  const float inf = __builtin_inff();
  const bool finite = fabsf(pt.x) < inf && fabsf(pt.y) < inf && fabsf(pt.z) < inf;
  const float pmax = fmaxf(fmaxf(fabsf(pt.x), fabsf(pt.y)), fabsf(pt.z));
  uint32_t sp = 0u;
  uint32_t cur = (b.n_nodes != 0u && active) ? 0u : kBvhEmpty;
  bool overflow = false;
  for (;;) {
    if (cur == kBvhEmpty) {
      if (sp == 0u) break;
      --sp;
      const uint2 e = stack[sp * 64u];
      // -lb fell strictly behind -bound meanwhile (an empty last slot has t = +inf: bound is d2max then)
      if (__uint_as_float(e.x) < -fminf(d2max, lt[CAP - 1])) continue;
      cur = e.y;
    }
    if ((cur & kBvhLeaf) != 0u) {
      const uint32_t first = cur & 0x0FFFFFFFu, count = ((cur >> 28) & 3u) + 1u;
      for (uint32_t j = 0; j < count; ++j) nearest_test_record<CAP>(b.records + 3u * (first + j), pt, d2max, cs, lt, lp);
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
    const float bound = fminf(d2max, lt[CAP - 1]);                 // t_last is +inf while the list is not full
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float pad = rho_c * (pmax + cmax[c]);
      const float gx = fmaxf(fmaxf(fmaxf(L[0][c] - pt.x, pt.x - Hh[0][c]), 0.0f) - pad, 0.0f);
      const float gy = fmaxf(fmaxf(fmaxf(L[1][c] - pt.y, pt.y - Hh[1][c]), 0.0f) - pad, 0.0f);
      const float gz = fmaxf(fmaxf(fmaxf(L[2][c] - pt.z, pt.z - Hh[2][c]), 0.0f) - pad, 0.0f);
      const float lb = ((gx * gx + gy * gy) + gz * gz) * kClosestDeflate;
      const bool decided = finite && lb == lb;
      float g = decided ? fmaxf(-lb, -FLT_MAX) : inf;              // nearest first; an undecided child is never dropped
      if (ref[c] == kBvhEmpty || (decided && lb > bound)) { ref[c] = kBvhEmpty; g = -inf; }
      good[c] = g;
    }
    // nearest first (a 5-exchange network); an empty reference carries -inf, a visited one at least -FLT_MAX
#define RT_NN_CSWAP(i, j)                                                                             \
    if (good[i] < good[j]) { const float tg = good[i]; good[i] = good[j]; good[j] = tg;               \
                             const uint32_t tr = ref[i]; ref[i] = ref[j]; ref[j] = tr; }
    RT_NN_CSWAP(0, 1) RT_NN_CSWAP(2, 3) RT_NN_CSWAP(0, 2) RT_NN_CSWAP(1, 3) RT_NN_CSWAP(1, 2)
#undef RT_NN_CSWAP
    cur = ref[0];
    auto push = [&](float g, uint32_t r) {
      if (r == kBvhEmpty) return;
      if (sp < b.stack_cap) { stack[sp * 64u] = make_uint2(__float_as_uint(g), r); ++sp; }
      else overflow = true;                                        // (cannot happen: the capacity is 3 x the tree's depth)
    };
    push(good[3], ref[3]); push(good[2], ref[2]); push(good[1], ref[1]);   // the nearer of them on top
  }
  if (overflow) {                                                  // an entry was not kept: every leaf record, from an empty list
    allhits_init<CAP>(lt, lp, max_hits);
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) nearest_test_record<CAP>(b.records + 3u * j, pt, d2max, cs, lt, lp);
  }
  if (active) {
    for (uint32_t j = 0; j < b.n_always; ++j) nearest_test_record<CAP>(b.records + 3u * (b.n_leaf_records + j), pt, d2max, cs, lt, lp);
    nearest_spheres<CAP>(p, pt, d2max, cs, lt, lp);
  }
  nearest_store<CAP>(p, pt, lt, lp, max_hits, hits + i * max_hits, counts + i);
}

// CAP = 4 for max_hits 1 .. 4, else 16, in both forms
hipError_t launch_nearest(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* pts, const float4* after,
                          uint32_t max_hits, float4* hits, uint32_t* counts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (max_hits == 0u || max_hits > kAllHitsMax || pts == nullptr || hits == nullptr || counts == nullptr) return hipErrorInvalidValue;
  const float4* const p4 = reinterpret_cast<const float4*>(pts);
  if (b != nullptr) {                                              // one wave per block, lane = point, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(max_hits <= 4u ? nearest_bvh_kernel<4> : nearest_bvh_kernel<16>, n, 64u, 64u, lds, st, p, *b, rho_c, n, p4, after,
                         max_hits, hits, counts);
  }
  return launch_blocks(max_hits <= 4u ? nearest_kernel<4> : nearest_kernel<16>, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, p4,
                       after, max_hits, hits, counts);
}

}  // namespace rtk
