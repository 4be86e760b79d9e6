// rt_bvh.hpp -- ray queries through the scene's bounding volume hierarchy (RT_QUERY_BVH).  Included by
// rt_kernels.hip only, behind rt_query.hpp.  It is built from the same device functions as the scan (pinhole, hit_sphere,
// hit_triangle_exact); the few lines that put a ray's result together (finish_query_hit) are stated here a second time and
// query_kernel keeps its own text: moving them into a function both kernels call was tried in nine shapes, and every one
// changed the scan kernel's schedule (tools/isa_diff.py), which this mode promises to leave as it is.
//
// Shape: one wave per block, lane = ray.  Each lane walks the 4-wide tree of rt_bvh_host.hpp on its own: a node is eight
// 16-byte loads (128 bytes, one line), the four child boxes are tested against the ray's LINE, the children worth a visit are
// ordered (far first under the reference's farthest-hit rule, near first under RT_FLAG_NEAREST_HIT), the best is entered and
// the others wait on the lane's stack.  The stack lives in LDS as 8-byte entries {goodness, reference} at entry * 64 + lane:
// a wave's pushes and pops touch 64 consecutive entries, free of bank conflicts (a runtime-indexed private array would live
// in scratch).  Its capacity is 3 x the tree's depth (three waiting siblings per level), which the builder bounds.
//
// Box test (restated in numpy by tests/query_accel_expect.py; fp32, operation by operation):
//   pad = rho * (max|o| + cmax)                 cmax: the largest |coordinate| of the child's box, from the node
//   t1 = ((lo - pad) - o) * (1 / d), t2 = ((hi + pad) - o) * (1 / d) per axis; enter = max of the min(t1, t2), exit = min
//   of the max(t1, t2)
//   skipped when  exit < enter,  or  exit < best t  (nearest rule: enter > best t, or exit <= 0)  -- strictly: a tie is visited,
//   a lower upload index may be waiting in it.  A NaN among the t1, t2 (0 * inf: the ray runs inside a slab's plane), or a ray
//   with a non-finite component, takes no pruning decision: the child is visited.
// A popped entry is dropped when its goodness (exit, or -enter) has fallen strictly behind the best t found meanwhile.
//
// Leaves: each lane tests its own triangle with hit_triangle_exact (the per-lane statement of the scan's test, same bits), and
// keeps the largest t, ties to the LOWEST upload index (nearest: the smallest t > 0, ties to the lowest index) -- the scan's
// first-scanned-wins rule in a form that does not depend on the order of the visits.  The always-tested list (triangles with
// a non-finite record) follows under the same rule.
//
// query_bvh_kernel keeps the walk in its own text -- the loop, the node unpack and the ordering network are A SECOND COPY of
// rt_bvh_walk.hpp's bvh_walk, its box test of bvh_slab: change them together.  On the shared function this kernel measured slower than its
// parent by more than the parent's own run-to-run spread, in every shape of the function that was tried.
#pragma once
#include "rt_bvh_walk.hpp"

namespace rtk {

// One ray's result from its best triangle (dist, win; win < 0: none): the spheres, scanned after the triangles by the trace
// kernel's rule (rt_trace.hpp), and the winner's u, v recomputed from its record (Kernels.cuh:50,57).
template <bool FMA>
__device__ __forceinline__ float4 finish_query_hit(const TraceParams& p, V3 o, V3 d, bool nearest, float dist, int win) {
  const uint32_t nt = p.n_tris;
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    float t = 0.0f;
    if (hit_sphere<FMA>(o, d, p.spheres[si], t) && (nearest ? (t > 0.0f && t < dist) : dist < t)) {
      dist = t;
      win = static_cast<int>(nt + si);
    }
  }
  float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
  if (win >= 0) {
    h.x = dist;
    h.w = __int_as_float(win);
    if (static_cast<uint32_t>(win) < nt) {
      const float4 A0 = p.tri_a[2 * win], A1 = p.tri_a[2 * win + 1];
      float t = 0.0f, u = 0.0f, v = 0.0f;
      int stage;
      (void)hit_triangle_exact<FMA>(o, d, {A1.z, A1.w, p.tri_b[win]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, RT_EPS, t, u, v, stage);
      h.y = u; h.z = v;
    }
  }
  return h;
}

// one record against one ray, under the order-free statement of the scan's rule
template <bool FMA>
__device__ __forceinline__ void bvh_test_record(const float4* __restrict__ rec, V3 o, V3 d, bool nearest, float& best_t, int& best_i) {
  const float4 A0 = rec[0], A1 = rec[1], B = rec[2];
  float t = 0.0f, u = 0.0f, v = 0.0f;
  int stage;
  if (!hit_triangle_exact<FMA>(o, d, {A1.z, A1.w, B.x}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, RT_EPS, t, u, v, stage)) return;
  const int idx = __float_as_int(B.y);
  const bool better = nearest ? (t > 0.0f && t < best_t) : (best_t < t);
  if (better || (t == best_t && idx < best_i)) {      // (best_i = -1 before the first hit: no tie with the initial value)
    best_t = t;
    best_i = idx;
  }
}

template <bool FMA>
__global__ __launch_bounds__(64) void query_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n, const float* __restrict__ rays,
                                                        const uint32_t* __restrict__ pixels, float* __restrict__ rays_out,
                                                        float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 64u;
  const size_t i = base + lane;
  const bool live = i < n;
  V3 o = {0.0f, 0.0f, 0.0f}, d = {0.0f, 0.0f, 0.0f};
  if (live) {
    if (pixels == nullptr) {
      const float* const r = rays + 6u * i;
      o = {r[0], r[1], r[2]}; d = {r[3], r[4], r[5]};
    } else {                                                       // the pixel's pinhole ray, as the trace kernel makes it
      pinhole<FMA>(p, pixels[2u * i], pixels[2u * i + 1u], o, d);
      if (rays_out != nullptr) {
        float* const out = rays_out + 6u * i;
        out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = d.x; out[4] = d.y; out[5] = d.z;
      }
    }
  }
  const bool nearest = (p.flags & TRACE_NEAREST_HIT) != 0u;
  float best_t = nearest ? FLT_MAX : -FLT_MAX;                     // Kernels.cuh:73
  int best_i = -1;

  if (live) {
    uint2* const stack = reinterpret_cast<uint2*>(s_mem) + lane;   // entry e at stack[e * 64]
    const float inf = __builtin_inff();
    const bool finite = fabsf(o.x) < inf && fabsf(o.y) < inf && fabsf(o.z) < inf && fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf;
    const V3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    const float omax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    uint32_t sp = 0u;
    uint32_t cur = b.n_nodes != 0u ? 0u : kBvhEmpty;
    bool overflow = false;
    for (;;) {
      if (cur == kBvhEmpty) {
        if (sp == 0u) break;
        --sp;
        const uint2 e = stack[sp * 64u];
        if (__uint_as_float(e.x) < (nearest ? -best_t : best_t)) continue;   // fell strictly behind the best meanwhile
        cur = e.y;
      }
      if ((cur & kBvhLeaf) != 0u) {
        const uint32_t first = cur & 0x0FFFFFFFu, count = ((cur >> 28) & 3u) + 1u;
        for (uint32_t j = 0; j < count; ++j) bvh_test_record<FMA>(b.records + 3u * (first + j), o, d, nearest, best_t, best_i);
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
      const float lim = nearest ? -best_t : best_t;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float pad = b.rho * (omax + cmax[c]);
        const float t1x = ((L[0][c] - pad) - o.x) * inv.x, t2x = ((Hh[0][c] + pad) - o.x) * inv.x;
        const float t1y = ((L[1][c] - pad) - o.y) * inv.y, t2y = ((Hh[1][c] + pad) - o.y) * inv.y;
        const float t1z = ((L[2][c] - pad) - o.z) * inv.z, t2z = ((Hh[2][c] + pad) - o.z) * inv.z;
        const bool nan = __builtin_isunordered(t1x, t2x) || __builtin_isunordered(t1y, t2y) || __builtin_isunordered(t1z, t2z);
        const float enter = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
        const float exit = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
        float g = nearest ? -enter : exit;
        const bool skip = (exit < enter) || (g < lim) || (nearest && exit <= 0.0f);
        const bool decided = finite && !nan;
        g = decided ? fmaxf(g, -FLT_MAX) : inf;
        if (ref[c] == kBvhEmpty || (decided && skip)) { ref[c] = kBvhEmpty; g = -inf; }
        good[c] = g;
      }
      // best first (a 5-exchange network); an empty reference carries -inf, a visited one at least -FLT_MAX
#define RT_BVH_CSWAP(i, j)                                                                            \
      if (good[i] < good[j]) { const float tg = good[i]; good[i] = good[j]; good[j] = tg;             \
                               const uint32_t tr = ref[i]; ref[i] = ref[j]; ref[j] = tr; }
      RT_BVH_CSWAP(0, 1) RT_BVH_CSWAP(2, 3) RT_BVH_CSWAP(0, 2) RT_BVH_CSWAP(1, 3) RT_BVH_CSWAP(1, 2)
#undef RT_BVH_CSWAP
      cur = ref[0];
      auto push = [&](float g, uint32_t r) {
        if (r == kBvhEmpty) return;
        if (sp < b.stack_cap) { stack[sp * 64u] = make_uint2(__float_as_uint(g), r); ++sp; }
        else overflow = true;                                      // (cannot happen: the capacity is 3 x the tree's depth)
      };
      push(good[3], ref[3]); push(good[2], ref[2]); push(good[1], ref[1]);   // the better of them on top
    }
    if (overflow) {                                                // an entry was not kept: every leaf record, in order
      best_t = nearest ? FLT_MAX : -FLT_MAX; best_i = -1;
      for (uint32_t j = 0; j < b.n_leaf_records; ++j) bvh_test_record<FMA>(b.records + 3u * j, o, d, nearest, best_t, best_i);
    }
    for (uint32_t j = 0; j < b.n_always; ++j)
      bvh_test_record<FMA>(b.records + 3u * (b.n_leaf_records + j), o, d, nearest, best_t, best_i);
    hits[i] = finish_query_hit<FMA>(p, o, d, nearest, best_t, best_i);
  }
}

// the ray query's one launch (rt_query.hpp's query_kernel is the scan: it is launched from here, where both kernels are seen)
hipError_t launch_query(const TraceParams& p, const BvhParams* b, bool fma, int K, uint32_t n, const float* rays, const uint32_t* pixels,
                        float* rays_out, float4* hits, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (hits == nullptr || (rays == nullptr && pixels == nullptr)) return hipErrorInvalidValue;
  if (b != nullptr) {                                              // one wave per block, lane = ray, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(fma ? query_bvh_kernel<true> : query_bvh_kernel<false>, n, 64u, 64u, lds, st, p, *b, n, rays, pixels, rays_out, hits);
  }
  if (K != 1 && K != 2 && K != 4) return hipErrorInvalidValue;
  const auto kern = fma ? (K == 1 ? query_kernel<true, 1> : K == 2 ? query_kernel<true, 2> : query_kernel<true, 4>)
                        : (K == 1 ? query_kernel<false, 1> : K == 2 ? query_kernel<false, 2> : query_kernel<false, 4>);
  return launch_blocks(kern, n, 256u * K, 256u, query_lds_bytes(p.n_tris, K), st, p, n, rays, pixels, rays_out, hits);
}

}  // namespace rtk
