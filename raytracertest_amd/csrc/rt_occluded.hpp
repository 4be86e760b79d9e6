// rt_occluded.hpp -- the visibility query (rt_tracer_occluded*): is ray i blocked by ANY primitive of the
// scene with tmin <= t <= tmax?  Included by rt_kernels.hip only, behind rt_bvh.hpp.  The triangle stages are stated here
// again (occluded_test_triangle beside rt_trace.hpp's test_triangle), because query_kernel keeps its schedule only while its
// text is its own (rt_bvh.hpp).
//
// A "hit" is the reference's HitTriangle returning true (Kernels.cuh:29-65) and its t is the value of :63, a sphere's the one t
// of hit_sphere; the interval is closed and compared in plain fp32 (a NaN t or bound, or tmin > tmax, never occludes).  The
// answer is an OR over the primitives: no winner, no order, no tie rule, and a ray is finished at its first accepted hit.
//
// occluded_kernel (RT_QUERY_SCAN): the scan of rt_scan.hpp in its stop-when-idle mode, K rays per lane (ray k * 256 + lane of
// the block): a finished ray leaves the ballots of the triangle stages, and a lane is open while one of its rays is not
// finished.  Rays are two 16-byte loads each, the answers one byte per ray (a wave's 64 lanes store 64 consecutive bytes).
// Padding lanes (ray index >= n) start finished.
//
// occluded_bvh_kernel (RT_QUERY_BVH): one wave per block, lane = ray, the walk of rt_bvh_walk.hpp as an any-hit traversal.  A
// child is skipped when  exit < enter,  exit < tmin  or  enter > tmax  (strictly: a tie is visited).  There is no best t, so a
// stack entry is the child's reference alone and no popped entry is judged again.  The child whose span overlaps [tmin, tmax]
// most is entered first.  The always-tested list comes before the tree (it may end the walk before it starts); a ray with a
// non-finite component or a zero direction, or a child with a NaN in its box arithmetic, takes no pruning decision.
// occluded_prune and occluded_child are the ray's side of that rule; exposure_bvh_kernel (rt_exposure.hpp) walks with them too.
#pragma once
#include "rt_bvh.hpp"

namespace rtk {

// One triangle against the unfinished rays of every lane: test_triangle's stages A-D (rt_trace.hpp: the same conservative
// wave-uniform rejections, the same operations in stage D, so t has the renderer's bits), a finished ray counting as rejected.
template <bool FMA, int K>
__device__ __forceinline__ void occluded_test_triangle(const float4 A0, const float4 A1, const float v0z, const V3 (&o)[K],
                                                       const V3 (&d)[K], const float (&tmin)[K], const float (&tmax)[K],
                                                       bool (&done)[K]) {
  using M = Math<FMA>;
  const V3 e2 = {A0.x, A0.y, A0.z}, e1 = {A0.w, A1.x, A1.y};
  // stage A: pv = cross(dir, e2), det = dot(e1, pv), culling (:39-45)
  V3 pv[K];
  float det[K];
  unsigned long long mk[K];
  unsigned long long live = 0ull;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    pv[k] = M::cross(d[k], e2);
    det[k] = M::dot(e1, pv[k]);
    mk[k] = __builtin_amdgcn_ballot_w64(!done[k] && !(det[k] < RT_EPS));
    live |= mk[k];
  }
  if (live == 0ull) return;
  // stage B: U = dot(origin - v0, pv) (:49-50), conservative u rejection
  const V3 v0 = {A1.z, A1.w, v0z};
  V3 tv[K];
  float U[K], thi[K], tlo[K];
  live = 0ull;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    tv[k] = rtd::sub(o[k], v0);
    U[k] = M::dot(tv[k], pv[k]);
    thi[k] = det[k] * 1.0001f;
    tlo[k] = det[k] * -1e-6f;
    mk[k] &= __builtin_amdgcn_ballot_w64(!(U[k] > thi[k])) & __builtin_amdgcn_ballot_w64(!(U[k] < tlo[k]));
    live |= mk[k];
  }
  if (live == 0ull) return;
  // stage C: V = dot(dir, cross(tv, e1)) (:56-57), conservative v rejection
  V3 qv[K];
  float V[K];
  live = 0ull;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    qv[k] = M::cross(tv[k], e1);
    V[k] = M::dot(d[k], qv[k]);
    mk[k] &= __builtin_amdgcn_ballot_w64(!(V[k] < tlo[k])) & __builtin_amdgcn_ballot_w64(!((U[k] + V[k]) > thi[k]));
    live |= mk[k];
  }
  if (live == 0ull) return;
  // stage D: the reference's exact tests (:42-63) wherever a ray may hit, then the closed interval
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (mk[k] != 0ull) {
      const float inv = 1.0f / det[k];                             // :47
      const float u = U[k] * inv;                                  // :50
      const float v = V[k] * inv;                                  // :57
      const float t = M::dot(e2, qv[k]) * inv;                     // :63
      const bool miss = (det[k] < RT_EPS) | (u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f);
      done[k] = done[k] | ((!miss) & (tmin[k] <= t) & (t <= tmax[k]));
    }
  }
}

template <bool FMA, int K>
__global__ __launch_bounds__(256, 4) void occluded_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ segs,
                                                           uint8_t* __restrict__ occluded) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * (256u * K);      // first ray of the block
  const uint32_t nb = (n - base < 256u * K) ? static_cast<uint32_t>(n - base) : 256u * K;

  V3 o[K], d[K];
  float tmin[K], tmax[K];
  bool done[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t r = static_cast<uint32_t>(k) * 256u + tid;
    float4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < nb) { s0 = segs[2u * (base + r)]; s1 = segs[2u * (base + r) + 1u]; }
    o[k] = {s0.x, s0.y, s0.z};
    d[k] = {s0.w, s1.x, s1.y};
    tmin[k] = s1.z; tmax[k] = s1.w;
    done[k] = !(r < nb);                                           // padding lanes start finished
  }

  // the spheres first: they are few (hit_sphere's one t)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    for (uint32_t si = 0; si < p.n_spheres; ++si) {
      float t = 0.0f;
      if (!done[k] && hit_sphere<FMA>(o[k], d[k], p.spheres[si], t) && tmin[k] <= t && t <= tmax[k]) done[k] = true;
    }
  }

  // the triangles, until every ray of the block is finished
  const auto open = [&] {
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) any = any || !done[k];
    return any;
  };
  scan_triangles<ScanMode::StopWhenIdle>(p, s_mem, open, [&](const float4 A0, const float4 A1, auto z, int) {
    occluded_test_triangle<FMA, K>(A0, A1, z(), o, d, tmin, tmax, done);
  });

#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t r = static_cast<uint32_t>(k) * 256u + tid;
    if (r < nb) occluded[base + r] = done[k] ? 1u : 0u;
  }
}

// one record against one ray: the exact test, then the closed interval
template <bool FMA>
__device__ __forceinline__ bool occluded_test_record(const float4* __restrict__ rec, V3 o, V3 d, float tmin, float tmax) {
  const BvhRecord r = bvh_record(rec);
  float t = 0.0f, u = 0.0f, v = 0.0f;
  int stage;
  if (!hit_triangle_exact<FMA>(o, d, r.v0, r.e1, r.e2, RT_EPS, t, u, v, stage)) return false;
  return tmin <= t && t <= tmax;
}

// what the any-hit walk keeps of a ray besides the segment: whether it prunes at all, 1 / d, max|o|
struct OccludedPrune {
  bool prunes;
  V3 inv;
  float omax;
};

__device__ __forceinline__ OccludedPrune occluded_prune(V3 o, V3 d) {
  const float inf = __builtin_inff();
  const bool finite = fabsf(o.x) < inf && fabsf(o.y) < inf && fabsf(o.z) < inf && fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf;
  return {finite && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f), {1.0f / d.x, 1.0f / d.y, 1.0f / d.z},
          fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z))};
}

// the goodness of child c (bvh_walk's convention): the overlap of the child's span with the interval
__device__ __forceinline__ float occluded_child(const BvhNode& nd, int c, float rho, const OccludedPrune& q, V3 o, float tmin, float tmax) {
  const float inf = __builtin_inff();
  float enter, exit;
  const bool nan = bvh_slab(nd, c, rho * (q.omax + nd.cmax[c]), o, q.inv, enter, exit);
  const bool skip = (exit < enter) || (exit < tmin) || (enter > tmax);
  // (inf - inf: a NaN, which fmaxf drops)
  return !(q.prunes && !nan) ? inf : skip ? -inf : fmaxf(fminf(exit, tmax) - fmaxf(enter, tmin), -FLT_MAX);
}

template <bool FMA>
__global__ __launch_bounds__(64) void occluded_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n,
                                                           const float4* __restrict__ segs, uint8_t* __restrict__ occluded) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const float4 s0 = segs[2u * i], s1 = segs[2u * i + 1u];
  const V3 o = {s0.x, s0.y, s0.z}, d = {s0.w, s1.x, s1.y};
  const float tmin = s1.z, tmax = s1.w;
  bool done = false;

  for (uint32_t si = 0; si < p.n_spheres && !done; ++si) {
    float t = 0.0f;
    done = hit_sphere<FMA>(o, d, p.spheres[si], t) && tmin <= t && t <= tmax;
  }
  for (uint32_t j = 0; j < b.n_always && !done; ++j)
    done = occluded_test_record<FMA>(b.records + 3u * (b.n_leaf_records + j), o, d, tmin, tmax);

  const OccludedPrune q = occluded_prune(o, d);
  const bool overflow = bvh_walk<64u, false>(
      b, s_mem, lane, !done, [&](const BvhNode& nd, int c) { return occluded_child(nd, c, b.rho, q, o, tmin, tmax); },
      [&](const float4* rec) { return done = occluded_test_record<FMA>(rec, o, d, tmin, tmax); }, [](float) { return false; });
  if (overflow && !done) {                                         // an entry was not kept: every leaf record
    for (uint32_t j = 0; j < b.n_leaf_records && !done; ++j) done = occluded_test_record<FMA>(b.records + 3u * j, o, d, tmin, tmax);
  }
  occluded[i] = done ? 1u : 0u;
}

hipError_t launch_occluded(const TraceParams& p, const BvhParams* b, bool fma, int K, uint32_t n, const float* segs, uint8_t* occluded,
                           hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (segs == nullptr || occluded == nullptr) return hipErrorInvalidValue;
  const float4* const s4 = reinterpret_cast<const float4*>(segs);
  if (b != nullptr) {                                              // one wave per block, lane = ray, the reference alone on the stack
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, false);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(fma ? occluded_bvh_kernel<true> : occluded_bvh_kernel<false>, n, 64u, 64u, lds, st, p, *b, n, s4, occluded);
  }
  if (K != 1 && K != 2 && K != 4) return hipErrorInvalidValue;
  const auto kern = fma ? (K == 1 ? occluded_kernel<true, 1> : K == 2 ? occluded_kernel<true, 2> : occluded_kernel<true, 4>)
                        : (K == 1 ? occluded_kernel<false, 1> : K == 2 ? occluded_kernel<false, 2> : occluded_kernel<false, 4>);
  return launch_blocks(kern, n, 256u * K, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, s4, occluded);
}

}  // namespace rtk
