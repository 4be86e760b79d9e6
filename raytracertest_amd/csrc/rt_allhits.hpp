// rt_allhits.hpp -- the all-hits query (rt_tracer_intersect_all*): the first max_hits hits of ray i within its own
// closed t interval, in ascending (t, prim) order.  Included by rt_kernels.hip only, behind rt_occluded.hpp.  The triangle stages
// are stated here a third time, because the scan kernels keep their schedule only while their text is theirs alone (rt_bvh.hpp,
// rt_occluded.hpp).
//
// A "hit" is rt_occluded.hpp's: the reference's HitTriangle returning true (Kernels.cuh:29-65) with the t of :63, a sphere with
// the one t of hit_sphere; tmin <= t && t <= tmax in plain fp32 (a NaN t or bound, or tmin > tmax: no hit).  Order: ascending
// t, equal t (==, so -0 equals +0) by ascending prim (upload index; n_tris + i for sphere i).  The rule names no visiting order,
// so the scan and the traversal cannot disagree about it.
//
// The list: CAP pairs (t, prim) in registers, touched with compile-time indices only (a runtime-indexed private array would
// live in scratch).  A new hit replaces the LAST slot when it sorts before it and is bubbled up by CAP - 1 compare-exchanges.
// max_hits <= CAP is a runtime argument: the leading CAP - max_hits slots start as (-inf, -1), which sorts before every hit and
// is therefore never displaced, the others as (+inf, INT_MAX), which sorts behind every hit.  The wanted list is then always the
// last max_hits slots, it is full exactly when the last slot is no longer the empty pair, and the last slot's t is the t_last
// the traversal prunes with -- no runtime index anywhere.  u and v are recomputed from the triangle's record when a row is
// written out (finish_query_hit's way: same operations as the scan, same bits), so the list holds 8 bytes per hit.
//
// allhits_kernel (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = ray, two 16-byte loads per ray, stages A-D
// with the conservative wave-uniform ballots and no early exit: nothing is ever finished.  Padding lanes and rays whose
// interval is empty (a NaN bound, tmin > tmax) stay out of the ballots.
//
// allhits_kernel keeps the scan in its own text -- the chunk loop, the LDS layout, the staging and the barriers are A SECOND
// COPY of rt_scan.hpp's scan_triangles, which is the first: change them together.  On the shared function this kernel measured
// slower than its parent by more than the parent's own run-to-run spread.
//
// allhits_bvh_kernel (RT_QUERY_BVH): one wave per block, lane = ray, the walk of rt_bvh_walk.hpp with 8-byte stack entries
// {-enter, reference}.  A child is skipped when  exit < enter,  exit < tmin,  enter > tmax  or, once the list is full,
// enter > t_last  (strictly: a tie is visited, a lower prim may be waiting in it).  The nearest child (smallest enter) is
// entered first; a popped entry is dropped when its enter has fallen strictly behind t_last meanwhile.  The always-tested list
// and the spheres are tested unconditionally.  A ray with a non-finite component or a zero direction, or a child with a NaN in
// its box arithmetic, takes no pruning decision (occluded_prune).
#pragma once
#include "rt_occluded.hpp"

namespace rtk {

constexpr int kAllHitsEmpty = 0x7FFFFFFF;      // prim of an empty slot (with t = +inf): behind every hit
constexpr uint32_t kAllHitsMax = 16u;          // RT_MAX_HITS

// (ta, pa) sorts strictly before (tb, pb)
__device__ __forceinline__ bool allhits_before(float ta, int pa, float tb, int pb) {
  return (ta < tb) | ((ta == tb) & (pa < pb));
}

template <int CAP>
__device__ __forceinline__ void allhits_init(float (&lt)[CAP], int (&lp)[CAP], uint32_t max_hits) {
  const float inf = __builtin_inff();
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    const bool wanted = static_cast<uint32_t>(s) + max_hits >= static_cast<uint32_t>(CAP);
    lt[s] = wanted ? inf : -inf;
    lp[s] = wanted ? kAllHitsEmpty : -1;
  }
}

// one accepted in-interval hit into the sorted list
template <int CAP>
__device__ __forceinline__ void allhits_insert(float (&lt)[CAP], int (&lp)[CAP], float t, int prim) {
  if (allhits_before(t, prim, lt[CAP - 1], lp[CAP - 1])) {
    lt[CAP - 1] = t; lp[CAP - 1] = prim;
#pragma unroll
    for (int s = CAP - 1; s > 0; --s) {
      const bool sw = allhits_before(lt[s], lp[s], lt[s - 1], lp[s - 1]);
      const float ta = lt[s - 1], tb = lt[s];
      const int pa = lp[s - 1], pb = lp[s];
      lt[s - 1] = sw ? tb : ta; lt[s] = sw ? ta : tb;
      lp[s - 1] = sw ? pb : pa; lp[s] = sw ? pa : pb;
    }
  }
}

// The ray's row: the last max_hits slots in order, u and v of a triangle from its record (Kernels.cuh:50,57), then records
// {0, 0, 0, -1}; and its count.  The list is consumed from the front (slot 0 is taken, the rest moves up: compile-time indices).
template <bool FMA, int CAP>
__device__ __forceinline__ void allhits_store(const TraceParams& p, V3 o, V3 d, float (&lt)[CAP], int (&lp)[CAP], uint32_t max_hits,
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
        int stage;
        (void)hit_triangle_exact<FMA>(o, d, {A1.z, A1.w, p.tri_b[prim]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, RT_EPS, t, u, v, stage);
        h.y = u; h.z = v;
      }
    }
    row[s + max_hits - static_cast<uint32_t>(CAP)] = h;
  }
  *count = cnt;
}

// the spheres through the same insert (hit_sphere's one t; prim = n_tris + sphere index)
template <bool FMA, int CAP>
__device__ __forceinline__ void allhits_spheres(const TraceParams& p, V3 o, V3 d, float tmin, float tmax, bool active,
                                                float (&lt)[CAP], int (&lp)[CAP]) {
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    float t = 0.0f;
    if (active && hit_sphere<FMA>(o, d, p.spheres[si], t) && tmin <= t && t <= tmax)
      allhits_insert<CAP>(lt, lp, t, static_cast<int>(p.n_tris + si));
  }
}

template <bool FMA, int CAP>
__global__ __launch_bounds__(256, 4) void allhits_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ segs,
                                                          uint32_t max_hits, float4* __restrict__ hits, uint32_t* __restrict__ counts) {
  using M = Math<FMA>;
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first ray of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  float4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (tid < nb) { s0 = segs[2u * (base + tid)]; s1 = segs[2u * (base + tid) + 1u]; }
  const V3 o = {s0.x, s0.y, s0.z}, d = {s0.w, s1.x, s1.y};
  const float tmin = s1.z, tmax = s1.w;
  const bool active = (tid < nb) & (tmin <= tmax);                 // padding lanes and empty intervals take no part

  float lt[CAP];
  int lp[CAP];
  allhits_init<CAP>(lt, lp, max_hits);

  // the triangles, staged into LDS chunk by chunk; every chunk is scanned (rt_scan.hpp's loop in its SkipIdleWaves mode)
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
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) continue;     // no ray of this wave can hit; it still helps staging
    for (uint32_t j = 0; j < cn; ++j) {
      const float4 A0 = sA[2u * j], A1 = sA[2u * j + 1u];
      const V3 e2 = {A0.x, A0.y, A0.z}, e1 = {A0.w, A1.x, A1.y};
      // stage A: pv = cross(dir, e2), det = dot(e1, pv), culling (:39-45)
      const V3 pv = M::cross(d, e2);
      const float det = M::dot(e1, pv);
      unsigned long long mk = __builtin_amdgcn_ballot_w64(active && !(det < RT_EPS));
      if (mk == 0ull) continue;
      // stage B: U = dot(origin - v0, pv) (:49-50), conservative u rejection
      const V3 v0 = {A1.z, A1.w, sB[j]};
      const V3 tv = rtd::sub(o, v0);
      const float U = M::dot(tv, pv);
      const float thi = det * 1.0001f, tlo = det * -1e-6f;
      mk &= __builtin_amdgcn_ballot_w64(!(U > thi)) & __builtin_amdgcn_ballot_w64(!(U < tlo));
      if (mk == 0ull) continue;
      // stage C: V = dot(dir, cross(tv, e1)) (:56-57), conservative v rejection
      const V3 qv = M::cross(tv, e1);
      const float V = M::dot(d, qv);
      mk &= __builtin_amdgcn_ballot_w64(!(V < tlo)) & __builtin_amdgcn_ballot_w64(!((U + V) > thi));
      if (mk == 0ull) continue;
      // stage D: the reference's exact tests (:42-63), then the closed interval, then the list
      const float inv = 1.0f / det;                                // :47
      const float u = U * inv;                                     // :50
      const float v = V * inv;                                     // :57
      const float t = M::dot(e2, qv) * inv;                        // :63
      const bool miss = (det < RT_EPS) | (u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f);
      if (active & (!miss) & (tmin <= t) & (t <= tmax)) allhits_insert<CAP>(lt, lp, t, static_cast<int>(c0 + j));
    }
  }

  allhits_spheres<FMA, CAP>(p, o, d, tmin, tmax, active, lt, lp);

  if (tid < nb) allhits_store<FMA, CAP>(p, o, d, lt, lp, max_hits, hits + (base + tid) * max_hits, counts + base + tid);
}

// one record against one ray: the exact test, the closed interval, the list
template <bool FMA, int CAP>
__device__ __forceinline__ void allhits_test_record(const float4* __restrict__ rec, V3 o, V3 d, float tmin, float tmax,
                                                    float (&lt)[CAP], int (&lp)[CAP]) {
  const BvhRecord r = bvh_record(rec);
  float t = 0.0f, u = 0.0f, v = 0.0f;
  int stage;
  if (!hit_triangle_exact<FMA>(o, d, r.v0, r.e1, r.e2, RT_EPS, t, u, v, stage)) return;
  if (tmin <= t && t <= tmax) allhits_insert<CAP>(lt, lp, t, r.idx);
}

template <bool FMA, int CAP>
__global__ __launch_bounds__(64) void allhits_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n, const float4* __restrict__ segs,
                                                          uint32_t max_hits, float4* __restrict__ hits, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const float4 s0 = segs[2u * i], s1 = segs[2u * i + 1u];
  const V3 o = {s0.x, s0.y, s0.z}, d = {s0.w, s1.x, s1.y};
  const float tmin = s1.z, tmax = s1.w;
  const bool active = tmin <= tmax;                                // a NaN bound or tmin > tmax: nothing can be in the interval

  float lt[CAP];
  int lp[CAP];
  allhits_init<CAP>(lt, lp, max_hits);

  const float inf = __builtin_inff();
  const OccludedPrune q = occluded_prune(o, d);
  auto child = [&](const BvhNode& nd, int c) {
    float enter, exit;
    const bool nan = bvh_slab(nd, c, b.rho * (q.omax + nd.cmax[c]), o, q.inv, enter, exit);
    // (t_last is +inf while the list is not full: enter > +inf never holds)
    const bool skip = (exit < enter) || (exit < tmin) || (enter > tmax) || (enter > lt[CAP - 1]);
    return !(q.prunes && !nan) ? inf : skip ? -inf : fmaxf(-enter, -FLT_MAX);   // nearest first
  };
  auto leaf = [&](const float4* rec) { allhits_test_record<FMA, CAP>(rec, o, d, tmin, tmax, lt, lp); return false; };
  // -enter fell strictly behind -t_last meanwhile (an empty last slot has t = +inf: nothing is below -inf)
  auto stale = [&](float key) { return key < -lt[CAP - 1]; };
  const bool overflow = bvh_walk<64u, true>(b, s_mem, lane, active, child, leaf, stale);
  if (overflow) {                                                  // an entry was not kept: every leaf record, from an empty list
    allhits_init<CAP>(lt, lp, max_hits);
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) allhits_test_record<FMA, CAP>(b.records + 3u * j, o, d, tmin, tmax, lt, lp);
  }
  if (active) {
    for (uint32_t j = 0; j < b.n_always; ++j)
      allhits_test_record<FMA, CAP>(b.records + 3u * (b.n_leaf_records + j), o, d, tmin, tmax, lt, lp);
  }
  allhits_spheres<FMA, CAP>(p, o, d, tmin, tmax, active, lt, lp);
  allhits_store<FMA, CAP>(p, o, d, lt, lp, max_hits, hits + i * max_hits, counts + i);
}

// CAP = 4 for max_hits 1 .. 4, else 16, in both forms
hipError_t launch_allhits(const TraceParams& p, const BvhParams* b, bool fma, uint32_t n, const float* segs, uint32_t max_hits,
                          float4* hits, uint32_t* counts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (max_hits == 0u || max_hits > kAllHitsMax || segs == nullptr || hits == nullptr || counts == nullptr) return hipErrorInvalidValue;
  const float4* const s4 = reinterpret_cast<const float4*>(segs);
  const bool small = max_hits <= 4u;
  if (b != nullptr) {                                              // one wave per block, lane = ray, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    const auto walk = fma ? (small ? allhits_bvh_kernel<true, 4> : allhits_bvh_kernel<true, 16>)
                          : (small ? allhits_bvh_kernel<false, 4> : allhits_bvh_kernel<false, 16>);
    return launch_blocks(walk, n, 64u, 64u, lds, st, p, *b, n, s4, max_hits, hits, counts);
  }
  const auto scan = fma ? (small ? allhits_kernel<true, 4> : allhits_kernel<true, 16>)
                        : (small ? allhits_kernel<false, 4> : allhits_kernel<false, 16>);
  return launch_blocks(scan, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, s4, max_hits, hits, counts);
}

}  // namespace rtk
