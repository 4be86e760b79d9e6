// rt_overlap.hpp -- the region query (rt_tracer_overlap*): the primitives of the tracer's scene that touch box i,
// the max_hits lowest of them in ascending prim order behind an optional cursor, and the total number of them.  Included by
// rt_kernels.hip only, behind rt_nearest.hpp.  Nothing is shared with the other queries beyond V3, Math<false> (the separately
// rounded cross and (x*x' + y*y') + z*z'), the staging of the scan kernels, the tree and bvh_walk.
//
// Acceptance is a pure function of (box, record, cursor), the text of include/rt_mi355x.h operation by operation; there is no
// reference arithmetic to be faithful to, so there is ONE arithmetic, every operation rounded separately (the library is
// compiled with -ffp-contract=off).  On the record the renderer intersects, A = v0, B = fl(v0 + e1), C = fl(v0 + e2):
//   step 1 (BoxRegion::step1)  per axis  lo <= hi,  neither B nor C a NaN,  min(A, B, C) <= hi,  max(A, B, C) >= lo
//   step 2 (separated)          c = 0.5*lo + 0.5*hi, h = 0.5*hi - 0.5*lo, n = e1 x e2:  separated when |n.(A - c)| > h.|n|
//   step 3 (overlap_axes)       the nine axes unit_k x f of f = e1, C' - B', A' - C' (corners moved by -c), each on two corners
// A step rejects when its "separated" is TRUE, so a NaN in steps 2-3 (overflow near FLT_MAX) never rejects; every comparison
// of step 1 is false on a NaN, so a NaN there always rejects.  A sphere is its surface (BoxRegion::sphere).
//
// Why the tree prunes exactly, with no slack: a leaf record's tree box is rtb::detail::tri_box -- the corners in double,
// rounded outward -- so step 1's [min, max] lies inside it and inside every ancestor's child box.  A child is entered when its
// box and the query box overlap under the same closed comparisons; a child the walk skips holds only records step 1 rejects.
// b.rho is not read: rt_dbg_query_accel_slack has no effect here.
//
// The kernels are written once for the three region shapes (the box here, the triangle of rt_trioverlap.hpp, the hexahedron of
// rt_hexoverlap.hpp); a shape is a policy type of static members (BoxRegion below) that states its rule and nothing else.
//
// region_kernel<Shape, CAP> (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = query, the query is
// Shape::kFloat4s 16-byte loads, spheres after the triangles.  Prims arrive in ascending order: the first max_hits accepted
// are stored (compile-time slots, selected by the count), the count runs on.  A record no lane's step 1 passes is left by
// ballot before steps 2-3.  A padding lane holds a query that accepts nothing and stores nothing.
// The kernel keeps the scan in its own text -- the chunk loop, the LDS layout, the staging and the barriers are A SECOND COPY
// of rt_scan.hpp's scan_triangles, which is the first: change them together.  On the shared function one of its 30 arms (the
// hexahedron at max_hits 16, 1 100 triangles) measured slower than the parent by more than the parent's own spread, and a
// template has one text.
//
// region_bvh_kernel<Shape, CAP> (RT_QUERY_BVH): one wave per block, lane = query, bvh_walk with 4-byte entries and a constant key
// for a child whose box overlaps the query's bounding box.  Records arrive in tree order: the list is rt_allhits.hpp's idiom on
// prims alone -- CAP ints behind compile-time indices, the leading CAP - max_hits slots pinned at -1, a new prim replaces the last
// slot when it is lower and is bubbled up.  A walk visits every record at most once, so the count is exact.  After the walk: the
// overflow redo (which RESTARTS list and count from every leaf record), the always-tested list, the spheres.
//
// CAP = 0 is max_hits = 0: no list, no row, the count alone.
#pragma once
#include "rt_nearest.hpp"

namespace rtk {

constexpr int kOverlapEmpty = 0x7FFFFFFF;      // prim of an empty slot of the tree kernel's list: above every prim

// the query box as the rule reads it: lo, hi, centre, half-extent, lo <= hi on all three axes (the pads are dropped here)
struct OverlapBox {
  V3 lo, hi, c, h;
  bool valid;
};

__device__ __forceinline__ OverlapBox overlap_box(float4 b0, float4 b1) {
  OverlapBox q;
  q.lo = {b0.x, b0.y, b0.z};
  q.hi = {b1.x, b1.y, b1.z};
  q.c = {0.5f * b0.x + 0.5f * b1.x, 0.5f * b0.y + 0.5f * b1.y, 0.5f * b0.z + 0.5f * b1.z};
  q.h = {0.5f * b1.x - 0.5f * b0.x, 0.5f * b1.y - 0.5f * b0.y, 0.5f * b1.z - 0.5f * b0.z};
  q.valid = (b0.x <= b1.x) & (b0.y <= b1.y) & (b0.z <= b1.z);
  return q;
}

// step 1 on one axis: closed, plain comparisons; fminf / fmaxf drop a NaN operand, hence the ordered test of B and C (a NaN A
// makes both NaN)
__device__ __forceinline__ bool overlap_axis1(float a, float b, float c, float lo, float hi) {
  const float mn = fminf(fminf(a, b), c), mx = fmaxf(fmaxf(a, b), c);
  return (!__builtin_isunordered(b, c)) & (mn <= hi) & (mx >= lo);
}

// step 3 for one edge vector f on the two corners P, Q (moved by -c) whose projections differ: the axes unit_x x f, unit_y x f,
// unit_z x f.  Four plain comparisons per axis: a NaN never separates.
__device__ __forceinline__ bool overlap_axes(V3 f, V3 P, V3 Q, V3 h) {
  const float ax = fabsf(f.x), ay = fabsf(f.y), az = fabsf(f.z);
  const float px0 = f.y * P.z - f.z * P.y, px1 = f.y * Q.z - f.z * Q.y, rx = h.y * az + h.z * ay;
  const float py0 = f.z * P.x - f.x * P.z, py1 = f.z * Q.x - f.x * Q.z, ry = h.x * az + h.z * ax;
  const float pz0 = f.x * P.y - f.y * P.x, pz1 = f.x * Q.y - f.y * Q.x, rz = h.x * ay + h.y * ax;
  return ((px0 > rx) & (px1 > rx)) | ((px0 < -rx) & (px1 < -rx)) | ((py0 > ry) & (py1 > ry)) | ((py0 < -ry) & (py1 < -ry)) |
         ((pz0 > rz) & (pz1 > rz)) | ((pz0 < -rz) & (pz1 < -rz));
}

// The box as a region shape: what region_kernel and region_bvh_kernel (below) ask of a shape, static members only.
struct NoSphereCtx {};
struct BoxRegion {
  static constexpr int kFloat4s = 2;                               // 16-byte loads per query
  static constexpr int kScanWaves = 4, kTreeWaves = 0;             // waves per SIMD of the two kernels (0: no bound)
  using Query = OverlapBox;
  using SphereCtx = NoSphereCtx;                                   // what the sphere rule alone needs of the query as given
  static constexpr bool kSphereCtx = false;

  // query base + lane; a lane that is not live is a padding lane
  __device__ static __forceinline__ void load(Query& q, const float4* boxes, size_t base, uint32_t lane, bool live) {
    float4 b0 = {1.0f, 1.0f, 1.0f, 0.0f}, b1 = {0.0f, 0.0f, 0.0f, 0.0f};   // padding lanes: lo > hi accepts nothing
    if (live) { b0 = boxes[2u * (base + lane)]; b1 = boxes[2u * (base + lane) + 1u]; }
    q = overlap_box(b0, b1);
  }
  __device__ static __forceinline__ SphereCtx sphere_ctx(const float4*, size_t, uint32_t) { return {}; }

  __device__ static __forceinline__ bool step1(const Query& q, V3 A, V3 B, V3 C) {
    const bool x = overlap_axis1(A.x, B.x, C.x, q.lo.x, q.hi.x), y = overlap_axis1(A.y, B.y, C.y, q.lo.y, q.hi.y);
    const bool z = overlap_axis1(A.z, B.z, C.z, q.lo.z, q.hi.z);
    return q.valid & x & y & z;
  }

  // steps 2 and 3: true when the plane or one of the nine axes separates the triangle from the box
  __device__ static __forceinline__ bool separated(const Query& q, V3 A, V3 B, V3 C, V3 e1, V3 e2) {
    using M = Math<false>;
    const V3 n = M::cross(e1, e2);
    const V3 a = rtd::sub(A, q.c), b = rtd::sub(B, q.c), c = rtd::sub(C, q.c);
    const float s = M::dot(n, a);
    const float r = M::dot(q.h, {fabsf(n.x), fabsf(n.y), fabsf(n.z)});
    const bool s0 = overlap_axes(e1, a, c, q.h), s1 = overlap_axes(rtd::sub(c, b), a, b, q.h), s2 = overlap_axes(rtd::sub(a, c), a, b, q.h);
    return (fabsf(s) > r) | s0 | s1 | s2;
  }

  // the sphere rule: the surface touches the box when the box's nearest point is inside the ball and its farthest corner is not
  __device__ static __forceinline__ bool sphere(const Query& q, SphereCtx, float4 sph) {
    const float ax = q.lo.x - sph.x, bx = sph.x - q.hi.x;
    const float ay = q.lo.y - sph.y, by = sph.y - q.hi.y;
    const float az = q.lo.z - sph.z, bz = sph.z - q.hi.z;
    const float gx = fmaxf(fmaxf(ax, bx), 0.0f), gy = fmaxf(fmaxf(ay, by), 0.0f), gz = fmaxf(fmaxf(az, bz), 0.0f);
    const float fx = fmaxf(fabsf(ax), fabsf(bx)), fy = fmaxf(fabsf(ay), fabsf(by)), fz = fmaxf(fabsf(az), fabsf(bz));
    const float d2min = (gx * gx + gy * gy) + gz * gz;
    const float d2max = (fx * fx + fy * fy) + fz * fz;
    const float rr = sph.w * sph.w;
    return q.valid & (d2min <= rr) & (rr <= d2max);
  }
};

// the continuation cursor of one box: RT_PRIM_NONE accepts every prim
__device__ __forceinline__ int overlap_cursor(const int* __restrict__ after, size_t i, bool valid) {
  return (after != nullptr && valid) ? after[i] : -1;
}
__device__ __forceinline__ bool overlap_behind(int prim, int after) { return (after == -1) | (prim > after); }

// The lowest prims of one box and their total.  Slots are touched with compile-time indices only (a runtime-indexed private
// array would live in scratch).
template <int CAP>
struct OverlapList {
  int lp[CAP > 0 ? CAP : 1];
  uint32_t cnt;

  // scan: slots 0 .. max_hits-1 filled in arrival order; tree: the wanted list is the last max_hits slots
  __device__ __forceinline__ void init_scan() {
    cnt = 0u;
#pragma unroll
    for (int s = 0; s < CAP; ++s) lp[s] = -1;
  }
  __device__ __forceinline__ void init_tree(uint32_t max_hits) {
    cnt = 0u;
#pragma unroll
    for (int s = 0; s < CAP; ++s) lp[s] = static_cast<uint32_t>(s) + max_hits >= static_cast<uint32_t>(CAP) ? kOverlapEmpty : -1;
  }
  // an accepted prim above every earlier one
  __device__ __forceinline__ void append(int prim, uint32_t max_hits) {
    if constexpr (CAP > 0) {
      if (cnt < max_hits) {
#pragma unroll
        for (int s = 0; s < CAP; ++s) lp[s] = (cnt == static_cast<uint32_t>(s)) ? prim : lp[s];
      }
    }
    ++cnt;
  }
  // an accepted prim in any order (each at most once)
  __device__ __forceinline__ void insert(int prim) {
    if constexpr (CAP > 0) {
      if (prim < lp[CAP - 1]) {
        lp[CAP - 1] = prim;
#pragma unroll
        for (int s = CAP - 1; s > 0; --s) {
          const int a = lp[s - 1], b = lp[s];
          lp[s - 1] = b < a ? b : a;
          lp[s] = b < a ? a : b;
        }
      }
    }
    ++cnt;
  }
  __device__ __forceinline__ void store_scan(uint32_t max_hits, int* __restrict__ row, uint32_t* __restrict__ count) const {
#pragma unroll
    for (int s = 0; s < CAP; ++s)
      if (static_cast<uint32_t>(s) < max_hits) row[s] = lp[s];
    *count = cnt;
  }
  __device__ __forceinline__ void store_tree(uint32_t max_hits, int* __restrict__ row, uint32_t* __restrict__ count) const {
#pragma unroll
    for (int s = 0; s < CAP; ++s)
      if (static_cast<uint32_t>(s) + max_hits >= static_cast<uint32_t>(CAP))
        row[static_cast<uint32_t>(s) + max_hits - static_cast<uint32_t>(CAP)] = lp[s] == kOverlapEmpty ? -1 : lp[s];
    *count = cnt;
  }
};

// ---- what every region shape shares: one scan kernel, one tree kernel, one launch ----
// A shape (BoxRegion above, TriRegion in rt_trioverlap.hpp, HexRegion in rt_hexoverlap.hpp) states:
//   kFloat4s                            16-byte loads per query (2 / 3 / 8)
//   Query, load(q, queries, base, lane, live)
//                                       query base + lane as the rule reads it, with lo, hi (its bounding box) and valid; a lane
//                                       that is not live is a padding lane, whose query accepts nothing
//   step1(q, A, B, C), separated(q, A, B, C, e1, e2)
//   SphereCtx, kSphereCtx, sphere_ctx(queries, base, lane), sphere(q, K, sph)
//                                       the sphere rule, and what it alone needs of the query as given: nothing (kSphereCtx false,
//                                       an empty K passed by value) but for the hexahedron, which loads its corners again once
//                                       there are spheres and the query is valid, so that the triangle loop does not carry them
//   kScanWaves, kTreeWaves              the waves-per-SIMD bound of the two kernels (0: none)
// The rule's functions ARE the policy's members: a forwarding layer in between changes the generated code.
template <class Shape, int CAP>
__global__ __launch_bounds__(256, Shape::kScanWaves) void region_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ queries,
                                                                         const int* __restrict__ after, uint32_t max_hits,
                                                                         int* __restrict__ prims, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first query of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  typename Shape::Query q;
  Shape::load(q, queries, base, tid, tid < nb);
  const int cur = overlap_cursor(after, base + tid, tid < nb);

  OverlapList<CAP> L;
  L.init_scan();

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
    if (__builtin_amdgcn_ballot_w64(q.valid) == 0ull) continue;    // no query of this wave accepts; it still helps staging
    for (uint32_t j = 0; j < cn; ++j) {
      const float4 A0 = sA[2u * j], A1 = sA[2u * j + 1u];
      const V3 e2 = {A0.x, A0.y, A0.z}, e1 = {A0.w, A1.x, A1.y}, A = {A1.z, A1.w, sB[j]};
      const V3 B = rtd::add(A, e1), C = rtd::add(A, e2);
      const int prim = static_cast<int>(c0 + j);
      const bool behind = overlap_behind(prim, cur);
      const bool in1 = Shape::step1(q, A, B, C) & behind;
      if (__builtin_amdgcn_ballot_w64(in1) == 0ull) continue;      // step 1 rejects it for every query of the wave
      if (in1 && !Shape::separated(q, A, B, C, e1, e2)) L.append(prim, max_hits);
    }
  }
  if (!Shape::kSphereCtx || (p.n_spheres != 0u && q.valid)) {      // (a valid query is no padding lane; no barrier below)
    const typename Shape::SphereCtx K = Shape::sphere_ctx(queries, base, tid);
    for (uint32_t si = 0; si < p.n_spheres; ++si) {
      const int prim = static_cast<int>(nt + si);
      if (Shape::sphere(q, K, p.spheres[si]) && overlap_behind(prim, cur)) L.append(prim, max_hits);
    }
  }

  if (tid < nb) L.store_scan(max_hits, prims + (base + tid) * max_hits, counts + base + tid);
}

// one 48-byte record against one query
template <class Shape, int CAP>
__device__ __forceinline__ void region_test_record(const float4* __restrict__ rec, const typename Shape::Query& q, int cur,
                                                   OverlapList<CAP>& L) {
  const BvhRecord r = bvh_record(rec);
  const V3 B = rtd::add(r.v0, r.e1), C = rtd::add(r.v0, r.e2);
  if (Shape::step1(q, r.v0, B, C) && overlap_behind(r.idx, cur) && !Shape::separated(q, r.v0, B, C, r.e1, r.e2)) L.insert(r.idx);
}

template <class Shape, int CAP>
__global__ __launch_bounds__(64, Shape::kTreeWaves) void region_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n,
                                                                            const float4* __restrict__ queries,
                                                                            const int* __restrict__ after, uint32_t max_hits,
                                                                            int* __restrict__ prims, uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 64u, i = base + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  typename Shape::Query q;
  Shape::load(q, queries, base, lane, true);
  const int cur = overlap_cursor(after, i, true);

  OverlapList<CAP> L;
  L.init_tree(max_hits);

  const float inf = __builtin_inff();
  // the child's box against the query's bounding box: step 1's comparisons, no inflation; the key is constant (nothing is ordered)
  auto child = [&](const BvhNode& nd, int c) {
    const bool in = (nd.lo[0][c] <= q.hi.x) & (nd.hi[0][c] >= q.lo.x) & (nd.lo[1][c] <= q.hi.y) & (nd.hi[1][c] >= q.lo.y) &
                    (nd.lo[2][c] <= q.hi.z) & (nd.hi[2][c] >= q.lo.z);
    return in ? 0.0f : -inf;
  };
  auto leaf = [&](const float4* rec) { region_test_record<Shape, CAP>(rec, q, cur, L); return false; };
  const bool overflow = bvh_walk<64u, false>(b, s_mem, lane, q.valid, child, leaf, [](float) { return false; });
  if (overflow) {                                                  // an entry was not kept: every leaf record, from an empty list and count
    L.init_tree(max_hits);
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) region_test_record<Shape, CAP>(b.records + 3u * j, q, cur, L);
  }
  if (q.valid) {
    for (uint32_t j = 0; j < b.n_always; ++j) region_test_record<Shape, CAP>(b.records + 3u * (b.n_leaf_records + j), q, cur, L);
    if (!Shape::kSphereCtx || p.n_spheres != 0u) {
      const typename Shape::SphereCtx K = Shape::sphere_ctx(queries, base, lane);
      for (uint32_t si = 0; si < p.n_spheres; ++si) {
        const int prim = static_cast<int>(p.n_tris + si);
        if (Shape::sphere(q, K, p.spheres[si]) && overlap_behind(prim, cur)) L.insert(prim);
      }
    }
  }
  L.store_tree(max_hits, prims + i * max_hits, counts + i);
}

// CAP = 0 for max_hits 0, 4 for 1 .. 4, else 16, in both forms
template <class Shape>
hipError_t launch_region(const TraceParams& p, const BvhParams* b, uint32_t n, const float* queries, const int* after, uint32_t max_hits,
                         int* prims, uint32_t* counts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (max_hits > kAllHitsMax || queries == nullptr || counts == nullptr || (prims == nullptr && max_hits != 0u)) return hipErrorInvalidValue;
  const float4* const q4 = reinterpret_cast<const float4*>(queries);
  if (b != nullptr) {                                              // one wave per block, lane = query, the reference alone on the stack
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, false);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    const auto walk = max_hits == 0u ? region_bvh_kernel<Shape, 0> : max_hits <= 4u ? region_bvh_kernel<Shape, 4> : region_bvh_kernel<Shape, 16>;
    return launch_blocks(walk, n, 64u, 64u, lds, st, p, *b, n, q4, after, max_hits, prims, counts);
  }
  const auto scan = max_hits == 0u ? region_kernel<Shape, 0> : max_hits <= 4u ? region_kernel<Shape, 4> : region_kernel<Shape, 16>;
  return launch_blocks(scan, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, q4, after, max_hits, prims, counts);
}

hipError_t launch_overlap(const TraceParams& p, const BvhParams* b, uint32_t n, const float* boxes, const int* after, uint32_t max_hits,
                          int* prims, uint32_t* counts, hipStream_t st) {
  return launch_region<BoxRegion>(p, b, n, boxes, after, max_hits, prims, counts, st);
}

}  // namespace rtk
