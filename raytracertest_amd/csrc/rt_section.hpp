// rt_section.hpp -- the section queries (rt_tracer_section*, rt_tracer_section_segments*): the primitives of the
// tracer's scene that a slab d0 <= n.x <= d1 touches (a plane when d0 == d1, a half-space when one end is infinite), the max_hits
// lowest of them in ascending prim order behind an optional cursor and the total number of them; and, as a post-pass over such
// rows, the segment in which the plane n.x = d0 (or d1) cuts each of them.  Included by rt_kernels.hip only, behind
// rt_hexoverlap.hpp.  rt_overlap.hpp's list (OverlapList<CAP>), cursor (overlap_cursor, overlap_behind), scan kernel
// (region_kernel) and record test (region_test_record) are used as they are: this file states the rule, as the shape SlabRegion,
// the tree kernel with the slab's own child test, and the cut.
//
// Acceptance is a pure function of (plane, record, cursor), the text of include/rt_mi355x.h operation by operation: ONE
// arithmetic, every operation rounded separately (the library is compiled with -ffp-contract=off).  With
//   p(X) = (nx*X.x + ny*X.y) + nz*X.z                            (Math<false>::dot)
// on the record the renderer intersects, A = v0, B = fl(v0 + e1), C = fl(v0 + e2):
//   valid     nx, ny, nz finite and d0 <= d1 as a plain comparison (infinite ends are allowed; a NaN accepts nothing)
//   triangle  valid, none of p(A), p(B), p(C) a NaN, min3 <= d1 and max3 >= d0 (closed: touching counts)
//   sphere    its surface: pc = p(centre), rn = R * sqrt(dot(n, n)); valid, pc - rn <= d1 and pc + rn >= d0 (a slab is unbounded,
//             so the ball touches it exactly when the surface does)
// There is no second step: SlabRegion::separated is constant false.
//
// Why the tree prunes exactly, with no slack.  Rounding is monotone: x -> fl(n_axis * x) is monotone in the direction of n_axis's
// sign, and fl(a + b) is monotone in both operands (flushing denormals keeps both).  For a child box [lo, hi] take per axis
// xlo = n_axis >= 0 ? lo : hi and xhi the other end; then for every fp32 point P with lo <= P <= hi componentwise
//   pmin = p(xlo) <= p(P) <= p(xhi) = pmax                        whenever no value is a NaN,
// term by term and sum by sum.  A, B and C lie inside rtb::detail::tri_box and inside every ancestor's child box (rt_overlap.hpp),
// so a child with pmin > d1 or pmax < d0 holds only records the rule rejects.  A NaN never skips.  b.rho is not read:
// rt_dbg_query_accel_slack has no effect here.
//
// region_kernel<SlabRegion, CAP> (RT_QUERY_SCAN): rt_overlap.hpp's scan; the query is two 16-byte loads {nx, ny, nz, d0},
// {d1, -, -, -}, the pads enter no arithmetic.
// section_bvh_kernel<CAP> (RT_QUERY_BVH): region_bvh_kernel's text with the child test above in the place of the bounding-box
// comparison -- one wave per block, lane = plane, bvh_walk with 4-byte entries and a constant key, the overflow redo, the
// always-tested list, the spheres.  It is a kernel of its own and not a hook of region_bvh_kernel: a forwarding layer changes the
// generated code of the three shapes that kernel serves.
//
// section_segments_kernel: 256-thread blocks, lane = record j of plane j / per_plane, the shape of sides_kernel.  Only prims[j]
// is read.  With d the chosen offset and sX = p(X) - d (the sign of an fp32 difference is exact), a corner is above (s > 0),
// below (s < 0) or on the plane (s == 0):
//   RT_CUT_NONE      RT_PRIM_NONE or a prim outside the scene (nothing is read), an invalid plane, a NaN among the s, or all
//                    corners strictly on one side: the record is all zeros
//   RT_CUT_COPLANAR  all three corners on the plane; the points are zero
//   RT_CUT_TOUCH     no corner above, or none below, and one or two on: p0, p1 are the on-corners bit for bit, in the order of
//                    the walk A -> B -> C -> A (one on-corner: both points)
//   RT_CUT_SEGMENT   a corner above and one below: the endpoints are the on-corner, if any, and the crossings of the edges whose
//                    ends are strictly opposite, each computed from the below end L towards the above end U,
//                      t = sL / (sL - sU),  X = L + t * (U - L)  per component, the division IEEE
//                    so two records that share an edge with bit-equal corners give bit-equal points.  p0 is where the walk
//                    leaves the above side, p1 where it enters it: the segment runs along n x (e1 x e2).
//   features = f0 | f1 << 8: 0 / 1 / 2 the edge AB / BC / CA, 4 / 5 / 6 the corner A / B / C.
//   RT_CUT_CIRCLE    a sphere with |pc - d| <= rn: p0 = centre + ((d - pc) / nn) * n, p1 = {sqrt(max(R*R - (d - pc)^2 / nn, 0)), 0, 0},
//                    nn = dot(n, n); else RT_CUT_NONE.
#pragma once
#include "rt_hexoverlap.hpp"

namespace rtk {

constexpr int kCutNone = 0, kCutSegment = 1, kCutTouch = 2, kCutCoplanar = 3, kCutCircle = 4;

// the slab as the rule reads it (the pads are dropped here)
struct SlabQuery {
  V3 n;
  float d0, d1;
  bool valid;
};

__device__ __forceinline__ SlabQuery slab_query(float4 s0, float4 s1) {
  SlabQuery q;
  q.n = {s0.x, s0.y, s0.z};
  q.d0 = s0.w;
  q.d1 = s1.x;
  const bool finite = tri_finite(s0), ends = s0.w <= s1.x;               // (rt_trioverlap.hpp: x, y, z finite; false on a NaN)
  q.valid = finite & ends;
  return q;
}

// The slab as a region shape (rt_overlap.hpp's skeleton).  The scan reads no bounding box of the query, and the tree kernel below
// has its own child test, so Query carries no lo, hi.
struct SlabRegion {
  static constexpr int kFloat4s = 2;
  static constexpr int kScanWaves = 4, kTreeWaves = 0;
  using Query = SlabQuery;
  using SphereCtx = NoSphereCtx;
  static constexpr bool kSphereCtx = false;

  __device__ static __forceinline__ void load(Query& q, const float4* planes, size_t base, uint32_t lane, bool live) {
    float4 s0 = {0.0f, 0.0f, 0.0f, 1.0f}, s1 = {0.0f, 0.0f, 0.0f, 0.0f};   // padding lanes: d0 > d1 accepts nothing
    if (live) { s0 = planes[2u * (base + lane)]; s1 = planes[2u * (base + lane) + 1u]; }
    q = slab_query(s0, s1);
  }
  __device__ static __forceinline__ SphereCtx sphere_ctx(const float4*, size_t, uint32_t) { return {}; }

  // the whole triangle rule: fminf / fmaxf drop a NaN operand, hence the ordered tests
  __device__ static __forceinline__ bool step1(const Query& q, V3 A, V3 B, V3 C) {
    using M = Math<false>;
    const float pa = M::dot(q.n, A), pb = M::dot(q.n, B), pc = M::dot(q.n, C);
    const float mn = fminf(fminf(pa, pb), pc), mx = fmaxf(fmaxf(pa, pb), pc);
    const bool ordered = !(__builtin_isunordered(pa, pb) | __builtin_isunordered(pc, pc));
    return q.valid & ordered & (mn <= q.d1) & (mx >= q.d0);
  }
  __device__ static __forceinline__ bool separated(const Query&, V3, V3, V3, V3, V3) { return false; }

  __device__ static __forceinline__ bool sphere(const Query& q, SphereCtx, float4 sph) {
    using M = Math<false>;
    const float pc = M::dot(q.n, {sph.x, sph.y, sph.z});
    const float rn = sph.w * __builtin_sqrtf(M::dot(q.n, q.n));
    return q.valid & (pc - rn <= q.d1) & (pc + rn >= q.d0);
  }
};

template <int CAP>
__global__ __launch_bounds__(64) void section_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n, const float4* __restrict__ planes,
                                                          const int* __restrict__ after, uint32_t max_hits, int* __restrict__ prims,
                                                          uint32_t* __restrict__ counts) {
  extern __shared__ float4 s_mem[];
  using M = Math<false>;
  const uint32_t lane = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 64u, i = base + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  SlabQuery q;
  SlabRegion::load(q, planes, base, lane, true);
  const int cur = overlap_cursor(after, i, true);

  OverlapList<CAP> L;
  L.init_tree(max_hits);

  const float inf = __builtin_inff();
  const bool px = q.n.x >= 0.0f, py = q.n.y >= 0.0f, pz = q.n.z >= 0.0f;
  // the child's box between its two extreme corners along n: p() itself, no inflation; the key is constant (nothing is ordered)
  auto child = [&](const BvhNode& nd, int c) {
    const V3 xlo = {px ? nd.lo[0][c] : nd.hi[0][c], py ? nd.lo[1][c] : nd.hi[1][c], pz ? nd.lo[2][c] : nd.hi[2][c]};
    const V3 xhi = {px ? nd.hi[0][c] : nd.lo[0][c], py ? nd.hi[1][c] : nd.lo[1][c], pz ? nd.hi[2][c] : nd.lo[2][c]};
    const float pmin = M::dot(q.n, xlo), pmax = M::dot(q.n, xhi);
    return ((pmin > q.d1) | (pmax < q.d0)) ? -inf : 0.0f;          // (a NaN never skips)
  };
  auto leaf = [&](const float4* rec) { region_test_record<SlabRegion, CAP>(rec, q, cur, L); return false; };
  const bool overflow = bvh_walk<64u, false>(b, s_mem, lane, q.valid, child, leaf, [](float) { return false; });
  if (overflow) {                                                  // an entry was not kept: every leaf record, from an empty list and count
    L.init_tree(max_hits);
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) region_test_record<SlabRegion, CAP>(b.records + 3u * j, q, cur, L);
  }
  if (q.valid) {
    for (uint32_t j = 0; j < b.n_always; ++j) region_test_record<SlabRegion, CAP>(b.records + 3u * (b.n_leaf_records + j), q, cur, L);
    for (uint32_t si = 0; si < p.n_spheres; ++si) {
      const int prim = static_cast<int>(p.n_tris + si);
      if (SlabRegion::sphere(q, {}, p.spheres[si]) && overlap_behind(prim, cur)) L.insert(prim);
    }
  }
  L.store_tree(max_hits, prims + i * max_hits, counts + i);
}

// CAP = 0 for max_hits 0, 4 for 1 .. 4, else 16, in both forms (launch_region's choices, with the slab's own tree kernel)
hipError_t launch_section(const TraceParams& p, const BvhParams* b, uint32_t n, const float* planes, const int* after, uint32_t max_hits,
                          int* prims, uint32_t* counts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (max_hits > kAllHitsMax || planes == nullptr || counts == nullptr || (prims == nullptr && max_hits != 0u)) return hipErrorInvalidValue;
  const float4* const q4 = reinterpret_cast<const float4*>(planes);
  if (b != nullptr) {
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, false);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    const auto walk = max_hits == 0u ? section_bvh_kernel<0> : max_hits <= 4u ? section_bvh_kernel<4> : section_bvh_kernel<16>;
    return launch_blocks(walk, n, 64u, 64u, lds, st, p, *b, n, q4, after, max_hits, prims, counts);
  }
  const auto scan = max_hits == 0u ? region_kernel<SlabRegion, 0> : max_hits <= 4u ? region_kernel<SlabRegion, 4> : region_kernel<SlabRegion, 16>;
  return launch_blocks(scan, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, q4, after, max_hits, prims, counts);
}

// the crossing of the edge from the below end L (sL < 0) to the above end U (sU > 0)
__device__ __forceinline__ V3 section_crossing(V3 L, V3 U, float sL, float sU) {
  const float t = sL / (sL - sU);
  return {L.x + t * (U.x - L.x), L.y + t * (U.y - L.y), L.z + t * (U.z - L.z)};
}

__global__ __launch_bounds__(256) void section_segments_kernel(const TraceParams p, uint64_t n_records, uint32_t per_plane, uint32_t side,
                                                                const float4* __restrict__ planes, const int* __restrict__ prims,
                                                                float4* __restrict__ cuts) {
  using M = Math<false>;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (j >= n_records) return;
  const int prim = prims[j];
  const uint32_t up = static_cast<uint32_t>(prim);                       // (a negative prim is beyond every scene)
  V3 p0 = {0.0f, 0.0f, 0.0f}, p1 = {0.0f, 0.0f, 0.0f};
  int kind = kCutNone, f0 = 0, f1 = 0;
  if (up < p.n_tris) {
    const uint64_t i = per_plane == 1u ? j : j / per_plane;
    const SlabQuery q = slab_query(planes[2u * i], planes[2u * i + 1u]);
    const float d = side != 0u ? q.d1 : q.d0;
    const float4 A0 = p.tri_a[2u * static_cast<size_t>(up)], A1 = p.tri_a[2u * static_cast<size_t>(up) + 1u];
    const V3 e2 = {A0.x, A0.y, A0.z}, e1 = {A0.w, A1.x, A1.y}, A = {A1.z, A1.w, p.tri_b[up]};
    const V3 P[3] = {A, rtd::add(A, e1), rtd::add(A, e2)};
    const float s[3] = {M::dot(q.n, P[0]) - d, M::dot(q.n, P[1]) - d, M::dot(q.n, P[2]) - d};
    const bool nan = __builtin_isunordered(s[0], s[1]) | __builtin_isunordered(s[2], s[2]);
    const int above = (s[0] > 0.0f) + (s[1] > 0.0f) + (s[2] > 0.0f), below = (s[0] < 0.0f) + (s[1] < 0.0f) + (s[2] < 0.0f);
    const int on = 3 - above - below;
    if (q.valid && !nan && above != 3 && below != 3) {
      if (on == 3) {
        kind = kCutCoplanar;
      } else if (above == 0 || below == 0) {                             // one or two corners on the plane, the rest on one side
        kind = kCutTouch;
        // the corner the walk meets first: with two on-corners the one whose successor is on as well
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
          if (s[k] == 0.0f && s[k2] != 0.0f) {                           // (the corner before k is off the plane: k is the first)
            const bool two = s[k1] == 0.0f;
            p0 = P[k]; f0 = 4 + k;
            p1 = two ? P[k1] : P[k]; f1 = two ? 4 + k1 : 4 + k;
          }
        }
      } else {
        kind = kCutSegment;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
          if (s[k] > 0.0f && s[k1] < 0.0f) { p0 = section_crossing(P[k1], P[k], s[k1], s[k]); f0 = k; }      // the edge leaves the above side
          if (s[k] < 0.0f && s[k1] > 0.0f) { p1 = section_crossing(P[k], P[k1], s[k], s[k1]); f1 = k; }      // ... enters it
          if (s[k] == 0.0f && s[k2] > 0.0f) { p0 = P[k]; f0 = 4 + k; }                                       // (then the next corner is below)
          if (s[k] == 0.0f && s[k2] < 0.0f) { p1 = P[k]; f1 = 4 + k; }
        }
      }
    }
  } else if (prim >= 0 && up - p.n_tris < p.n_spheres) {
    const uint64_t i = per_plane == 1u ? j : j / per_plane;
    const SlabQuery q = slab_query(planes[2u * i], planes[2u * i + 1u]);
    const float d = side != 0u ? q.d1 : q.d0;
    const float4 sph = p.spheres[up - p.n_tris];
    const float pc = M::dot(q.n, {sph.x, sph.y, sph.z}), nn = M::dot(q.n, q.n);
    const float rn = sph.w * __builtin_sqrtf(nn), e = d - pc;
    if (q.valid && fabsf(pc - d) <= rn) {
      const float k = e / nn;
      kind = kCutCircle;
      p0 = {sph.x + k * q.n.x, sph.y + k * q.n.y, sph.z + k * q.n.z};
      p1 = {__builtin_sqrtf(fmaxf(sph.w * sph.w - (e * e) / nn, 0.0f)), 0.0f, 0.0f};
    }
  }
  cuts[2u * j] = make_float4(p0.x, p0.y, p0.z, __int_as_float(kind));
  cuts[2u * j + 1u] = make_float4(p1.x, p1.y, p1.z, __int_as_float(f0 | (f1 << 8)));
}

// planes n x 8 floats; prims and cuts n * per_plane records; planes and cuts 16-byte aligned
hipError_t launch_section_segments(const TraceParams& p, uint32_t n, uint32_t per_plane, uint32_t side, const float* planes, const int* prims,
                                   void* cuts, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (per_plane == 0u || per_plane > kAllHitsMax || side > 1u || planes == nullptr || prims == nullptr || cuts == nullptr) return hipErrorInvalidValue;
  const uint64_t total = static_cast<uint64_t>(n) * per_plane;
  const dim3 grid(static_cast<uint32_t>((total + 255u) / 256u));         // (at most 2^28 blocks)
  hipLaunchKernelGGL(section_segments_kernel, grid, dim3(256), 0, st, p, total, per_plane, side, reinterpret_cast<const float4*>(planes), prims,
                     static_cast<float4*>(cuts));
  return hipGetLastError();
}

}  // namespace rtk
