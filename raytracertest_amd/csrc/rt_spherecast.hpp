// rt_spherecast.hpp -- the swept query (rt_tracer_sphere_cast*): a sphere of radius r whose centre moves along
// c(t) = o + t*d, 0 <= t <= tmax; when and where does it first touch the tracer's scene?  Included by rt_kernels.hip only, behind
// rt_overlap.hpp.  Shared with the other queries: V3, Math<false> (the separately rounded cross and (x*x' + y*y') + z*z'),
// closest_triangle (rt_closest.hpp), the staging of the scan kernels, the tree, bvh_slab and bvh_walk.
//
// One arithmetic for both math modes, the text of include/rt_mi355x.h operation by operation (the library is compiled with
// -ffp-contract=off; division and sqrt are correctly rounded).  Per triangle record (v0, e1, e2), with w = o - v0:
//   start    closest_triangle(o).t <= r*r: the candidate is t = 0 with that evaluation's (u, v)
//   else     the smallest of seven entry roots (+inf: none) -- the face moved by r towards the origin's side (sweep_face), the
//            cylinders about the edges AB, AC, BC (sweep_edge), the balls about A, B, C (sweep_entry) -- certified: c = o + t*d,
//            closest_triangle(c).t <= (r + s)^2 with s = kSweepSlack * (max|c| + r); (u, v) are that evaluation's.  A smallest
//            root that fails yields no contact for the triangle.
// A sphere of the scene is its surface (sweep_sphere): start overlap by ClosestPoint's |sqrt(w.w) - R|, the entry root against
// R + r from outside, the exit root against R - r from inside, certified by the same expression.  Accepted when t <= tmax; the
// winner is the smallest (t, prim), equal t (==) to the lowest prim -- no visiting order is named, so the scan and the walk
// cannot disagree once the walk visits every record that holds an accepted contact.
//
// Why the walk may prune: an accepted contact is CERTIFIED -- the fp32 point c lies within (r + s) of the record by
// closest_triangle's own arithmetic, hence (its error bound added) inside the record's box grown by r + s + pad, whatever the
// conditioning of the root that produced t.  spherecast_bvh_kernel's child() runs bvh_slab on the child's box grown by
//   g = (r + kSweepTiny) + s_box + pad,   s_box = 4 * kSweepSlack * (cmax + r),   pad = rho_s * (max|o| + cmax + r)
// (s_box bounds s for every centre inside the grown box; DESIGN.md 4.3k derives rho_s) and skips the child only when the line
// misses the grown box, leaves it before t = 0, or enters it STRICTLY after min(best, tmax): a tie may hide a lower prim.
// Nearest entry first; a popped entry that has fallen strictly behind best is dropped.  A sweep with a non-finite component or
// a zero direction, or a child with a NaN in its slab test, takes no pruning decision.
//
// The ends of fp32's range (sweep_range_guard, once per lane; restated by tests/spherecast_expect.py).  The argument above takes
// "t0 <= r*r" and "d2 <= (r + s)^2" to mean what they say.  Two things break that, and the walk allows for both:
//   underflow  A square below 2^-149 rounds to a multiple of 2^-149: each of the three products of closest_triangle's t and the
//              threshold itself is off by at most 2^-150, so an accepted record may lie 2^-74 farther away than the threshold
//              says (sqrt(x + 4 * 2^-150) <= sqrt(x) + 2^-74), which matters once r + s is that small -- a scene of size 2^-64
//              or less.  The box is therefore grown by kSweepTiny = 2^-72 more, four times that: the leading r of g is
//              r + kSweepTiny, formed once per lane.  From r >= 2^-47 the sum is r bit for bit.
//   overflow   Where r*r or (r + s)^2 is +inf, "inf <= inf" accepts a record at any distance.  (r + s)^2 is finite for every
//              centre the boxes can hold while m = (max|o| + cmax_root) + r < kSweepHuge = 2^62 (cmax_root: the largest
//              |coordinate| of the root's four child boxes, so |c| <= cmax_root + g <= 2m, r + s < 2m and its square below
//              2^126); a sweep with m >= 2^62, or a NaN m, takes no pruning decision.
//
// spherecast_kernel (RT_QUERY_SCAN): the scan of rt_scan.hpp (idle waves skip), lane = sweep, two 16-byte loads per sweep,
// spheres after the triangles.
// spherecast_bvh_kernel (RT_QUERY_BVH): one wave per block, lane = sweep, bvh_walk with keyed entries {-enter, reference}.
#pragma once
#include "rt_overlap.hpp"

namespace rtk {

// what a lane keeps of its sweep: origin, direction, radius, r*r, d.d, and the best contact so far (best starts at tmax with
// best_i = -1, as closest_keep expects: t == tmax is accepted)
struct Sweep {
  V3 o, d;
  float r, rr, dd;
  float best, bu, bv;
  int best_i;
};

__device__ __forceinline__ Sweep sweep_load(float4 s0, float4 s1) {
  Sweep q;
  q.o = {s0.x, s0.y, s0.z};
  q.d = {s0.w, s1.x, s1.y};
  q.r = s1.z;
  q.rr = s1.z * s1.z;
  q.dd = Math<false>::dot(q.d, q.d);
  q.best = s1.w; q.bu = 0.0f; q.bv = 0.0f;
  q.best_i = -1;
  return q;
}

// radius >= 0 and finite, tmax >= 0; a NaN fails every comparison
__device__ __forceinline__ bool sweep_valid(float r, float tmax) { return (r >= 0.0f) & (r < __builtin_inff()) & (tmax >= 0.0f); }

__device__ __forceinline__ V3 sweep_axpy(V3 m, float k, V3 v) { return {m.x + k * v.x, m.y + k * v.y, m.z + k * v.z}; }
__device__ __forceinline__ V3 sweep_axmy(V3 m, float k, V3 v) { return {m.x - k * v.x, m.y - k * v.y, m.z - k * v.z}; }

// the entry root of the line m + t*dv (a = dv.dv) into the ball of squared radius rr about the origin, in the form that
// cancels nothing: b' = -m.dv > 0, l = m + (b'/a)*dv, disc = rr - l.l >= 0, t = (m.m - rr) / (b' + sqrt(a*disc)) > 0; +inf: none
__device__ __forceinline__ float sweep_entry(V3 m, V3 dv, float a, float rr) {
  using M = Math<false>;
  const float bp = -M::dot(m, dv);
  const V3 l = sweep_axpy(m, bp / a, dv);
  const float disc = rr - M::dot(l, l);
  const float t = (M::dot(m, m) - rr) / (bp + __builtin_sqrtf(a * disc));
  return ((bp > 0.0f) & (disc >= 0.0f) & (t > 0.0f)) ? t : __builtin_inff();
}

// the cylinder of squared radius rr about the edge from m's origin along e: the axial components of m and d are removed, the
// entry root is sweep_entry's, accepted when its axial parameter s0 + t*sd lies in [0, 1]
__device__ __forceinline__ float sweep_edge(V3 m, V3 e, V3 d, float rr) {
  using M = Math<false>;
  const float ee = M::dot(e, e);
  const float s0 = M::dot(m, e) / ee, sd = M::dot(d, e) / ee;
  const V3 mp = sweep_axmy(m, s0, e), dp = sweep_axmy(d, sd, e);
  const float t = sweep_entry(mp, dp, M::dot(dp, dp), rr);
  const float s = s0 + t * sd;
  return ((s >= 0.0f) & (s <= 1.0f)) ? t : __builtin_inff();
}

// the face moved by r along the unit normal towards the origin's side: h = n.w, the plane is reached at
// t = (|h| - r*|n|) / (-+ n.d) (numerator and denominator > 0: from outside the slab, approaching), and the point w + t*d has
// the barycentrics u = n.((w + t*d) x e2) / n.n, v = n.(e1 x (w + t*d)) / n.n, closed bounds
__device__ __forceinline__ float sweep_face(V3 w, V3 e1, V3 e2, V3 d, float r) {
  using M = Math<false>;
  const V3 n = M::cross(e1, e2);
  const float nn = M::dot(n, n);
  const float h = M::dot(n, w), dn = M::dot(n, d);
  const float num = fabsf(h) - r * __builtin_sqrtf(nn);
  const float den = h >= 0.0f ? -dn : dn;
  const float t = num / den;
  const V3 q = sweep_axpy(w, t, d);
  const float u = M::dot(M::cross(q, e2), n) / nn, v = M::dot(M::cross(e1, q), n) / nn;
  return ((num > 0.0f) & (den > 0.0f) & (t > 0.0f) & (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f)) ? t : __builtin_inff();
}

// one accepted contact under the order-free winner rule
__device__ __forceinline__ void sweep_keep(Sweep& q, float t, float u, float v, int prim) {
  if ((t < q.best) | ((t == q.best) & ((q.best_i < 0) | (prim < q.best_i)))) { q.best = t; q.bu = u; q.bv = v; q.best_i = prim; }
}
// the two constants of the range guard (the header comment derives them)
constexpr float kSweepTiny = 0x1p-72f, kSweepHuge = 0x1p62f;

// may this sweep prune at all, as far as fp32's range goes?  m = (max|o| + cmax_root) + r below kSweepHuge
__device__ __forceinline__ bool sweep_range_guard(const BvhParams& b, float omax, float r) {
  if (b.n_nodes == 0u) return true;
  const float4 cm = b.nodes[7];                                    // the root's cmax[4] (an empty child's is 0)
  const float croot = fmaxf(fmaxf(cm.x, cm.y), fmaxf(cm.z, cm.w));
  return (omax + croot) + r < kSweepHuge;
}

// could a contact at t still win?  (t <= best implies t <= tmax: best starts there)
__device__ __forceinline__ bool sweep_could_win(const Sweep& q, float t, int prim) {
  return (t < q.best) | ((t == q.best) & ((q.best_i < 0) | (prim < q.best_i)));
}

// the certification slack of a centre c
__device__ __forceinline__ float sweep_slack(V3 c, float r) {
  return kSweepSlack * (fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fabsf(c.z)) + r);
}

// one triangle against one sweep.  A candidate that cannot win skips its certification: the answer is the same.
__device__ __forceinline__ void sweep_triangle(Sweep& q, V3 v0, V3 e1, V3 e2, int prim) {
  float t0, u, v;
  closest_triangle(q.o, v0, e1, e2, t0, u, v);
  if (t0 <= q.rr) {                                                // start overlap
    sweep_keep(q, 0.0f, u, v, prim);
    return;
  }
  const V3 w = rtd::sub(q.o, v0), wb = rtd::sub(w, e1), wc = rtd::sub(w, e2);
  float t = sweep_face(w, e1, e2, q.d, q.r);
  t = fminf(t, sweep_edge(w, e1, q.d, q.rr));
  t = fminf(t, sweep_edge(w, e2, q.d, q.rr));
  t = fminf(t, sweep_edge(wb, rtd::sub(e2, e1), q.d, q.rr));
  t = fminf(t, sweep_entry(w, q.d, q.dd, q.rr));
  t = fminf(t, sweep_entry(wb, q.d, q.dd, q.rr));
  t = fminf(t, sweep_entry(wc, q.d, q.dd, q.rr));
  if (!(t < __builtin_inff()) || !sweep_could_win(q, t, prim)) return;
  const V3 c = sweep_axpy(q.o, t, q.d);
  const float rs = q.r + sweep_slack(c, q.r);
  float d2;
  closest_triangle(c, v0, e1, e2, d2, u, v);
  if (d2 <= rs * rs) sweep_keep(q, t, u, v, prim);
}

// one sphere of the scene (its surface) against one sweep
__device__ __forceinline__ void sweep_sphere(Sweep& q, float4 sph, int prim) {
  using M = Math<false>;
  const V3 ctr = {sph.x, sph.y, sph.z};
  const V3 w = rtd::sub(q.o, ctr);
  const float ww = M::dot(w, w);
  const float dist = __builtin_sqrtf(ww);
  const float s0 = fabsf(dist - sph.w);
  if (s0 * s0 <= q.rr) {                                           // start overlap
    sweep_keep(q, 0.0f, 0.0f, 0.0f, prim);
    return;
  }
  float t = __builtin_inff();
  if (dist > sph.w) {                                              // from outside: the entry root against R + r
    const float ro = sph.w + q.r;
    t = sweep_entry(w, q.d, q.dd, ro * ro);
  } else if ((dist < sph.w) & (q.r < sph.w)) {                     // from inside: the exit root against R - r
    const float ri = sph.w - q.r, rri = ri * ri;
    const float bp = -M::dot(w, q.d);
    const V3 l = sweep_axpy(w, bp / q.dd, q.d);
    const float disc = rri - M::dot(l, l);
    const float sq = __builtin_sqrtf(q.dd * disc);
    const float tx = bp > 0.0f ? (bp + sq) / q.dd : (rri - ww) / (sq - bp);
    t = ((disc >= 0.0f) & (tx > 0.0f)) ? tx : __builtin_inff();
  }
  if (!(t < __builtin_inff()) || !sweep_could_win(q, t, prim)) return;
  const V3 c = sweep_axpy(q.o, t, q.d);
  const float rs = q.r + sweep_slack(c, q.r);
  const V3 wc = rtd::sub(c, ctr);
  const float s1 = fabsf(__builtin_sqrtf(M::dot(wc, wc)) - sph.w);
  if (s1 * s1 <= rs * rs) sweep_keep(q, t, 0.0f, 0.0f, prim);
}

// the spheres (prim = n_tris + sphere index), then the sweep's record
__device__ __forceinline__ float4 sweep_finish(const TraceParams& p, Sweep& q) {
  for (uint32_t si = 0; si < p.n_spheres; ++si) sweep_sphere(q, p.spheres[si], static_cast<int>(p.n_tris + si));
  if (q.best_i < 0) return make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
  return make_float4(q.best, q.bu, q.bv, __int_as_float(q.best_i));
}

__global__ __launch_bounds__(256, 4) void spherecast_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ sweeps,
                                                             float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * 256u;           // first sweep of the block
  const uint32_t nb = (n - base < 256u) ? static_cast<uint32_t>(n - base) : 256u;

  float4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = {0.0f, 0.0f, -1.0f, -1.0f};   // padding lanes accept nothing
  if (tid < nb) { s0 = sweeps[2u * (base + tid)]; s1 = sweeps[2u * (base + tid) + 1u]; }
  Sweep q = sweep_load(s0, s1);
  const bool active = sweep_valid(s1.z, s1.w);

  // the triangles; every chunk is scanned, by the waves that hold a sweep that accepts
  scan_triangles<ScanMode::SkipIdleWaves>(p, s_mem, [&] { return active; }, [&](const float4 A0, const float4 A1, auto z, int prim) {
    if (active) sweep_triangle(q, {A1.z, A1.w, z()}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, prim);
  });
  if (tid < nb) {
    float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
    if (active) h = sweep_finish(p, q);
    hits[base + tid] = h;
  }
}

// one 48-byte record against one sweep
__device__ __forceinline__ void sweep_test_record(const float4* __restrict__ rec, Sweep& q) {
  const BvhRecord r = bvh_record(rec);
  sweep_triangle(q, r.v0, r.e1, r.e2, r.idx);
}

// ks = 4 * kSweepSlack and rho_s, both times the tracer's slack (rt_dbg_query_accel_slack)
__global__ __launch_bounds__(64) void spherecast_bvh_kernel(const TraceParams p, const BvhParams b, float ks, float rho_s, uint32_t n,
                                                             const float4* __restrict__ sweeps, float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t lane = threadIdx.x;
  const size_t i = static_cast<size_t>(blockIdx.x) * 64u + lane;
  if (i >= n) return;                                              // (no barrier and no cross-lane operation below)
  const float4 s0 = sweeps[2u * i], s1 = sweeps[2u * i + 1u];
  if (!sweep_valid(s1.z, s1.w)) {
    hits[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    return;
  }
  Sweep q = sweep_load(s0, s1);
  const float tmax = s1.w;

  const OccludedPrune pr = occluded_prune(q.o, q.d);               // prunes at all?  1 / d, max|o|
  const bool prunes = pr.prunes && sweep_range_guard(b, pr.omax, q.r);
  const float rg = q.r + kSweepTiny;                               // (r itself from 2^-47 up)
  const float inf = __builtin_inff();
  auto child = [&](const BvhNode& nd, int c) {
    const float g = rg + (ks * (nd.cmax[c] + q.r) + rho_s * ((pr.omax + nd.cmax[c]) + q.r));
    float enter, exit;
    const bool nan = bvh_slab(nd, c, g, q.o, pr.inv, enter, exit);
    const bool skip = (exit < enter) || (exit < 0.0f) || (enter > q.best);
    return !(prunes && !nan) ? inf : skip ? -inf : fmaxf(-enter, -FLT_MAX);
  };
  auto leaf = [&](const float4* rec) { sweep_test_record(rec, q); return false; };
  const bool overflow = bvh_walk<64u, true>(b, s_mem, lane, true, child, leaf, [&](float key) { return key < -q.best; });
  if (overflow) {                                                  // an entry was not kept: every leaf record, from the start
    q.best = tmax; q.best_i = -1;
    for (uint32_t j = 0; j < b.n_leaf_records; ++j) sweep_test_record(b.records + 3u * j, q);
  }
  for (uint32_t j = 0; j < b.n_always; ++j) sweep_test_record(b.records + 3u * (b.n_leaf_records + j), q);
  hits[i] = sweep_finish(p, q);
}

hipError_t launch_sphere_cast(const TraceParams& p, const BvhParams* b, float slack, uint32_t n, const float* sweeps, float4* hits,
                              hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (sweeps == nullptr || hits == nullptr) return hipErrorInvalidValue;
  const float4* const s4 = reinterpret_cast<const float4*>(sweeps);
  if (b != nullptr) {                                              // one wave per block, lane = sweep, keyed stack entries
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 64u, true);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(spherecast_bvh_kernel, n, 64u, 64u, lds, st, p, *b, 4.0f * kSweepSlack * slack, RT_SWEEP_RHO * slack, n, s4, hits);
  }
  return launch_blocks(spherecast_kernel, n, 256u, 256u, query_chunk_lds_bytes(p.n_tris), st, p, n, s4, hits);
}

}  // namespace rtk
