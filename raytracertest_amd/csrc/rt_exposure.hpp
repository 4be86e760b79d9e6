// rt_exposure.hpp -- the exposure query (rt_tracer_exposure*): a bundle of up to 64 rays per point, made in
// registers from the point's segment record and a direction table all points share, answered as ONE 64-bit mask per point --
// bit j set when direction j is OPEN, i.e. rt_tracer_occluded would answer 0 for {origin, d_j, tmin, tmax}.  Included by
// rt_kernels.hip only, behind rt_occluded.hpp: the hit, the closed fp32 interval, the NaN rules, the triangle stages
// (occluded_test_triangle) and the record test (occluded_test_record) are that file's.
//
// Mapping: one wave is one point, one lane one direction, 256-thread blocks (four points).  The point is two 16-byte loads at
// a wave-uniform address, lane j loads dirs[j] (one coalesced 16-byte load), the ray never leaves registers.  Lanes j >= n_dirs
// and the waves of a partial last block start finished, with a zero direction.  The answer is one __ballot, stored by one
// lane as a plain 8-byte vector store.
//
// exposure_ray is the one statement of the ray generator: both kernels, the debug kernel and the host form of
// rt_dbg_exposure_rays call it.  One arithmetic in both math modes, every operation rounded separately (the build has
// -ffp-contract=off on both sides), the one division correctly rounded.
//
// exposure_kernel (RT_QUERY_SCAN): spheres first, then the scan of rt_scan.hpp in its stop-when-idle mode.  No thread returns
// before the last barrier.  The kernel keeps the scan in its own text -- the chunk loop, the LDS layout, the staging and the
// barriers are A SECOND COPY of rt_scan.hpp's scan_triangles, which is the first: change them together.  On the shared
// function two of its four arms measured slower than the parent by more than the parent's own spread.
//
// exposure_bvh_kernel (RT_QUERY_BVH): every lane runs occluded_bvh_kernel's any-hit walk on its own ray -- occluded_child's
// pruning, spheres and the always-tested list first, the overflow fallback -- with the lane's stack in LDS at entry * 256 + tid.
// No lane returns before the ballot of exposure_store.
#pragma once
#include "rt_occluded.hpp"

namespace rtk {

constexpr uint32_t kExposureMaxDirs = 64u;     // RT_MAX_DIRS: one lane per direction
constexpr uint32_t kExposureWorld = 1u;        // RT_EXPOSURE_WORLD

struct ExposureRay { V3 o, d; float tmin, tmax; };

// Ray j of a point: s0, s1 are the point's record {origin, normal, tmin, tmax}, l = dirs[j] (w ignored).  RT_EXPOSURE_LOCAL:
// l lives in the frame (T, B, n) of the normal n = (x, y, z), the branchless basis of Duff et al. (JCGT 6(1), 2017), written
// out operation by operation in include/rt_mi355x.h:
//   s = copysignf(1, z);  a = -1 / (s + z);  b = (x * y) * a
//   T = (1 + s * ((x * x) * a),  s * b,  -(s * x));   B = (b,  s + (y * y) * a,  -y)
//   d = ((l.x * T + l.y * B) + l.z * n)   per component, in this order
// RT_EXPOSURE_WORLD: d = l; the normal slots enter no arithmetic.
__host__ __device__ __forceinline__ ExposureRay exposure_ray(const float4 s0, const float4 s1, const float4 l, const uint32_t flags) {
  ExposureRay r;
  r.o = {s0.x, s0.y, s0.z};
  r.tmin = s1.z; r.tmax = s1.w;
  if ((flags & kExposureWorld) != 0u) { r.d = {l.x, l.y, l.z}; return r; }
  const float x = s0.w, y = s1.x, z = s1.y;
  const float s = __builtin_copysignf(1.0f, z);
  const float a = -1.0f / (s + z);
  const float b = (x * y) * a;
  const V3 T = {1.0f + s * ((x * x) * a), s * b, -(s * x)};
  const V3 B = {b, s + (y * y) * a, -y};
  r.d = {(l.x * T.x + l.y * B.x) + l.z * x, (l.x * T.y + l.y * B.y) + l.z * y, (l.x * T.z + l.y * B.z) + l.z * z};
  return r;
}

// the wave's point and the lane's direction -> the lane's ray; false: a padding lane (zero direction, starts finished)
__device__ __forceinline__ bool exposure_load(uint32_t n, const float4* __restrict__ points, const float4* __restrict__ dirs,
                                              uint32_t n_dirs, uint32_t flags, size_t& point, ExposureRay& r) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  point = static_cast<size_t>(blockIdx.x) * 4u + wave;
  const bool live = point < n && lane < n_dirs;
  float4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = {0.0f, 0.0f, 0.0f, 0.0f}, l = {0.0f, 0.0f, 0.0f, 0.0f};
  if (point < n) { s0 = points[2u * point]; s1 = points[2u * point + 1u]; }
  if (live) l = dirs[lane];
  r = exposure_ray(s0, s1, l, flags);
  if (!live) r.d = {0.0f, 0.0f, 0.0f};
  return live;
}

// bit j = direction j is open; one lane of a live wave stores the word
__device__ __forceinline__ void exposure_store(uint32_t n, size_t point, bool done, uint32_t n_dirs,
                                               unsigned long long* __restrict__ masks) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long open = __builtin_amdgcn_ballot_w64(!done && lane < n_dirs);
  if (lane == 0u && point < n) masks[point] = open;
}

template <bool FMA>
__global__ __launch_bounds__(256, 4) void exposure_kernel(const TraceParams p, uint32_t n, const float4* __restrict__ points,
                                                           const float4* __restrict__ dirs, uint32_t n_dirs, uint32_t flags,
                                                           unsigned long long* __restrict__ masks) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  size_t point;
  ExposureRay r;
  const bool live = exposure_load(n, points, dirs, n_dirs, flags, point, r);
  const V3 o[1] = {r.o}, d[1] = {r.d};
  const float tmin[1] = {r.tmin}, tmax[1] = {r.tmax};
  bool done[1] = {!live};                                          // padding lanes and padding waves start finished

  // the spheres first: they are few (hit_sphere's one t)
  for (uint32_t si = 0; si < p.n_spheres; ++si) {
    float t = 0.0f;
    if (!done[0] && hit_sphere<FMA>(o[0], d[0], p.spheres[si], t) && tmin[0] <= t && t <= tmax[0]) done[0] = true;
  }

  // the triangles, staged into LDS chunk by chunk, until every ray of the block is finished (rt_scan.hpp's loop in its
  // StopWhenIdle mode)
  const uint32_t nt = p.n_tris;
  const uint32_t cap = nt < kQueryChunk ? nt : kQueryChunk;
  float4* const sA = s_mem;                                        // 2 float4 per triangle
  float* const sB = reinterpret_cast<float*>(s_mem + 2u * cap);    // v0.z
  for (uint32_t c0 = 0; c0 < nt; c0 += kQueryChunk) {
    const uint32_t cn = (nt - c0 < kQueryChunk) ? nt - c0 : kQueryChunk;
    const bool open = !done[0];
    // the barrier between two chunks (the previous one is read) carries the block's verdict: every thread gets the same
    if (__syncthreads_or(open ? 1 : 0) == 0) break;
    for (uint32_t i = tid; i < 2u * cn; i += 256u) sA[i] = p.tri_a[2u * c0 + i];
    for (uint32_t i = tid; i < cn; i += 256u) sB[i] = p.tri_b[c0 + i];
    __syncthreads();
    if (__builtin_amdgcn_ballot_w64(open) == 0ull) continue;       // this point is finished; its wave still helps staging
    for (uint32_t j = 0; j < cn; ++j) {
      const float4 A0 = sA[2u * j], A1 = sA[2u * j + 1u];
      occluded_test_triangle<FMA, 1>(A0, A1, sB[j], o, d, tmin, tmax, done);
    }
  }
  exposure_store(n, point, done[0], n_dirs, masks);
}

template <bool FMA>
__global__ __launch_bounds__(256) void exposure_bvh_kernel(const TraceParams p, const BvhParams b, uint32_t n,
                                                            const float4* __restrict__ points, const float4* __restrict__ dirs,
                                                            uint32_t n_dirs, uint32_t flags, unsigned long long* __restrict__ masks) {
  extern __shared__ float4 s_mem[];
  size_t point;
  ExposureRay r;
  bool done = !exposure_load(n, points, dirs, n_dirs, flags, point, r);   // (no lane returns: the ballot below wants them all)
  const V3 o = r.o, d = r.d;
  const float tmin = r.tmin, tmax = r.tmax;

  for (uint32_t si = 0; si < p.n_spheres && !done; ++si) {
    float t = 0.0f;
    done = hit_sphere<FMA>(o, d, p.spheres[si], t) && tmin <= t && t <= tmax;
  }
  for (uint32_t j = 0; j < b.n_always && !done; ++j)
    done = occluded_test_record<FMA>(b.records + 3u * (b.n_leaf_records + j), o, d, tmin, tmax);

  const OccludedPrune q = occluded_prune(o, d);
  const bool overflow = bvh_walk<256u, false>(
      b, s_mem, threadIdx.x, !done, [&](const BvhNode& nd, int c) { return occluded_child(nd, c, b.rho, q, o, tmin, tmax); },
      [&](const float4* rec) { return done = occluded_test_record<FMA>(rec, o, d, tmin, tmax); }, [](float) { return false; });
  if (overflow && !done) {                                         // an entry was not kept: every leaf record
    for (uint32_t j = 0; j < b.n_leaf_records && !done; ++j) done = occluded_test_record<FMA>(b.records + 3u * j, o, d, tmin, tmax);
  }
  exposure_store(n, point, done, n_dirs, masks);
}

// debug: the n * n_dirs segments the kernels above trace, point-major, through the same device function
__global__ __launch_bounds__(256) void exposure_rays_kernel(uint32_t n, const float4* __restrict__ points, const float4* __restrict__ dirs,
                                                             uint32_t n_dirs, uint32_t flags, float4* __restrict__ segs) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  if (idx >= static_cast<size_t>(n) * n_dirs) return;
  const size_t i = idx / n_dirs;
  const ExposureRay r = exposure_ray(points[2u * i], points[2u * i + 1u], dirs[idx - i * n_dirs], flags);
  segs[2u * idx] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
  segs[2u * idx + 1u] = make_float4(r.d.y, r.d.z, r.tmin, r.tmax);
}

// the same on the host (rt_dbg_exposure_rays without a tracer)
void exposure_rays_host(size_t n, const float* points, const float* dirs, uint32_t n_dirs, uint32_t flags, float* segs) {
  for (size_t i = 0; i < n; ++i) {
    const float* q = points + 8u * i;
    for (uint32_t j = 0; j < n_dirs; ++j) {
      const float* l = dirs + 4u * j;
      const ExposureRay r = exposure_ray(make_float4(q[0], q[1], q[2], q[3]), make_float4(q[4], q[5], q[6], q[7]),
                                         make_float4(l[0], l[1], l[2], l[3]), flags);
      float* s = segs + 8u * (i * n_dirs + j);
      s[0] = r.o.x; s[1] = r.o.y; s[2] = r.o.z; s[3] = r.d.x; s[4] = r.d.y; s[5] = r.d.z; s[6] = r.tmin; s[7] = r.tmax;
    }
  }
}

// the launch functions' own guard (the entry points have checked the same rules with an error text: rt_query_api.hpp)
static bool exposure_launch_ok(const float* points, const float* dirs, uint32_t n_dirs, uint32_t flags, const void* out) {
  return points != nullptr && dirs != nullptr && out != nullptr && n_dirs != 0u && n_dirs <= kExposureMaxDirs && (flags & ~kExposureWorld) == 0u;
}

// four points (waves) to a 256-thread block in both forms; the walk's stacks at stride 256, the reference alone
hipError_t launch_exposure(const TraceParams& p, const BvhParams* b, bool fma, uint32_t n, const float* points, const float* dirs,
                           uint32_t n_dirs, uint32_t flags, uint64_t* masks, hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (!exposure_launch_ok(points, dirs, n_dirs, flags, masks)) return hipErrorInvalidValue;
  const float4* const p4 = reinterpret_cast<const float4*>(points);
  const float4* const d4 = reinterpret_cast<const float4*>(dirs);
  unsigned long long* const m = reinterpret_cast<unsigned long long*>(masks);
  if (b != nullptr) {
    const uint32_t lds = bvh_stack_lds_bytes(b->stack_cap, 256u, false);
    if (!bvh_stack_fits(lds)) return hipErrorInvalidValue;
    return launch_blocks(fma ? exposure_bvh_kernel<true> : exposure_bvh_kernel<false>, n, 4u, 256u, lds, st, p, *b, n, p4, d4, n_dirs, flags, m);
  }
  const uint32_t lds = query_chunk_lds_bytes(p.n_tris);
  if (lds > 65536u) return hipErrorInvalidValue;                   // (kQueryChunk records are 36 KiB)
  return launch_blocks(fma ? exposure_kernel<true> : exposure_kernel<false>, n, 4u, 256u, lds, st, p, n, p4, d4, n_dirs, flags, m);
}

hipError_t launch_exposure_rays(uint32_t n, const float* points, const float* dirs, uint32_t n_dirs, uint32_t flags, float* segs,
                                hipStream_t st) {
  if (n == 0u) return hipSuccess;
  if (!exposure_launch_ok(points, dirs, n_dirs, flags, segs)) return hipErrorInvalidValue;
  const uint64_t blocks = (static_cast<uint64_t>(n) * n_dirs + 255u) / 256u;
  if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exposure_rays_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st, n,
                     reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(dirs), n_dirs, flags,
                     reinterpret_cast<float4*>(segs));
  return hipGetLastError();
}

}  // namespace rtk
