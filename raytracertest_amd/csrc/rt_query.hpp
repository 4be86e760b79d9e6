// rt_query.hpp -- ray queries: caller rays (or the pinhole rays of caller pixels) against the tracer's scene, with the
// renderer's own arithmetic and hit rule (RayTracer/Kernels.cuh:29-92, ThinLensCamera.cuh:111-130).  Included by
// rt_kernels.hip only (rt_lists.hpp defines non-template kernels: a second translation unit would define them twice).
//
// Shape: the scan of rt_scan.hpp (every chunk, every wave), each lane holding K rays -- ray k * 256 + lane of the block, so
// that every load and store of a wave covers one contiguous span.  The block's rays (6 floats each) are read with
// consecutive threads on consecutive floats into LDS and from there into registers; the chunks then go through the same LDS
// and every ray scans all of them through rtk::test_triangle -- the trace kernel's own code, so the arithmetic is the
// renderer's by construction.  Spheres follow (the trace kernel's rule), and the winner's u, v are recomputed once from its
// record with hit_triangle_exact (as the smooth-shading block does: same operations as the scan, same bits).
// Padding lanes (ray index >= n) carry o = d = 0: det = dot(e1, cross(0, e2)) = 0 < 1e-10 culls them at stage A for
// every finite triangle, so they never keep a triangle alive in the ballots; their results are never stored.
#pragma once
#include "rt_scan.hpp"

namespace rtk {

// Output record: {t, u, v, bits of the int32 primitive} (rt_hit).  prim = triangle index, n_tris + sphere index, or -1.
template <bool FMA, int K>
__global__ __launch_bounds__(256, 4) void query_kernel(const TraceParams p, uint32_t n, const float* __restrict__ rays,
                                                        const uint32_t* __restrict__ pixels, float* __restrict__ rays_out,
                                                        float4* __restrict__ hits) {
  extern __shared__ float4 s_mem[];
  const uint32_t tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * (256u * K);      // first ray of the block
  const uint32_t nb = (n - base < 256u * K) ? static_cast<uint32_t>(n - base) : 256u * K;

  V3 o[K], d[K];
  if (pixels == nullptr) {
    // the block's rays, coalesced, through LDS
    float* const sR = reinterpret_cast<float*>(s_mem);
    const float* const src = rays + 6u * base;
    for (uint32_t i = tid; i < 6u * nb; i += 256u) sR[i] = src[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t r = static_cast<uint32_t>(k) * 256u + tid;
      if (r < nb) {
        o[k] = {sR[6u * r], sR[6u * r + 1u], sR[6u * r + 2u]};
        d[k] = {sR[6u * r + 3u], sR[6u * r + 4u], sR[6u * r + 5u]};
      } else {
        o[k] = {0.0f, 0.0f, 0.0f}; d[k] = {0.0f, 0.0f, 0.0f};
      }
    }
  } else {
    // the pixels' pinhole rays (ThinLensCamera.cuh:111-130) with the launch's camera, as the trace kernel makes them
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t r = static_cast<uint32_t>(k) * 256u + tid;
      if (r < nb) {
        const size_t i = base + r;
        pinhole<FMA>(p, pixels[2u * i], pixels[2u * i + 1u], o[k], d[k]);
        if (rays_out != nullptr) {
          float* const out = rays_out + 6u * i;
          out[0] = o[k].x; out[1] = o[k].y; out[2] = o[k].z; out[3] = d[k].x; out[4] = d[k].y; out[5] = d[k].z;
        }
      } else {
        o[k] = {0.0f, 0.0f, 0.0f}; d[k] = {0.0f, 0.0f, 0.0f};
      }
    }
  }

  // false: the reference's rule (farthest t, negative t accepted, Kernels.cuh:73,84); true: nearest t > 0.  Wave-uniform.
  const bool nearest = (p.flags & TRACE_NEAREST_HIT) != 0u;
  float best_t[K];
  int best_i[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    best_t[k] = nearest ? FLT_MAX : -FLT_MAX;                      // :73
    best_i[k] = -1;
  }
  unsigned long long st_exit[4] = {0, 0, 0, 0}, st_skip[4] = {0, 0, 0, 0};   // (no counters: STATS = false)

  // every triangle, ascending (:75, first-scanned wins ties :84); the scan's first barrier comes after the rays are read
  scan_triangles<ScanMode::EveryWave>(p, s_mem, [] { return true; }, [&](const float4 A0, const float4 A1, auto z, int prim) {
    test_triangle<FMA, K, true, false>(A0, A1, z, prim, o, d, best_t, best_i, nearest, true, static_cast<uint32_t>(K), st_exit, st_skip);
  });

  const uint32_t nt = p.n_tris;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t r = static_cast<uint32_t>(k) * 256u + tid;
    if (r < nb) {
      float dist = best_t[k];
      int win = best_i[k];
      for (uint32_t si = 0; si < p.n_spheres; ++si) {              // the trace kernel's sphere rule (rt_trace.hpp)
        float t = 0.0f;
        if (hit_sphere<FMA>(o[k], d[k], p.spheres[si], t) && (nearest ? (t > 0.0f && t < dist) : dist < t)) {
          dist = t;
          win = static_cast<int>(nt + si);
        }
      }
      float4 h = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
      if (win >= 0) {
        h.x = dist;
        h.w = __int_as_float(win);
        if (static_cast<uint32_t>(win) < nt) {                     // u, v of the winner (Kernels.cuh:50,57)
          const float4 A0 = p.tri_a[2 * win], A1 = p.tri_a[2 * win + 1];
          float t = 0.0f, u = 0.0f, v = 0.0f;
          int stage;
          (void)hit_triangle_exact<FMA>(o[k], d[k], {A1.z, A1.w, p.tri_b[win]}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z},
                                        RT_EPS, t, u, v, stage);
          h.y = u; h.z = v;
        }
      }
      hits[base + r] = h;
    }
  }
}

// What the launch functions of the seven query headers share (host).  Each query has ONE launch function, launch_X(p, b, ...):
// b == nullptr is the scan, otherwise the walk of *b; it guards its arguments, picks the instantiation and states the launch
// geometry -- elements per block, threads per block, dynamic LDS -- in its call of launch_blocks.  launch_query is in rt_bvh.hpp.

// query_kernel stages its block's rays (24 bytes each) through the same LDS first
static uint32_t query_lds_bytes(uint32_t n_tris, int K) {
  const uint32_t tris = query_chunk_lds_bytes(n_tris);
  const uint32_t rays = 256u * static_cast<uint32_t>(K) * 24u;
  return tris > rays ? tris : rays;
}

// kern(a...) over n > 0 elements, per_block of them to a block of `threads` threads (the grid rounded up in 64 bits)
template <class... KA, class... A>
hipError_t launch_blocks(void (*kern)(KA...), uint32_t n, uint32_t per_block, uint32_t threads, size_t lds, hipStream_t st,
                         const A&... a) {
  const dim3 grid(static_cast<uint32_t>((static_cast<uint64_t>(n) + per_block - 1u) / per_block));
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, a...);
  return hipGetLastError();
}

}  // namespace rtk
