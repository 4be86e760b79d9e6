// rt_scan.hpp -- the scan of every triangle of the scene (RT_QUERY_SCAN) as one function, the scan side's counterpart of
// rt_bvh_walk.hpp.  Included by rt_kernels.hip only, behind rt_trace.hpp.  Six of the nine scan kernels call scan_triangles:
// query_kernel, occluded_kernel, closest_kernel, nearest_kernel, spherecast_kernel and tridistance_kernel.  allhits_kernel,
// exposure_kernel and region_kernel state the same loop in their own text (rt_allhits.hpp, rt_exposure.hpp, rt_overlap.hpp: on
// scan_triangles an arm of each measured slower than its parent): a change of the loop is made here and in
// those three.  A query brings its open() and its per-record test as callables; the LDS layout, the staging, the barriers
// and the per-wave skip are stated here.
//
// Shape: 256-thread blocks (kScanThreads), lane = query (query_kernel and occluded_kernel: K queries per lane).  The block
// stages the triangles into LDS in ascending chunks of kQueryChunk 36-byte records -- 2 float4 {e2, e1, v0.x, v0.y} from
// tri_a, then the chunk's v0.z from tri_b behind them (as TracePath::FullScan does) -- with consecutive threads on consecutive
// words, and every lane then reads the chunk's records in ascending order at wave-uniform addresses (two ds_read_b128 and,
// where the query asks for it, one ds_read_b32 per record).  Candidates therefore arrive in ascending upload index c0 + j.
//
// The three modes differ in the barrier between two chunks and in what a wave does after staging:
//   EveryWave      a plain barrier; every wave scans every chunk.  open() is not called.
//   SkipIdleWaves  a plain barrier; a wave none of whose lanes is open skips the chunk's records.
//   StopWhenIdle   as SkipIdleWaves, and the block leaves the loop once no lane of it is open.  The barrier between two
//                  chunks is __syncthreads_or(open): it is needed anyway (the previous chunk is read), it hands every
//                  thread the same verdict, so the break is block-uniform and no barrier is ever under divergent control
//                  flow, and a wave that finished early learns there that another wave still wants the next chunk.
// An idle wave still takes part in staging: the chunk belongs to the block, the staging loops are strided by the block's
// thread count, and both barriers count every wave.  That is why the skip is a `continue` behind the second barrier and
// never a return, and why no thread of a scan kernel may return before the loop.
//
// The first barrier of a chunk separates the reads of what was in this LDS before -- the previous chunk, or what the kernel
// itself put there before the call (query_kernel's rays) -- from the chunk's writes.
//
// The callables:
//   open()                   is this lane still interested?  Evaluated once per chunk by EVERY thread of the block, before the
//                            barrier, so padding lanes must be able to call it (and answer false).  It may change between
//                            chunks (StopWhenIdle's finished rays).
//   test(A0, A1, z, prim)    one record: A0, A1 its two float4, z() its v0.z -- a callable, so that a query whose first stage
//                            rejects the record for the whole wave never loads it -- and prim = c0 + j its upload index.
//                            Called by every lane of a wave that has an open lane: the per-lane `if (active)` stays in the body.
// Neither callable may contain a barrier.  A ballot inside test sees the whole wave: no lane has left the loop.
#pragma once
#include "rt_trace.hpp"

namespace rtk {

constexpr uint32_t kQueryChunk = 1024u;    // triangles per LDS chunk: 36 KiB, four blocks share a CU's 160 KiB
constexpr uint32_t kScanThreads = 256u;    // threads of a scan kernel's block

enum class ScanMode { EveryWave, SkipIdleWaves, StopWhenIdle };

// the dynamic LDS of a scan kernel's staged chunk: min(n_tris, kQueryChunk) records of 36 bytes
static uint32_t query_chunk_lds_bytes(uint32_t n_tris) {
  return (n_tris < kQueryChunk ? n_tris : kQueryChunk) * 36u;
}

template <ScanMode MODE, class Open, class Test>
__device__ __forceinline__ void scan_triangles(const TraceParams& p, float4* s_mem, Open open, Test test) {
  const uint32_t tid = threadIdx.x;
  const uint32_t nt = p.n_tris;
  const uint32_t cap = nt < kQueryChunk ? nt : kQueryChunk;
  float4* const sA = s_mem;                                        // 2 float4 per triangle
  float* const sB = reinterpret_cast<float*>(s_mem + 2u * cap);    // v0.z
  for (uint32_t c0 = 0; c0 < nt; c0 += kQueryChunk) {
    const uint32_t cn = (nt - c0 < kQueryChunk) ? nt - c0 : kQueryChunk;
    bool o = true;
    if constexpr (MODE != ScanMode::EveryWave) o = open();
    if constexpr (MODE == ScanMode::StopWhenIdle) {
      if (__syncthreads_or(o ? 1 : 0) == 0) break;                 // the barrier carries the block's verdict
    } else {
      __syncthreads();                                             // what was here before is read
    }
    for (uint32_t i = tid; i < 2u * cn; i += kScanThreads) sA[i] = p.tri_a[2u * c0 + i];
    for (uint32_t i = tid; i < cn; i += kScanThreads) sB[i] = p.tri_b[c0 + i];
    __syncthreads();
    if constexpr (MODE != ScanMode::EveryWave) {
      if (__builtin_amdgcn_ballot_w64(o) == 0ull) continue;        // an idle wave; it has helped staging
    }
    for (uint32_t j = 0; j < cn; ++j) {
      const float4 A0 = sA[2u * j], A1 = sA[2u * j + 1u];
      test(A0, A1, [&] { return sB[j]; }, static_cast<int>(c0 + j));
    }
  }
}

}  // namespace rtk
