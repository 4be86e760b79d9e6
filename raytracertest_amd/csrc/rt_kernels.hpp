// rt_kernels.hpp -- launch interface between the host runtime (rt_tracer.cpp) and the
// gfx950 kernels (rt_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <atomic>

namespace rtk {

// Everything rt::TraceKernel receives by value (RayTracer/Kernels.cuh:110-118), for a row
// band [row0, row0+rows) of a W x H image.
constexpr uint32_t kSuperChunk = 1024u, kSuperMaxChunks = 64u;   // super tiles: triangles per chunk list, chunks per scene at most (rt_lists.hpp)

struct TraceParams {
  float4*   render;    // rows*W RGBA float accumulators (mRenderBuffer)
  uint32_t* rng;       // 6 planes of rows*W u32: d, v0..v4 (mRandomStates, SoA); the launches read and write v0..v4 only
  // The two state words that are the same for every pixel of the band travel as scalars (rt_tracer::take_uniform_state):
  // the XORWOW Weyl word d at the start of the launch (every pixel makes 3 draws per sample on every path, a draw adds
  // 362437) and the sample count before it (mSampleCountBuffer; 0 with TRACE_ZERO_ACC).  Plane 0 of `rng` and the count
  // buffer are filled from them when somebody reads them (rt_tracer::materialise).
  uint32_t  weyl, count;
  uint32_t  W, H;      // full image size (camera uses the full height)
  uint32_t  row0, rows;
  uint32_t  npix;      // rows*W
  uint32_t  samples;   // sampleCount of this launch
  float     cam[12];   // mCameraTransformation: xyz of the 4 columns
  float     half_height, aspect, focal, aperture;
  // full 8x8 tiles bound their focal points from the four corner pixels (focal_bounds): tile_curv >= the distance, per
  // component, between a focal point of the tile and the bilinear interpolant of the corners' (host, params());
  // tile_round = the magnitude the rounding allowance of that bound scales with.  tile_curv <= 0: bound over all 64 lanes.
  float     tile_curv, tile_round;
  const float4* tri_a;      // 2 float4 per triangle: (e2.xyz, e1.x), (e1.yz, v0.xy); e1 = v1-v0, e2 = v2-v0
  const float*  tri_b;      // 1 float per triangle: v0.z
  const float4* tri_color;  // abs(normalize(cross(e1,e2)))
  uint32_t  n_tris;
  const float4* spheres;    // centre xyz, radius (build-defined extension)
  uint32_t  n_spheres;
  uint32_t  chunk;          // triangles staged into LDS at a time (full-scan path)
  uint32_t  bin_list;       // candidate records per wave in LDS (binned path), multiple of 64
  uint32_t  block_list;     // block-level pre-cull list (indices) in LDS; 0 = every wave scans the scene
  unsigned long long* stats; // null in the product path; 16 counters for the instrumented launch
  uint32_t* image;     // rows*W BGRA8, written when flags & TRACE_EMIT_IMAGE (mImageBuffer)
  const float4* tri_n; // 3 per triangle: unpacked vertex normals (edge-format scenes with smooth shading), or null
#ifdef RT_TIMELINE
  unsigned long long* timeline;   // experiment builds only (tools/timeline.py): 8 u64 per wave
#endif
  uint32_t* image_host;     // optional second BGRA8 target in pinned host memory (update hand-off), or null
  uint32_t  pretest_on;     // host decision: launches OR TRACE_PRETEST into flags (large-scene kernels)
  uint32_t  iters;          // fused launches: consecutive iterations of p.samples samples (>= 1)
  // Macro-tile triangle lists (scenes larger than the per-wave list): written by macro_bin_kernel
  // once per launch, read by the trace kernel's block-level pre-cull instead of the whole scene.
  // Per macro tile of macro_w x macro_h pixels: count (or 0xFFFFFFFF = overflow, scan the scene)
  // followed by macro_cap ascending triangle indices.  null = no macro level.
  uint32_t* macro_lists;
  uint32_t  macro_cap, macro_w, macro_h, macro_nx;
  // One level above (dense scenes): super tiles of super_f x super_f macro tiles, binned by super_bin_kernel against the whole
  // scene in chunks of 1 024 triangles (rt_lists.hpp); macro_bin_kernel then tests only its super tile's lists.  Per (super
  // tile, chunk): count, then up to 1 024 ascending indices.  null = the macro level scans the scene.
  uint32_t* super_lists;
  uint32_t  super_chunks, super_f, super_nx;
  float*    macro_bounds;   // with super_lists: 8 floats per macro tile -- focal box lo[3], hi[3], ok, any (macro_bounds_kernel)
  uint32_t* tile_lists; // small scenes: per wave tile count | winner << 10 | certain << 31, then bin_list triangle indices
                        // (written by tile_lists_kernel, read by the trace kernel); null: no lists (large scene, no triangles)
  // small scenes, split launches: this kernel traces every second block row of the band -- block row 2 * blockIdx.y + row_phase --
  // so that the two kernels of a launch cost the same whatever the picture (row_il = 0: the grid's rows are the band's)
  uint32_t  row_il, row_phase;
  // list builder (two-level): tiles that will generate rays, counted per half of the band -- [0]: block rows < cost_split_brow,
  // [1]: the others (device counters, published to the host by publish_half_cost; null: not counted)
  uint32_t* half_cost;
  uint32_t  cost_split_brow;
  // small scenes: per triangle, what a pixel of a certain-winner tile accumulates in one launch of p.samples samples --
  // {sum.x, sum.y, sum.z, bits of the BGRA8 word of a freshly cleared pixel} (sure_table_kernel; null: the kernel adds)
  const float4* sure_table;
  // dense scenes (the per-sample forms): the tiles' candidate lists in HBM, written by wave_lists_kernel and read by
  // dense_trace_kernel (rt_dense.hpp): per tile slot of the launch grid (1 + wave_cap) records of 16 dwords; null: the
  // trace kernel classifies on its own (instrumented launches, frames whose lists would not fit)
  uint32_t* wave_lists;
  uint32_t  wave_cap;
  uint32_t  flags;     // TRACE_*
};

// The accumulators are logically zero (first launch after ClearRenderBuffer/ClearSampleCountBuffer,
// RayTracerImpl.cu:242-243): skip their loads and the memsets; 0.0f + x is still evaluated.
constexpr uint32_t TRACE_ZERO_ACC = 1u;
// Also write the BGRA8 image from the updated accumulators (ConverterKernel fused, Kernels.cuh:149-169).
constexpr uint32_t TRACE_EMIT_IMAGE = 2u;
// Hit selection: keep the nearest t > 0 instead of the reference's farthest t (build-defined extension).
constexpr uint32_t TRACE_NEAREST_HIT = 4u;
// (8, 16: were TRACE_LISTS_STORE / TRACE_LISTS_LOAD while the small-scene trace kernels classified on their own; the lists
//  are now always built by tile_lists_kernel and always loaded)
// large-scene kernels: per-sample conservative forms per candidate (9 more floats per LDS record)
constexpr uint32_t TRACE_PRETEST = 32u;
// small-scene kernels: do not skip the intersection tests of tiles whose list is one certainly-hit triangle (A/B, tests)
constexpr uint32_t TRACE_NO_SURE_HIT = 64u;
// small-scene kernels: the waves of certain-winner tiles leave their pixels' xorshift words alone -- no load, no
// rng_discard, no store; the host sums the draws they skipped and rng_settle_kernel pays them later (rt_tracer::settle)
constexpr uint32_t TRACE_OWE_RNG = 128u;

// How the waves of a trace launch get their candidate triangles: trace_kernel's Path.  The host picks it per (half-)launch
// in one place (rt_tracer::trace_path).
enum class TracePath : uint32_t {
  FullScan,        // RT_FLAG_NO_BINNING: the block stages the scene into LDS in chunks and every ray scans all of it
  SmallLists,      // n_tris <= bin_list: each tile's list comes from tile_lists_kernel (p.tile_lists)
  Classify,        // larger scenes: each wave classifies the scene (or its block's and macro tile's survivors) into LDS
  ClassifyForms,   // Classify with the per-sample forms of TRACE_PRETEST: instrumented launches, no macro lists, large frames
  DenseLists,      // forms and lists from HBM (p.wave_lists, wave_lists_kernel): no classification in the trace kernel
};

// jump: J^(2^k), k < 32, 160 columns x 8 words; win: the 4-bit window tables of J^(2^m), m < 6 (rt_rng_host.hpp).
// Writes planes 1..5 (v0..v4); the Weyl word seeded[0] is every pixel's and stays with the host (TraceParams::weyl).
// npix <= kRngInitMaxPixels: the kernel's chunk loop (base += stride, i = base + lane) and the launcher's rounded-up block
// count are 32-bit, and the margin of 2^19 holds the largest stride (512 blocks x 512 threads = 2^18) and that rounding.
constexpr uint64_t kRngInitMaxPixels = (1ull << 32) - (1ull << 19);
hipError_t launch_rng_init(uint32_t* rng, uint32_t npix, uint32_t p0, const uint32_t seeded[6],
                           const uint32_t* jump, const uint32_t* win, hipStream_t st);
// Small scenes: advances v0..v4 of every pixel of the certain-winner tiles of the (half-)launch `p` (p.tile_lists, p.rng and
// the grid of trace_grid(p)) by `draws` xorshift steps.  table: the window table of T^draws in device memory
// (rth::build_window_table), or null = step.
hipError_t launch_rng_settle(const TraceParams& p, uint32_t draws, const uint32_t* table, hipStream_t st);
hipError_t launch_prep_triangles(bool fma, bool edges, const float4* verts, uint32_t n, float4* tri_a, float* tri_b,
                                 float4* color, float4* normals, hipStream_t st);
uint32_t trace_lds_bytes(const TraceParams& p, TracePath path);
// The block grid of the trace launch `p`: one block per 32 x 8 pixels; with row_il only the block rows of its phase
// (groups of row_il block rows, alternating; y may come out 0).  launch_rng_settle walks the same grid.
inline dim3 trace_grid(const TraceParams& p) {
  dim3 grid((p.W + 31u) / 32u, (p.rows + 7u) / 8u);
  if (p.row_il != 0u) {
    const uint32_t R = grid.y, G = p.row_il, full = R / (2u * G), rest = R % (2u * G);
    grid.y = full * G + (p.row_phase == 0u ? (rest < G ? rest : G) : (rest > G ? rest - G : 0u));
  }
  return grid;
}
// Launch descriptors: the hipFunction_t of every trace and list-builder instantiation, resolved from the kernel's host symbol
// the first time it is launched and kept -- a launch through the table skips the runtime's look-up of the host stub and the
// template switch.  A descriptor belongs to a device: one table per tracer.
struct KernelTable {
  std::atomic<hipFunction_t> trace[2][3][2][5][2][2] = {};   // fma, K (1, 2, 4), filter, path, fused iterations, instrumented
  std::atomic<hipFunction_t> lists[2][4] = {};               // fma, builder (launch_tile_lists)
};
// table: null resolves the kernel for this launch only.  stop: an event the launch binds to the kernel -- it completes when the
// kernel does and serves hipStreamWaitEvent on other streams like an event recorded behind it, without a packet of its own
// (where nothing is launched it is recorded instead); null: none.
hipError_t launch_trace(const TraceParams& p, bool fma, bool filter, TracePath path, int K, hipStream_t st, KernelTable* table = nullptr,
                        hipEvent_t stop = nullptr);
int trace_occupancy(int K, size_t lds);
hipError_t launch_convert(const float4* render, uint32_t count, uint32_t* image, uint32_t npix, hipStream_t st);

// The queries below have one launch function each: b == nullptr is the scan of the staged triangles (256-thread blocks), otherwise
// the walk of the tree *b (rt_bvh_walk.hpp; one element per lane).  An argument only one form reads is ignored by the other.  n == 0
// launches nothing; a null array, a K or max_hits outside its range or a stack beyond 64 KiB of LDS is hipErrorInvalidValue.
#define RT_BVH_RHO 0.00390625f      // 2^-8: DESIGN.md 4.3b derives it

// the scene's bounding volume hierarchy as the walks take it (the tree: rt_bvh_host.hpp)
struct BvhParams {
  const float4* nodes;      // 8 float4 per node
  const float4* records;    // 3 float4 per record: (e2.xyz, e1.x), (e1.yz, v0.xy), (v0.z, upload index, 0, 0)
  uint32_t n_nodes;         // 0: no tree (no finite triangle)
  uint32_t n_leaf_records;  // records [0, n_leaf_records) are the leaves', [n_leaf_records, + n_always) the always-tested list
  uint32_t n_always;
  uint32_t stack_cap;       // entries per lane
  float rho;                // RT_BVH_RHO x the tracer's slack
};
// the dynamic LDS of the walks' stacks (rt_bvh_walk.hpp): stride lanes per block, 8-byte keyed or 4-byte entries
uint32_t bvh_stack_lds_bytes(uint32_t stack_cap, uint32_t stride, bool keyed);

// Ray queries (rt_query.hpp, rt_bvh.hpp): n rays {origin xyz, direction xyz} -- or, when `pixels` is not null, the pinhole rays of n
// full-image (x, y) pairs, also written to rays_out when that is not null -- against p's scene under p.flags' hit rule; hits[i] =
// {t, u, v, bits of the int32 primitive}.  The scan with K in {1, 2, 4} rays per lane, or the walk, one ray per lane (K not read).
hipError_t launch_query(const TraceParams& p, const BvhParams* b, bool fma, int K, uint32_t n, const float* rays, const uint32_t* pixels,
                        float* rays_out, float4* hits, hipStream_t st);

// The visibility query (rt_occluded.hpp): n segments {origin xyz, direction xyz, tmin, tmax}, 16-byte aligned; occluded[i] = 1
// when some primitive of p's scene is hit by ray i with tmin <= t <= tmax (closed, plain fp32 comparisons), else 0.  p.flags'
// hit rule plays no part.  The scan with K in {1, 2, 4} rays per lane, or the any-hit walk, one ray per lane (K not read).
hipError_t launch_occluded(const TraceParams& p, const BvhParams* b, bool fma, int K, uint32_t n, const float* segs, uint8_t* occluded,
                           hipStream_t st);

// The exposure query (rt_exposure.hpp): n points {origin xyz, normal xyz, tmin, tmax} and a table of n_dirs (1 .. 64) directions
// {x, y, z, -}, both 16-byte aligned; bit j of masks[i] (8-byte aligned) = 1 when launch_occluded would answer 0 for the segment
// {origin_i, d_ij, tmin_i, tmax_i}, d_ij = direction j in the frame of normal i (flags = 0) or as given (flags = 1); bits >= n_dirs
// are 0.  One wave per point, one lane per direction, in both forms.  launch_exposure_rays / exposure_rays_host: the n * n_dirs
// segments themselves, point-major, from the same function (debug).
hipError_t launch_exposure(const TraceParams& p, const BvhParams* b, bool fma, uint32_t n, const float* points, const float* dirs,
                           uint32_t n_dirs, uint32_t flags, uint64_t* masks, hipStream_t st);
hipError_t launch_exposure_rays(uint32_t n, const float* points, const float* dirs, uint32_t n_dirs, uint32_t flags, float* segs,
                                hipStream_t st);
void exposure_rays_host(size_t n, const float* points, const float* dirs, uint32_t n_dirs, uint32_t flags, float* segs);

// The all-hits query (rt_allhits.hpp): the same segments; row i of hits (max_hits records {t, u, v, bits of the int32 primitive},
// 16-byte aligned) holds the ray's first counts[i] <= max_hits in-interval hits in ascending (t, prim) order, then records
// {0, 0, 0, -1}.  1 <= max_hits <= 16; one ray per lane in both forms.
hipError_t launch_allhits(const TraceParams& p, const BvhParams* b, bool fma, uint32_t n, const float* segs, uint32_t max_hits,
                          float4* hits, uint32_t* counts, hipStream_t st);

// The point query (rt_closest.hpp): n points {x, y, z, d2max}, 16-byte aligned; hits[i] = {squared distance, u, v, bits of the
// int32 primitive} of the nearest candidate with t <= d2max, smallest (t, prim), or {0, 0, 0, -1}.  One arithmetic for both
// math modes; one point per lane in both forms.  rho_c: RT_CLOSEST_RHO x the tracer's slack (the walk's; the scan does not read it).
#define RT_CLOSEST_RHO 3.814697265625e-06f      // 2^-18: DESIGN.md 4.3f derives it
hipError_t launch_closest(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* pts, float4* hits,
                          hipStream_t st);

// The k-nearest point query (rt_nearest.hpp): the same points and rho_c; after (or nullptr) n cursor records, 16-byte aligned; row
// i of hits (max_hits records) holds the point's counts[i] <= max_hits nearest accepted candidates behind its cursor in ascending
// (t, prim) order, then records {0, 0, 0, -1}.  1 <= max_hits <= 16; one point per lane in both forms.
hipError_t launch_nearest(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* pts, const float4* after,
                          uint32_t max_hits, float4* hits, uint32_t* counts, hipStream_t st);

// The three region queries are launch_region<Shape> (rt_overlap.hpp) for one shape each.
// The region query (rt_overlap.hpp): n boxes {lo xyz, -, hi xyz, -}, 16-byte aligned; after (or nullptr) n int32 cursors; row i
// of prims (max_hits int32) holds the min(counts[i], max_hits) lowest accepted prims behind the cursor in ascending order, then
// -1; counts[i] is the total, not capped.  0 <= max_hits <= 16 (0: prims may be nullptr); one arithmetic for both math modes;
// one box per lane in both forms.  The tree form reads neither b->rho nor a slack: its prune is exact.
hipError_t launch_overlap(const TraceParams& p, const BvhParams* b, uint32_t n, const float* boxes, const int* after, uint32_t max_hits,
                          int* prims, uint32_t* counts, hipStream_t st);

// The triangle-shaped region query (rt_trioverlap.hpp): n query triangles {P0 xyz, -, P1 xyz, -, P2 xyz, -}, 16-byte aligned;
// after, max_hits, prims and counts as launch_overlap's.  One arithmetic for both math modes; one query per lane in both forms.
// The tree form reads neither b->rho nor a slack: its prune is exact.
hipError_t launch_overlap_triangles(const TraceParams& p, const BvhParams* b, uint32_t n, const float* tris, const int* after,
                                    uint32_t max_hits, int* prims, uint32_t* counts, hipStream_t st);

// The hexahedron-shaped region query (rt_hexoverlap.hpp): n regions of eight corners {C_k xyz, -}, k = 0 .. 7 in box-like order,
// 16-byte aligned; after, max_hits, prims and counts as launch_overlap's.  One arithmetic for both math modes; one query per
// lane in both forms.  The tree form reads neither b->rho nor a slack: its prune is exact.
hipError_t launch_overlap_hexahedra(const TraceParams& p, const BvhParams* b, uint32_t n, const float* hexa, const int* after,
                                    uint32_t max_hits, int* prims, uint32_t* counts, hipStream_t st);

// The section query (rt_section.hpp): n slabs {nx, ny, nz, d0, d1, -, -, -}, 16-byte aligned; after, max_hits, prims and counts as
// launch_overlap's.  One arithmetic for both math modes; one slab per lane in both forms.  The tree form (a kernel of its own)
// reads neither b->rho nor a slack: its prune is exact.
hipError_t launch_section(const TraceParams& p, const BvhParams* b, uint32_t n, const float* planes, const int* after, uint32_t max_hits,
                          int* prims, uint32_t* counts, hipStream_t st);

// The cut post-pass (rt_section.hpp): n slabs, n * per_plane prims of them (as launch_section wrote them) -> as many 32-byte records
// {p0 xyz, kind, p1 xyz, features}, 16-byte aligned, of the plane n.x = d0 (side 0) or d1 (side 1).  No tree.
hipError_t launch_section_segments(const TraceParams& p, uint32_t n, uint32_t per_plane, uint32_t side, const float* planes, const int* prims,
                                   void* cuts, hipStream_t st);

// The triangle-shaped proximity query (rt_tridistance.hpp): n query triangles {P0 xyz, d2max, P1 xyz, -, P2 xyz, -}, 16-byte
// aligned; hits[i] as launch_closest's for the nearest primitive of the triangle, witness[i] = {the winning point on the query
// triangle, bits of its int32 candidate index}, or {0, 0, 0, -1} in both.  One arithmetic for both math modes; one query per lane
// in both forms.  rho_c as launch_closest's.
hipError_t launch_triangle_distance(const TraceParams& p, const BvhParams* b, float rho_c, uint32_t n, const float* tris, float4* hits,
                                    float4* witness, hipStream_t st);

// The swept query (rt_spherecast.hpp): n sweeps {origin xyz, direction xyz, radius, tmax}, 16-byte aligned; hits[i] = {t of the
// first contact, u, v of the contact point, bits of the int32 primitive} of the smallest (t, prim) among the certified contacts
// with t <= tmax, or {0, 0, 0, -1}.  One arithmetic for both math modes; one sweep per lane in both forms.  slack: the tracer's
// (rt_dbg_query_accel_slack / 1000), which scales the walk's allowance beyond r (the scan does not read it).
constexpr float kSweepSlack = 0.00048828125f;   // RT_SWEEP_SLACK = 2^-11 (include/rt_mi355x.h)
#define RT_SWEEP_RHO 1.52587890625e-05f        // rho_s = 2^-16: DESIGN.md 4.3k derives it
hipError_t launch_sphere_cast(const TraceParams& p, const BvhParams* b, float slack, uint32_t n, const float* sweeps, float4* hits,
                              hipStream_t st);

// The side post-pass (rt_sides.hpp): n points, n * per_point records of them (hits, as the point queries wrote them), the feature
// table (7 float4 per triangle, rt_features_host.hpp) -> n * per_point {s, feature} pairs of 8 bytes.
hipError_t launch_sides(const TraceParams& p, const float4* table, uint32_t n, uint32_t per_point, const float* pts, const float4* hits,
                        void* sides, hipStream_t st);

// Refit of that tree on the device (rt_refit.hpp): the records of the current scene into their slots (flag: set to 1 when a
// slot's triangle changed between finite and non-finite), the boxes of one level's nodes (deepest level first), the tree's cost.
hipError_t launch_refit_gather(const float4* tri_a, const float* tri_b, uint32_t n_tris, float4* records, uint32_t n_leaf_records,
                               uint32_t n_records, uint32_t* flag, hipStream_t st);
hipError_t launch_refit_level(float4* nodes, uint32_t n_nodes, const float4* records, uint32_t n_leaf_records, const uint32_t* level_nodes,
                              uint32_t count, hipStream_t st);
hipError_t launch_refit_cost(const float4* nodes, uint32_t n_nodes, double* out, hipStream_t st);

hipError_t launch_dbg_hit_triangle(bool fma, uint32_t n, const float* rays, const float* tris, int eps_mode,
                                   int* hit, float* tuv, float* normal, float* point, hipStream_t st);
bool trace_can_fuse(TracePath path, bool filter);   // launches with TraceParams::iters > 1 are available
hipError_t launch_macro_bin(const TraceParams& p, bool fma, hipStream_t st);
// the level above: p.super_lists (before launch_macro_bin)
hipError_t launch_super_bin(const TraceParams& p, bool fma, hipStream_t st);
// dense scenes: the per-wave candidate lists + forms of the (half-)launch `p` into p.wave_lists (after launch_macro_bin)
hipError_t launch_wave_lists(const TraceParams& p, bool fma, hipStream_t st);
// one wave that does nothing for `us` microseconds (bounded): the stagger of the first split launch after the tracer was idle
hipError_t launch_delay(uint32_t us, hipStream_t st);
// small scenes: hands the builder's per-half counts (TraceParams::half_cost) to the host -- *host_word = upper | lower << 32 --
// and clears them for the next build
hipError_t launch_publish_half_cost(uint32_t* half_cost, unsigned long long* host_word, hipStream_t st);
// small scenes: the per-triangle table TraceParams::sure_table for launches of `samples` samples
hipError_t launch_sure_table(const float4* colors, uint32_t n_tris, uint32_t samples, float4* out, hipStream_t st);
// small scenes: the tiles' candidate lists + certain-winner verdicts of the (half-)launch `p` into p.tile_lists
// (table, stop: as launch_trace takes them).  kind: where a builder was launched, which of the four (0: region pairs, 1: regions,
// 2: tiles of up to 32 triangles, 3: tiles of up to 64 per step); untouched where nothing was
hipError_t launch_tile_lists(const TraceParams& p, bool fma, hipStream_t st, KernelTable* table = nullptr, hipEvent_t stop = nullptr,
                             int* kind = nullptr);
hipError_t launch_dbg_check_midrange(unsigned long long* out, hipStream_t st);
hipError_t launch_dbg_focal_boxes(bool fma, const TraceParams& p, float* boxes, float* focal, hipStream_t st);
hipError_t launch_dbg_classify(bool fma, bool forms, uint32_t slack_milli, const TraceParams& p, uint32_t level, uint32_t n_regions,
                               const uint32_t* regions, float* out, hipStream_t st);
hipError_t launch_dbg_valu_peak(uint32_t blocks, int iters, float* out, unsigned long long* clk, hipStream_t st);
hipError_t launch_dbg_sincos(uint32_t n, const float* x, float* s, float* c, hipStream_t st);
hipError_t launch_dbg_uniform(uint32_t n, uint32_t m, uint32_t* states, float* out, hipStream_t st);
hipError_t launch_dbg_get_ray(bool fma, const TraceParams& p, uint32_t n, const uint32_t* pixels,
                              uint32_t* states, float* rays, hipStream_t st);

}  // namespace rtk
