/*
 * rt_mi355x.h -- C ABI of librt_mi355x.so, the MI355X-native drop-in for the RayTracer/
 * sub-project of ipilter/RayTracerTest.
 *
 * The reference's boundary is a C++ class in a static library (RayTracer/RayTracer.h:14-41,
 * callback type RayTracer/RaytracerCallback.h:9); its only caller is
 * OpenGLView/MainFrame.cpp:45,219-220,233,249,254,293,311,438.  This header is the flat
 * extern "C" form of exactly that class -- one entry point per public method, same
 * argument order, units and error behaviour -- so that any FFI (the header-only C++
 * class in include/RayTracer.h, ctypes in raytracertest_amd/api.py, cgo, JNI ...) binds
 * the same symbols.  Plain pointers and sizes only.
 *
 * Declared semantic change (BASELINE.json north_star): the OpenGL PBO interop is cut.  The
 * pointer handed to the callbacks is a HOST-readable BGRA8 image (pinned memory owned by
 * the tracer, valid until the next rt_tracer_resize / rt_tracer_destroy), not a device
 * pointer as in RayTracerImpl.cu:272,304.
 *
 * Error behaviour follows the reference: nothing throws across the API.  Functions that
 * the reference declares void either return void here or an int status that callers may
 * ignore; the text of the last failure is kept (rt_tracer_last_error / rt_last_error).
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK              0
#define RT_ERR_INVALID     1   /* bad argument (e.g. UploadScene size not a multiple of 3) */
#define RT_ERR_NO_DEVICE   2   /* no usable HIP device: the HIP path is mandatory, there is no CPU fallback */
#define RT_ERR_HIP         3   /* a HIP runtime call or kernel launch failed */
#define RT_ERR_STATE       4

#define RT_MATH_FMA        0u  /* default: the documented a*b+c shapes are fused (nvcc -fmad=true analogue) */
#define RT_MATH_STRICT     1u  /* every source-level operation rounds separately */

#define RT_FLAG_NO_FILTER  1u  /* disable the conservative wave-uniform rejections (debug / parity tests) */
#define RT_FLAG_NO_BINNING 2u  /* disable the per-tile triangle classification: every ray scans the whole
                                  list from block-staged LDS chunks (debug / parity tests / A-B) */

#define RT_FLAG_NEAREST_HIT 4u  /* hit selection extension: keep the nearest hit with t > 0 instead of the
                                  reference's farthest hit incl. negative t (Kernels.cuh:73,84).  Not the default. */

#define RT_FLAG_NO_MACRO_BINS 16u /* disable the macro-tile level of the classification (large scenes): every block
                                  pre-culls the whole triangle list (debug / parity tests / A-B) */
#define RT_FLAG_NO_SUPER_BINS 64u /* dense scenes: the macro tiles scan the whole triangle list instead of their super tile's
                                  (debug / parity tests / A-B; the result is the same) */
#define RT_FLAG_NO_SURE_HIT 32u /* small scenes: run the intersection tests also on tiles whose candidate list is one triangle that
                                  every ray of the tile certainly hits (debug / parity tests / A-B; the result is the same) */
#define RT_FLAG_SMOOTH_NORMALS 8u /* shading extension for scenes uploaded with rt_tracer_upload_scene_edges: the
                                  colour is |normalize(w*n0 + u*n1 + v*n2)|, the rows' packed vertex normals
                                  interpolated at the hit (w = (1-u)-v), instead of |face normal| (Kernels.cuh:97-99).
                                  No effect on scenes uploaded as absolute vertices.  Not the default. */

#define RT_BUF_RENDER      0   /* rows*W*4 float  RGBA accumulators   (mRenderBuffer)      */
#define RT_BUF_COUNTS      1   /* rows*W   uint32 sample counts       (mSampleCountBuffer) */
#define RT_BUF_IMAGE       2   /* rows*W   uint32 BGRA8               (mImageBuffer)       */
#define RT_BUF_RNG         3   /* 6 planes of rows*W uint32: d, v0..v4 (mRandomStates)     */
#define RT_BUF_FRAME       4   /* H*W uint32 BGRA8: the gathered frame of a sharded image, on its root only */
#define RT_GROUP_ID_BYTES  128 /* rt_group_unique_id (an ncclUniqueId)                      */

typedef struct rt_tracer rt_tracer;                      /* opaque: rt::RayTracer + rt::RayTracerImpl */
typedef struct rt_float4 { float x, y, z, w; } rt_float4;   /* CUDA's float4, RayTracer.h:34 */

/* rt::CallBackFunction, RaytracerCallback.h:9: (ColorPtr imageBuffer, size_t size in bytes) + user data.
 * Runs on the tracer's render thread (RayTracerImpl.cu:256-272,287-305). */
typedef void (*rt_callback_fn)(uint32_t* imageBuffer, size_t size, void* user);

/* Extensions the reference has no way to express (all optional; zero-initialise + struct_size). */
typedef struct rt_options {
  uint32_t struct_size;        /* sizeof(rt_options) */
  int32_t  device;             /* HIP device ordinal; the reference pins device 0 (GLCanvas.cpp:259-260) */
  uint32_t full_height;        /* 0: the tracer owns the whole image.  Otherwise the image is
                                  imageSize[0] x full_height and this tracer owns the row band
                                  [row_begin, row_begin + imageSize[1])  (multi-GPU sharding) */
  uint32_t row_begin;
  uint32_t use_time_seed;      /* 1: seed = (uint32)time(NULL) like Random.cu:45 (default when no options) */
  uint32_t math_mode;          /* RT_MATH_FMA | RT_MATH_STRICT */
  uint64_t seed;               /* curand_init seed when use_time_seed == 0 */
  uint32_t flags;              /* RT_FLAG_* */
  uint32_t samples_in_flight;  /* samples of a pixel kept in registers per pass (1,2,4; 0 = auto) */
  uint32_t lds_chunk;          /* full-scan path: triangles staged in LDS at a time (0 = auto) */
  uint32_t bin_list;           /* binned path: candidate records per wave in LDS (0 = auto; multiple of 64) */
  uint32_t transport;          /* rt_tracer_create_multi: RT_TRANSPORT_RCCL (default) | RT_TRANSPORT_PEER */
} rt_options;

#define RT_TRANSPORT_RCCL  0u  /* finished tiles travel to the root with grouped ncclSend / ncclRecv (RCCL over xGMI) */
#define RT_TRANSPORT_PEER  1u  /* one process only: the bands' trace kernels store their BGRA8 tiles straight into the root's frame
                                  through a peer mapping (hipDeviceEnablePeerAccess): no collective, no kernels on the root.  Falls
                                  back to RCCL, with the reason in rt_tracer_group_info, when a device may not map the root's memory */

/* ---- the reference's public methods, one to one -------------------------------------- */

/* RayTracer::RayTracer, RayTracer.h:17-22.  imageSize = {width, height} pixels, fov in
 * degrees, cameraAngles in radians.  cameraPosition is stored and ignored exactly like
 * the reference (ThinLensCamera.cuh:54-57,132-141: the camera sits at the world origin).
 * Sizes: a frame (imageSize, or imageSize[0] x full_height) holds at most 2^32 - 1 pixels -- a pixel's random subsequence
 * x + y * width is a 32-bit word, Kernels.cuh:128 -- and ONE tracer at most 2^32 - 2^19 of them; a larger frame is rendered as
 * several row bands (rt_options.full_height / row_begin).  rt_tracer_create_ex, rt_tracer_resize and rt_tracer_set_band refuse
 * anything else with RT_ERR_INVALID before they allocate or release a buffer: the tracer stays as it was. */
int  rt_tracer_create(const uint32_t imageSize[2], const float cameraPosition[3],
                      const float cameraAngles[2], float fov, float focalLength, float aperture,
                      rt_tracer** out);
int  rt_tracer_create_ex(const uint32_t imageSize[2], const float cameraPosition[3],
                         const float cameraAngles[2], float fov, float focalLength, float aperture,
                         const rt_options* options, rt_tracer** out);
/* RayTracer::~RayTracer, RayTracer.h:23: cancels and joins a running trace. */
void rt_tracer_destroy(rt_tracer* t);
/* RayTracer::Trace, RayTracer.h:25-27: asynchronous; cancels+joins a previous run, clears
 * the buffers, runs iterationCount launches of samplesPerIteration samples, fires the
 * update callback when i > 0 && updateInterval > 0 && i % updateInterval == 0 and the
 * finished callback at the end (not when stopped).  RayTracerImpl.cu:69-87,236-315. */
int  rt_tracer_trace(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration,
                     uint32_t updateInterval);
/* RayTracer::Stop, RayTracer.h:28: sets the cancel flag (granularity: one kernel). */
void rt_tracer_stop(rt_tracer* t);
/* RayTracer::Resize, RayTracer.h:29: new buffers, RNG states re-created.  (Joins a running
 * trace first; the reference races here, RayTracerImpl.cu:94-103.) */
int  rt_tracer_resize(rt_tracer* t, const uint32_t size[2]);
/* RayTracer::SetCameraParameters, RayTracer.h:30-32 (fov degrees). */
void rt_tracer_set_camera_parameters(rt_tracer* t, float fov, float focalLength, float aperture);
/* RayTracer::RotateCamera, RayTracer.h:33: angles += delta (radians), matrix rebuilt. */
void rt_tracer_rotate_camera(rt_tracer* t, const float angles[2]);
/* RayTracer::UploadScene, RayTracer.h:34: count float4, three absolute vertices per
 * triangle, .w ignored; count < 3 or count % 3 != 0 is rejected and the previous scene
 * kept (RayTracerImpl.cu:121-125). */
int  rt_tracer_upload_scene(rt_tracer* t, const rt_float4* hostData, size_t count);
/* Same scene in the layout the reference's notes plan for the GPU (Documentation/gpu.meshes.txt:16-17):
 * per triangle v0, e0 = v1 - v0, e1 = v2 - v0, each .w free for a packed vertex normal
 * (rt_pack_normal).  With e0/e1 computed in fp32 the result equals rt_tracer_upload_scene. */
int  rt_tracer_upload_scene_edges(rt_tracer* t, const rt_float4* hostData, size_t count);
/* Corrected form of the reference's experimental normal packing (UnitTests/NormalPackingTest.cpp:10-23):
 * three components in [-1,1] as 8-bit fields in the fraction of one float.  unpack(pack(n)) == n for
 * every n whose components are multiples of 1/127. */
float rt_pack_normal(const float n[3]);
void  rt_unpack_normal(float packed, float n[3]);
/* RayTracer::SetUpdateCallback / SetFinishedCallback, RayTracer.h:36-37. */
void rt_tracer_set_update_callback(rt_tracer* t, rt_callback_fn fn, void* user);
void rt_tracer_set_finished_callback(rt_tracer* t, rt_callback_fn fn, void* user);

/* ---- additive extensions --------------------------------------------------------------- */

/* Block until the render thread of the last rt_tracer_trace has ended.  Returns 1 when it
 * ran to completion (finished callback fired), 0 when it was stopped or failed. */
int  rt_tracer_wait(rt_tracer* t);
/* Re-create the RNG states from an explicit seed (the reference has no seed control). */
int  rt_tracer_set_seed(rt_tracer* t, uint64_t seed);
/* Spheres: count float4 = centre xyz + radius (build-defined, Documentation/ray.sphere.png). */
int  rt_tracer_upload_spheres(rt_tracer* t, const rt_float4* spheres, size_t count);
/* Device-resident form of one Trace for throughput measurement and multi-GPU drivers:
 * enqueue clear + iterationCount trace launches + conversion on the tracer's stream, no
 * callbacks, no host synchronisation.  rt_tracer_sync waits for the stream. */
int  rt_tracer_trace_enqueue(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration);
/* n_steps consecutive passes of rt_tracer_trace_enqueue, enqueued by one call (the host loop of a throughput
 * driver runs inside the library: one lock, no per-step crossing of a foreign-function boundary).  Identical to
 * n_steps calls of rt_tracer_trace_enqueue. */
int  rt_tracer_trace_enqueue_n(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration, uint32_t n_steps);
int  rt_tracer_sync(rt_tracer* t);
/* One iteration of TraceFunct's loop as a building block for external drivers (the
 * multi-GPU progressive path, raytracertest_amd/dist.py): enqueue ONE trace launch of
 * `samples` spp.  clear_first != 0: the accumulators are cleared first (iteration 0,
 * RayTracerImpl.cu:242-243); emit_image != 0: the BGRA8 image is refreshed too (an update or
 * the last iteration, RayTracerImpl.cu:259-270,287-295).  No callbacks, no host sync. */
int  rt_tracer_launch(rt_tracer* t, uint32_t samples, int clear_first, int emit_image);
/* `iterations` consecutive iterations of the loop as ONE launch, bit-identical to `iterations` calls of
 * rt_tracer_launch (the per-iteration accumulate order is kept; state traffic and triangle classification
 * are paid once).  iterations <= rt_tracer_fused_iterations(t, samples) (>= 1; 1 when fusing is unavailable). */
int  rt_tracer_launch_iterations(rt_tracer* t, uint32_t samples, uint32_t iterations, int clear_first, int emit_image);
int  rt_tracer_fused_iterations(rt_tracer* t, uint32_t samples);
/* Small scenes keep each tile's candidate-triangle list (the result of the conservative classification, a
 * camera-dependent acceleration structure) in device memory.  across_traces != 0 (default): the lists stay
 * valid from one Trace to the next until the camera, the lens, the scene, the frame or the arithmetic mode
 * changes; 0: they are reused by the accumulating launches of one Trace only and every Trace classifies
 * afresh (what bench.py's headline figure uses).  Results are identical either way. */
int  rt_tracer_set_list_reuse(rt_tracer* t, int across_traces);
/* Second BGRA8 target of the emitting launches of rt_tracer_launch* / rt_tracer_trace_enqueue: a
 * device-visible buffer of at least rt_tracer_buffer_bytes(t, RT_BUF_IMAGE) bytes (device memory such
 * as a collective's send buffer, or pinned host memory) that the kernel writes alongside RT_BUF_IMAGE --
 * no copy afterwards.  NULL switches it off.  The caller orders its consumers behind the launch
 * (rt_tracer_stream) and keeps the buffer alive. */
int  rt_tracer_set_image_mirror(rt_tracer* t, void* device_visible_image);
/* Sum of the durations of the SAMPLED trace launches (HIP events on the tracer's stream, around
 * every 16th launch and every launch the caller waits for: an event pair costs ~5 us per launch) and
 * their number since the last reset; total_ms / launches = mean launch duration -- of a split launch
 * (see rt_tracer_stream_b) the upper half-frame kernel's, whose execution overlaps the lower half's.  reset_after != 0
 * clears both and makes the next launch a sampled one. */
int  rt_tracer_kernel_time(rt_tracer* t, double* total_ms, uint64_t* launches, int reset_after);
/* The same sampled launches by what they COST: a split launch counts from the start of its upper half to the end of the
 * LATER of its two halves (the lower half runs on rt_tracer_stream_b), an unsplit launch as above.  This is what the load
 * balancer uses (rt_tracer_rebalance, RowBandJob.rebalance): a band whose expensive rows lie in its lower half must not look
 * cheap.  Shares its sample set and its reset with rt_tracer_kernel_time. */
int  rt_tracer_launch_time(rt_tracer* t, double* total_ms, uint64_t* launches, int reset_after);
/* One instrumented launch (clear + trace of `samples` spp with counters; not a timed path).
 * Lane-level counters need RT_FLAG_NO_FILTER (reference-order path), wave-level ones the
 * default filtered path:
 *   out[0..3] ray-triangle tests by the reference's exit point: culled at det
 *             (Kernels.cuh:42), rejected at u (:51), rejected at v (:58), full hit (:63);
 *   out[4..7] (wave, triangle) pairs skipped by the __ballot early-outs after stage A
 *             (culling), B (u), C (v), and pairs that reached the exact stage D;
 *   out[8]    candidate triangles kept by the per-tile classification, summed over waves and
 *             rounds; out[9] classification rounds (one per wave when its list fits in LDS).
 *   out[10]   large scenes: candidate tests of a sample batch skipped by the per-sample forms; small scenes: sample
 *             batches of tiles that skipped their tests because the one candidate is certainly hit;
 *   out[11..15] small scenes: tiles without candidates / with 1 / with a certain winner (any list length) / with 2 /
 *             with more candidates. */
int  rt_tracer_trace_stats(rt_tracer* t, uint32_t samples, uint64_t out[16]);
/* Copy one of the tracer's device buffers to host memory / to another device pointer. */
int  rt_tracer_read_buffer(rt_tracer* t, int which, void* dst, size_t bytes);
int  rt_tracer_copy_buffer_to_device(rt_tracer* t, int which, void* dst_device, size_t bytes);
/* Same copy without the host synchronisation, and the tracer's HIP stream (a hipStream_t) so
 * that a driver can order its own work (e.g. the RCCL tile gather on another stream) behind it
 * with events instead of blocking the host. */
int  rt_tracer_copy_buffer_to_device_async(rt_tracer* t, int which, void* dst_device, size_t bytes);
void* rt_tracer_stream(rt_tracer* t);
/* Trace launches of frames of 128 rows or more run as two half-frame kernels, the upper half on
 * rt_tracer_stream, the lower half on this second stream (consecutive launches then overlap one half's
 * drain with the other half's work).  Every other entry point orders itself behind both; a driver that
 * orders its OWN work behind a launch without blocking either stream records one event on each and
 * waits for both (raytracertest_amd/dist.py), or calls rt_tracer_sync. */
void* rt_tracer_stream_b(rt_tracer* t);
/* The device address of one of the tracer's buffers.  The Weyl word d of the RNG states (plane 0 of RT_BUF_RNG) and the
 * sample count are the same for every pixel of a tracer, so the launches carry them as scalars and do not write these
 * two planes: the read and copy entry points above fill them first, and a pointer obtained here for RT_BUF_RNG or
 * RT_BUF_COUNTS holds d / the counts AS OF THIS CALL (filled on rt_tracer_stream: order behind it or call
 * rt_tracer_sync; ask again after later launches).  Planes 1..5 of RT_BUF_RNG and the other buffers are always current. */
void* rt_tracer_device_pointer(rt_tracer* t, int which);
size_t rt_tracer_buffer_bytes(rt_tracer* t, int which);
/* Launch geometry actually used: out[0]=K, out[1]=lds_chunk, out[2]=dynamic LDS bytes,
 * out[3]=grid.x, out[4]=grid.y, out[5]=n_tris, out[6]=n_spheres, out[7]=device. */
int  rt_tracer_info(rt_tracer* t, uint32_t out[8]);
const char* rt_tracer_last_error(rt_tracer* t);
const char* rt_last_error(void);          /* for failures before a tracer exists */
int  rt_device_count(void);
const char* rt_version(void);

/* ---- ray queries ---------------------------------------------------------------------------
 * What a ray hits in the tracer's scene, under the tracer's own rules: its arithmetic (RT_MATH_FMA / RT_MATH_STRICT) and
 * its hit rule (the reference's farthest hit incl. negative t, or RT_FLAG_NEAREST_HIT).  The answer is exactly what the
 * renderer computes for that ray (HitTriangle, Kernels.cuh:29-65, the scan of :73-92).
 *   rays    n x 6 floats: origin xyz, direction xyz, used as given (Ray(o, d, false): nothing is normalised).
 *   scan    triangles in upload order, then spheres; ties keep the first one scanned (Kernels.cuh:84).  Edge-format scenes
 *           (rt_tracer_upload_scene_edges) are intersected with their uploaded rows.  No scene: every ray misses.
 *   prim    a triangle index in [0, n_tris); n_tris + i for sphere i; RT_PRIM_NONE for no hit.
 *   t u v   a triangle's t, u, v exactly as HitTriangle computes them (:50,:57,:63; t may be negative under the reference
 *           rule); a sphere's t with u = v = 0; no hit: all 0.  NaN, infinite and zero-length rays get whatever the
 *           reference arithmetic gives them.
 * n = 0 is a no-op.  Queries never cancel or join a running Trace (a pick during a progressive render leaves it unchanged):
 * they are serialised with the other calls and read only the scene and the camera.  A query sees the scene of the last
 * upload that returned; uploads and destroy wait for the queries in flight before they replace the scene.  A multi-device
 * handle (rt_tracer_create_multi) answers from its first band; a band tracer of a process group answers locally. */
typedef struct rt_hit { float t, u, v; int32_t prim; } rt_hit;   /* 16 bytes */
#define RT_PRIM_NONE (-1)
/* Host arrays: rays n*6, hits n.  Returns with the hits in host memory. */
int  rt_tracer_intersect(rt_tracer* t, const float* rays, size_t n, rt_hit* hits);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  hits must be 16-byte aligned. */
int  rt_tracer_intersect_device(rt_tracer* t, const float* rays, size_t n, rt_hit* hits, void* stream);
/* n (x, y) pixels in FULL-image coordinates (a band tracer may pick rows outside its band) through their pinhole rays
 * (ThinLensCamera.cuh:111-130) of the camera the tracer holds at the call, computed on the device as the trace kernel does.
 * rays (n*6, or NULL) receives those rays, for the hit point o + t*d.  A pixel outside the image: RT_ERR_INVALID, nothing
 * written.  Returns with the results in host memory. */
int  rt_tracer_pick(rt_tracer* t, const uint32_t* pixels, size_t n, rt_hit* hits, float* rays);
/* Click to focus: picks (x, y); when the hit has prim >= 0 and 0 < t < inf, sets ONLY the focal length to t (for the
 * normalised pinhole direction the focal point sits at focalLength along it, ThinLensCamera.cuh:45) and returns it through
 * focal_length (or NULL).  fov and aperture keep their bits.  Otherwise RT_ERR_INVALID (background, or the hit is not in
 * front of the camera; rt_tracer_last_error says which) and the camera is unchanged.  Like SetCameraParameters it does not
 * join a running Trace. */
int  rt_tracer_focus_at(rt_tracer* t, uint32_t x, uint32_t y, float* focal_length);

/* Opt-in acceleration of the four entry points above: a bounding volume hierarchy (BVH) over the uploaded triangles, built on the
 * host by the first query after an upload (UploadScene / UploadSceneEdges invalidate it, UploadSpheres does not; the build waits
 * for no Trace) and walked per ray on the device.  RT_QUERY_SCAN is the default and launches exactly the kernels described
 * above.  A multi-device handle forwards both calls to its first band.
 * With RT_QUERY_BVH the answer is the scan's -- same prim, and t, u, v with the same bits, under both hit rules, both arithmetic
 * modes, both scene layouts, with spheres (scanned after the triangles as before) -- for every ray whose scan winner is WELL
 * CONDITIONED: in float64, det / (|d| |e1| |e2|) >= 2^-10, det = e1 . (d x e2) of the record the kernel intersects.  The
 * reason: the boxes prune by geometry, and for a ray within rounding of a triangle's plane the fp32 test's det, u and v are
 * noise, so that the scan may report a hit the line passes nowhere near; no finite padding of a box covers that.  For a ray
 * whose scan winner is not well conditioned the BVH mode may return another primitive that the exact test accepts, or none; it
 * never returns a primitive the exact test rejects.  Rays with a non-finite component, a zero direction, or for which the box
 * arithmetic yields a NaN take no pruning decision and get the scan's answer unconditionally.  All of this is said of scenes
 * whose hit arithmetic stays finite in fp32: its products are cubic in a record's size and distance from the origin, and beyond
 * about 2^42 they overflow -- the exact test can then report t = +inf for a triangle behind the ray, which follows no geometry
 * and which the tree does not reproduce. */
#define RT_QUERY_SCAN 0u   /* default: every ray scans every triangle */
#define RT_QUERY_BVH  1u
int  rt_tracer_set_query_accel(rt_tracer* t, uint32_t mode);
/* out = {mode, tree valid (0/1), nodes, leaves, max depth (levels of nodes), triangles in the always-tested list, host build
 * time in us, device bytes of the tree}; the last six are 0 while no valid tree exists. */
int  rt_tracer_query_accel_info(rt_tracer* t, uint64_t out[8]);

/* What an upload does to the tree of RT_QUERY_BVH.  RT_ACCEL_REBUILD (default) is the behaviour described above.  Under
 * RT_ACCEL_REFIT the next RT_QUERY_BVH query REFITS instead of building when a tree has been built (for any earlier upload),
 * its record count equals the scene's triangle count, and rt_tracer_query_accel_rebuild has not been called since: the tree keeps
 * its topology, every record slot takes the 36 bytes of the triangle with its upload index, and every box is recomputed on the
 * device from the leaves up -- about ten small launches instead of a read-back, a host build and an upload.  The upload layout may
 * differ between the two uploads (only the records matter); several uploads without a query in between are fine (the refit reads
 * the current records only).  The first tree, a changed triangle count and an explicit rebuild build as before; UploadSpheres
 * touches nothing.
 * Contract: a refitted tree is a valid bounding tree of the new records, so every RT_QUERY_BVH contract above and below holds word
 * for word, rho and rt_dbg_query_accel_slack included.  Only speed depends on how far the geometry moved: the tree's COST -- the sum
 * over all nodes and their present children of half_area(child box), in double, divided by the half area of the union of the
 * root's child boxes; 0 without nodes or when that union has no area -- is reported so that a caller can notice the degradation
 * and call rt_tracer_query_accel_rebuild.  Nothing rebuilds by itself.
 * Partition rule: a refit never moves a triangle between the leaves and the always-tested list.  A triangle is FINITE when its
 * nine record floats and its outward-rounded box are finite.  If a leaf's triangle became non-finite or an always-tested one
 * finite, the refit is abandoned and the tree is built on the host instead; out[2] counts these.
 * A multi-device handle forwards all three calls to its first band. */
#define RT_ACCEL_REBUILD 0u   /* default: an upload invalidates the tree, the next RT_QUERY_BVH query rebuilds it on the host */
#define RT_ACCEL_REFIT   1u   /* an upload of the same number of triangles keeps the tree's topology; the next query refits its boxes on the device */
int  rt_tracer_set_query_accel_update(rt_tracer* t, uint32_t policy);   /* other values: RT_ERR_INVALID */
/* Drops the tree now: the next RT_QUERY_BVH query builds afresh, whatever the policy. */
int  rt_tracer_query_accel_rebuild(rt_tracer* t);
/* out = {policy, refits since the last build, refits that fell back to a build (over the tracer's life), device time of the last
 * refit in us, tree cost now, tree cost at the last build (both doubles, bit-cast; 0 while no valid tree exists), the stack
 * entries per lane the walks of the valid tree run with (3 x its depth unless rt_dbg_query_stack_cap lowered it; 0 without a
 * valid tree), 0} */
int  rt_tracer_query_accel_update_info(rt_tracer* t, uint64_t out[8]);

/* Visibility (shadow rays, line of sight, ambient occlusion): is ray i blocked within its own t interval?
 *   segs      n x 8 floats: origin xyz, direction xyz (used as given, nothing normalised), tmin, tmax.
 *   occluded  occluded[i] = 1 when some primitive of the tracer's scene is hit by ray i with tmin <= t <= tmax, else 0.
 *   hit       HitTriangle (Kernels.cuh:29-65) returns true in the tracer's arithmetic mode (RT_MATH_FMA / RT_MATH_STRICT) for
 *             the record the renderer intersects (edge-format scenes: their uploaded rows); t is the value of :63, exactly as
 *             rt_tracer_intersect reports it.  A sphere counts with the one t its ray-sphere test computes.
 *   interval  closed, compared in plain fp32: tmin <= t && t <= tmax.  A NaN t or a NaN bound never occludes; tmin > tmax never
 *             occludes; +-inf bounds are allowed, and [-inf, +inf] means any hit at all, negative t included.
 * The answer is an OR over the primitives: it does not depend on RT_FLAG_NEAREST_HIT nor on the order of the tests.  No scene:
 * every ray is unoccluded; spheres alone are enough to occlude; n = 0 is a no-op.  NaN, infinite and zero-length rays get
 * whatever the reference arithmetic gives them.  Scheduling is that of the other queries: never cancels or joins a running
 * Trace, serialised with the other calls, waited for by uploads and destroy; a multi-device handle answers from its first
 * band, a band tracer locally.
 * RT_QUERY_SCAN (default): exact, the OR described above.  RT_QUERY_BVH: the same tree and box inflation as the other
 * queries, under the any-hit form of their contract.  Call an accepted in-interval triangle WELL CONDITIONED when, in float64,
 * det / (|d| |e1| |e2|) >= 2^-10.  Then BVH = 1 implies scan = 1 (never an occluder the exact test rejects); BVH = scan when
 * scan = 0; BVH = scan when at least one in-interval occluder of the ray is well conditioned or is a sphere.  The two may
 * differ only when every in-interval occluder of a ray is ill conditioned.  A ray with a non-finite component, a zero
 * direction or a NaN in its box arithmetic takes no pruning decision and gets the scan's answer; triangles with a non-finite
 * record are always tested. */
/* Host arrays: segs n*8, occluded n.  Returns with the answers in host memory. */
int  rt_tracer_occluded(rt_tracer* t, const float* segs, size_t n, uint8_t* occluded);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  segs must be 16-byte aligned (a ray is two 16-byte loads); otherwise RT_ERR_INVALID. */
int  rt_tracer_occluded_device(rt_tracer* t, const float* segs, size_t n, uint8_t* occluded, void* stream);

/* Exposure (ambient occlusion, sky-view factor, light-map visibility, several lights shadowed at once): a bundle of up to
 * RT_MAX_DIRS rays from each point, in one fixed pattern, answered as one bit mask per point.  The rays are made on the device, in
 * registers; the caller never materialises them.
 *   points    n x 8 floats, laid out exactly like a segment of rt_tracer_occluded: origin xyz, NORMAL xyz in the direction slots,
 *             tmin, tmax.  The normal is used as given: the caller supplies a unit normal, the library does not normalise and
 *             does not check.
 *   dirs      n_dirs x 4 floats {x, y, z, w}; w is ignored.  All points share the table.
 *   n_dirs    1 .. RT_MAX_DIRS; otherwise RT_ERR_INVALID (whatever n is).
 *   flags     RT_EXPOSURE_LOCAL (0): the directions live in the frame of each point's normal, z along the normal (below).
 *             RT_EXPOSURE_WORLD (1): the directions are used as given; the normal slots are not read into any arithmetic, so NaNs
 *             there change nothing (sky view, a set of sun positions, several lights).  Any other bit: RT_ERR_INVALID.
 *   masks     n x uint64.  Bit j of masks[i] is set when direction j from point i is OPEN: rt_tracer_occluded would answer 0
 *             for the segment {origin_i, d_ij, tmin_i, tmax_i}.  Bits j >= n_dirs are 0.
 *   hit, interval, NaN   rt_tracer_occluded's, word for word: HitTriangle returns true in the tracer's arithmetic mode for the
 *             record the renderer intersects, t is the value of Kernels.cuh:63, a sphere counts with the one t of its ray-sphere
 *             test; the interval is closed and compared in plain fp32; a NaN t or a NaN bound never occludes and tmin > tmax
 *             never occludes, so such a point has every bit j < n_dirs set.  Triangles are single-sided (the hit test culls back
 *             faces, as for rt_tracer_occluded); spheres count.  The answer is an OR over the primitives and does not depend on
 *             RT_FLAG_NEAREST_HIT.
 *   frame     one arithmetic in both math modes, fp32, every operation rounded separately (nothing fused), the one division
 *             correctly rounded: the branchless orthonormal basis of Duff et al. (JCGT 6(1), 2017).  With the normal
 *             n = (x, y, z) and a table entry l:
 *                 s = copysignf(1, z)           (z = -0 takes s = -1)
 *                 a = -1 / (s + z)
 *                 b = (x * y) * a
 *                 T = (1 + s * ((x * x) * a),   s * b,               -(s * x))
 *                 B = (b,                       s + (y * y) * a,     -y)
 *                 d.c = ((l.x * T.c + l.y * B.c) + l.z * n.c)        for c = x, y, z, in this order
 *             (T, B, n) is right-handed and orthonormal to rounding for a unit n.  A non-finite normal yields NaN directions:
 *             they never occlude and take no pruning decision, exactly as rt_tracer_occluded treats such a ray.
 * No scene: every bit j < n_dirs is set; spheres alone are enough to occlude; n = 0 is a no-op; a NULL array with n > 0 is
 * RT_ERR_INVALID.  Scheduling is that of the other queries: never cancels or joins a running Trace, serialised with the other
 * calls, on the query stream or the caller's, waited for by uploads and destroy; a multi-device handle answers from its first
 * band, a band tracer locally.
 * RT_QUERY_SCAN (default): exact.  RT_QUERY_BVH: every ray walks the tree as a ray of rt_tracer_occluded does (the same box test,
 * rho, rt_dbg_query_accel_slack and RT_ACCEL_REFIT), so bit j is the complement of what rt_tracer_occluded answers for that
 * segment in that mode, under the any-hit contract stated there. */
#define RT_MAX_DIRS 64u
#define RT_EXPOSURE_LOCAL 0u
#define RT_EXPOSURE_WORLD 1u
/* Host arrays: points n*8, dirs n_dirs*4, masks n.  Returns with the masks in host memory. */
int  rt_tracer_exposure(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags,
                        uint64_t* masks);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  points and dirs must be 16-byte aligned, masks 8-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_exposure_device(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags,
                               uint64_t* masks, void* stream);

/* All hits along a ray (seeing through surfaces, wall thickness, point-in-solid by the parity of the crossings, the nearest hit
 * in front of the origin under any hit rule): the first max_hits hits of ray i within its own t interval, in order.
 *   segs      n x 8 floats, exactly as rt_tracer_occluded takes them: origin, direction used as given, tmin, tmax.
 *   max_hits  1 .. RT_MAX_HITS; otherwise RT_ERR_INVALID.
 *   hits      n * max_hits records.  Row i (hits + i * max_hits) holds counts[i] <= max_hits hits, then records
 *             {0, 0, 0, RT_PRIM_NONE}.
 *   counts    counts[i] = hits stored for ray i.  counts[i] == max_hits means there MAY be more.  To continue, call again
 *             with tmin = the last stored t and skip the (t, prim) pairs already seen -- the interval is closed, so hits with
 *             that same t come again, which is what keeps coincident surfaces from being lost.
 *   hit       rt_tracer_occluded's definition word for word: HitTriangle returns true in the tracer's arithmetic mode for the
 *             record the renderer intersects (edge-format scenes: their uploaded rows), t is the value of Kernels.cuh:63; a
 *             sphere counts with the one t of its ray-sphere test and u = v = 0 (prim = triangle count + sphere index).  The
 *             interval is closed and compared in plain fp32; a NaN t, a NaN bound or tmin > tmax gives no hit; [-inf, +inf]
 *             means every hit, negative t included.
 *   order     ascending t; equal t (==, so -0 equals +0) by ascending prim.  The rule names no visiting order and does not
 *             depend on RT_FLAG_NEAREST_HIT.
 *   bits      t, u and v of a stored hit are exactly what rt_tracer_intersect reports for that (ray, primitive).
 * No scene: every count is 0; spheres alone can be hit; n = 0 is a no-op; a NULL array with n > 0 is RT_ERR_INVALID.
 * Scheduling is that of the other queries: never cancels or joins a running Trace, serialised with the other calls, waited for
 * by uploads and destroy; a multi-device handle answers from its first band, a band tracer locally.
 * RT_QUERY_SCAN (default): exact.  RT_QUERY_BVH: let E be the ray's exact set of in-interval hits, and W the subset of E made
 * of the spheres and of the WELL CONDITIONED triangles (in float64, det / (|d| |e1| |e2|) >= 2^-10).  The answer is the first
 * max_hits elements, in the order above, of some set E' with W <= E' <= E: it never stores a hit the exact test rejects or
 * that lies outside the interval, the bits are the scan's, only ill-conditioned hits may be lost, and what is kept is what the
 * rule gives on the rest.  A ray with a non-finite component, a zero direction or a NaN in its box arithmetic takes no pruning
 * decision and gets the scan's answer; triangles with a non-finite record are always tested. */
#define RT_MAX_HITS 16u
/* Host arrays: segs n*8, hits n*max_hits, counts n.  Returns with the results in host memory. */
int  rt_tracer_intersect_all(rt_tracer* t, const float* segs, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  segs and hits must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_intersect_all_device(rt_tracer* t, const float* segs, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts,
                                    void* stream);

/* ---- point queries --------------------------------------------------------------------------
 * The nearest surface point of the tracer's scene to a point, and how far away it is (proximity and collision tests, snapping a
 * camera target to the geometry, distance-field sampling, "which triangle did I click next to").
 *   pts         n x 4 floats: x, y, z, d2max -- the SQUARED search radius of that point; +inf = unbounded.
 *   out         out[i] = rt_hit with t = the squared distance, u, v = the nearest point's barycentrics, prim as in the ray queries
 *               (a triangle index in [0, n_tris); n_tris + i for sphere i).  The nearest point is v0 + u*e1 + v*e2 of the
 *               triangle's record, for the caller to form (a sphere: centre + radius * (p - centre) / |p - centre|).
 *   candidates  every triangle through the record the renderer intersects (v0, e1, e2); for edge-format scenes
 *               (rt_tracer_upload_scene_edges) these are the uploaded rows.  Every sphere through its surface.
 *   triangle    Ericson's closest point on a triangle restated on the record.  There is no reference arithmetic to be faithful
 *               to, so it is the same in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation,
 *               division is correctly rounded, dot products are (x*x' + y*y') + z*z'.
 *                 With ap = p - v0:  a = e1.e1, b = e1.e2, c = e2.e2, d1 = e1.ap, d2 = e2.ap,
 *                                    d3 = d1 - a, d4 = d2 - b, d5 = d1 - b, d6 = d2 - c;
 *                 vc = d1*d4 - d3*d2,  vb = d5*d2 - d1*d6,  va = d3*d6 - d5*d4.
 *                 The first of these regions that holds gives (u, v):
 *                   1. d1 <= 0 && d2 <= 0                       (0, 0)
 *                   2. d3 >= 0 && d4 <= d3                      (1, 0)
 *                   3. vc <= 0 && d1 >= 0 && d3 <= 0            (d1 / (d1 - d3), 0)
 *                   4. d6 >= 0 && d5 <= d6                      (0, 1)
 *                   5. vb <= 0 && d2 >= 0 && d6 <= 0            (0, d2 / (d2 - d6))
 *                   6. va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), (1 - w, w)
 *                   7. otherwise                                den = 1 / ((va + vb) + vc), (vb * den, vc * den)
 *                 Then r = (ap - u*e1) - v*e2 per component, and t = r.r.
 *   sphere      w = p - centre, s = |sqrt(w.w) - radius| with the correctly rounded sqrt, t = s*s, u = v = 0, prim = n_tris + i.
 *   accepted    a candidate is accepted when t <= d2max in plain fp32.  A NaN t is never accepted; a NaN or negative d2max
 *               accepts nothing.
 *   winner      the accepted candidate with the smallest (t, prim): equal t (==) goes to the lowest prim.  The rule names no
 *               visiting order and does not depend on RT_FLAG_NEAREST_HIT.
 *   no winner   {0, 0, 0, RT_PRIM_NONE}.
 * No scene: every answer is that; spheres alone can win; n = 0 is a no-op; a NULL array with n > 0 is RT_ERR_INVALID.
 * Scheduling is that of the ray queries: never cancels or joins a running Trace, serialised with the other calls, on the query
 * stream or the caller's, waited for by uploads and destroy; a multi-device handle answers from its first band, a band tracer
 * locally.
 * RT_QUERY_SCAN (default): every point tests every candidate.  RT_QUERY_BVH: the ray queries' tree (built, or under
 * RT_ACCEL_REFIT refitted, by the first query after an upload), walked nearest box first; bit for bit the scan's answer for
 * every point whose three coordinates are finite.  There is no conditioning clause: a distance, unlike a ray against a plane it
 * grazes, is well conditioned; regions 1-7 yield u, v in [0, 1] by the signs they test and region 7 divides by a sum of three
 * positives, so a computed closest point never leaves its triangle's box by more than rounding, which the box test's allowance
 * rho_c covers (rt_dbg_query_accel_slack scales it as it scales rho).  A point with a non-finite coordinate takes no pruning
 * decision; triangles with a non-finite record stay in the always-tested list and go through the same rule.
 * Range.  The rule has no absolute constant, so a scene and its points multiplied by 2^k answer the same u, v and prim and t
 * times 2^2k -- while the fourth powers of a length it forms (va, vb, vc; region 7 divides by their sum) stay within fp32: for
 * inputs of order 1, k = -31 .. 31.  Beyond that range the interior region's u and v are the first to go (a sum that is +inf
 * or whose reciprocal is: the record answers NaN and is not accepted), then t itself below 2^-63 or above 2^63; scan and tree
 * still agree bit for bit at every scale, and denormals are kept, not flushed (tests/range_cases.py, test_gpu_query_range.py).
 * Accuracy, as measured (K = 64, four times the largest value seen): with scale = max|p| + the largest |vertex
 * coordinate| and eps = 2^-24, sqrt(t) >= D - K*eps*scale for D the true distance to the nearest triangle -- the reported
 * distance is never below the true one by more than rounding -- and sqrt(t) <= D_ws + K*eps*scale for D_ws the true distance to
 * the nearest WELL-SHAPED triangle (smallest corner-angle sine >= 2^-6): within rounding of the true one whenever the truly
 * nearest triangle is well shaped. */
/* Host arrays: pts n*4, out n.  Returns with the answers in host memory. */
int  rt_tracer_closest_point(rt_tracer* t, const float* pts, size_t n, rt_hit* out);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  pts and out must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_closest_point_device(rt_tracer* t, const float* pts, size_t n, rt_hit* out, void* stream);

/* The k nearest primitives to a point, in order (collision broad phase: every triangle a sphere touches; contact sets at edges
 * and corners; blending the nearest few surfaces; "what else is near where I clicked"), with a cursor that enumerates ALL
 * primitives within the radius however many there are.
 *   pts         n x 4 floats, exactly as rt_tracer_closest_point takes them: x, y, z, d2max (the SQUARED search radius).
 *   max_hits    1 .. RT_MAX_HITS; otherwise RT_ERR_INVALID.
 *   candidates, arithmetic and acceptance are rt_tracer_closest_point's word for word: one arithmetic for both math modes; a
 *               candidate is accepted when t <= d2max in plain fp32; a NaN t is never accepted; a NaN or negative d2max accepts
 *               nothing.
 *   after       optional (NULL: none): n records, the cursor of a continuation.  Where after[i].prim != RT_PRIM_NONE a candidate
 *               of point i is additionally accepted only if it sorts strictly behind (after[i].t, after[i].prim): t > after.t,
 *               or t == after.t && prim > after.prim with prim compared as int32.  A NaN after.t accepts nothing.  u and v of
 *               the cursor are ignored.
 *   order       ascending t; equal t (==) by ascending prim.  The rule names no visiting order.
 *   hits        n * max_hits records.  Row i (hits + i * max_hits) holds counts[i] <= max_hits records in that order, then
 *               records {0, 0, 0, RT_PRIM_NONE}.
 *   counts      counts[i] = records stored for point i.  counts[i] == max_hits means there MAY be more.  To continue, call again
 *               with after[i] = the row's last stored record: nothing is repeated and nothing is lost, coincident surfaces
 *               included.
 *   bits        t, u and v of a stored record are exactly what the triangle rule (or the sphere rule) of rt_tracer_closest_point
 *               gives for that (point, primitive).  So with after == NULL record 0 of every row equals rt_tracer_closest_point's
 *               answer bit for bit, for every max_hits.
 * No scene: every count is 0; spheres alone can answer; n = 0 is a no-op; NULL pts, hits or counts with n > 0 is RT_ERR_INVALID.
 * Scheduling is rt_tracer_closest_point's; a multi-device handle answers from its first band, a band tracer locally.
 * RT_QUERY_SCAN (default): every point tests every candidate.  RT_QUERY_BVH: rt_tracer_closest_point's walk, pruning against
 * min(d2max, the t of the list's last entry once the list is full) instead of against one best; bit for bit the scan's answer,
 * counts included, for every point whose three coordinates are finite.  There is no conditioning clause, and the range over
 * which answers rescale with the scene is rt_tracer_closest_point's (fourth powers: k = -31 .. 31).  A child is skipped
 * only when its lower bound lies strictly above that bound, so it holds no record that could enter the list; the cursor takes
 * no pruning decision. */
/* Host arrays: pts n*4, after n or NULL, hits n*max_hits, counts n.  Returns with the results in host memory. */
int  rt_tracer_closest_all(rt_tracer* t, const float* pts, const rt_hit* after, size_t n, uint32_t max_hits, rt_hit* hits,
                           uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  pts, after (where given) and hits must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_closest_all_device(rt_tracer* t, const float* pts, const rt_hit* after, size_t n, uint32_t max_hits, rt_hit* hits,
                                  uint32_t* counts, void* stream);

/* ---- signed point queries ------------------------------------------------------------------------
 * Which side of the nearest surface a point lies on (is it inside the mesh, how far has a contact penetrated, which side of a
 * wall is the camera on, sampling a signed distance field).  The hit half of the answer IS rt_tracer_closest_point's answer; the
 * side half is a post-pass over those records (one kernel, one lane per record), so the searches are the point queries' own.
 *   pts         n x 4 floats, exactly as rt_tracer_closest_point takes them: x, y, z, d2max (the SQUARED search radius).
 *   hits        hits[i] is bit for bit rt_tracer_closest_point's out[i] in the current query mode.
 *   sides       sides[i] = rt_side {s, feature} of hits[i]:
 *     triangle  the triangle rule of rt_tracer_closest_point is evaluated again on the record of hits[i].prim -- the same
 *               operations on the same operands, so the same region and the same residual r = (ap - u*e1) - v*e2 per component.
 *               feature = the part of the triangle that holds the nearest point: RT_FEATURE_FACE 0 (region 7); 1, 2, 3 the
 *               vertices A = v0, B = v0 + e1, C = v0 + e2 (regions 1, 2, 4); 4, 5, 6 the edges AB, AC, BC (regions 3, 5, 6).
 *               N = the fp32 unit normal of that feature in the scene's feature table (below), and
 *                 s = (r.x*N.x + r.y*N.y) + r.z*N.z
 *               every operation one separately rounded fp32 operation, the same in RT_MATH_FMA and RT_MATH_STRICT.
 *     sphere    feature = RT_FEATURE_SPHERE 7, w = p - centre, s = sqrt(w.w) - radius with the correctly rounded sqrt (the
 *               operands of the point query's sphere rule, without the absolute value).
 *     none      hits[i].prim == RT_PRIM_NONE (or any prim outside the scene): {0, RT_FEATURE_NONE}.
 *   reading s   s > 0: the front side of the surface (outside, for a closed mesh wound outward); s < 0: the back side; s == 0:
 *               on the surface, or undecided (a degenerate feature has the zero normal).  No epsilon is applied.  The signed
 *               distance is copysign(sqrt(hits[i].t), s), for the caller to form.
 *   feature table   seven unit normals per triangle in the order above (7 x 16 bytes, .w = 0): the angle-weighted pseudonormals of
 *               Baerentzen & Aanaes, whose dot product with p - c has the right sign at faces, edges and vertices alike (a face
 *               normal alone gives the wrong sign at a sharp convex vertex or a concave edge).  Computed in float64 from the
 *               uploaded fp32 positions, each component rounded to fp32 at the end:
 *                 face    (B - A) x (C - A), normalised.  A triangle whose cross product is zero or not finite contributes
 *                         nothing anywhere and its own face entry is the zero vector.
 *                 vertex  the sum over the incident contributing triangles, in ascending triangle index, of (the interior angle
 *                         at the vertex, atan2(|a x b|, a . b) of its two edge vectors) * (the unit face normal), normalised.
 *                 edge    the sum of the unit face normals of all contributing triangles that share the undirected edge, in
 *                         ascending index, normalised (one triangle at a boundary edge, three or more at a non-manifold one).
 *                 a zero sum gives the zero vector.
 *               Vertices are welded by their exact fp32 bits, -0 taken as +0: the uploaded absolute vertex for
 *               rt_tracer_upload_scene; fp32 v0, v0 + e0, v0 + e1 for rt_tracer_upload_scene_edges.  The tracer keeps one host
 *               copy of the rows of its last upload for this.  The table is built on the host by the first signed query after
 *               an upload and uploaded once; RT_ACCEL_REFIT does not refit it, it is rebuilt.
 * No scene: every answer is {0, 0, 0, RT_PRIM_NONE} and {0, RT_FEATURE_NONE}; spheres alone can win; n = 0 is a no-op; a NULL
 * array with n > 0 is RT_ERR_INVALID.
 * Scheduling is that of the ray queries: never cancels or joins a running Trace, serialised with the other calls, on the query
 * stream or the caller's, waited for by uploads and destroy; a multi-device handle answers from its first band, a band tracer
 * locally.  RT_QUERY_SCAN and RT_QUERY_BVH decide how hits are found, exactly as for rt_tracer_closest_point; sides are a
 * function of (point, record, table) and do not depend on the mode.  Range: rt_tracer_closest_point's (k = -31 .. 31 for
 * inputs of order 1); s rescales by 2^k, the feature does not change. */
typedef struct rt_side { float s; int32_t feature; } rt_side;   /* 8 bytes */
#define RT_FEATURE_NONE   (-1)
#define RT_FEATURE_FACE   0
#define RT_FEATURE_SPHERE 7
/* Host arrays: pts n*4, hits n, sides n.  Returns with the answers in host memory. */
int  rt_tracer_signed_distance(rt_tracer* t, const float* pts, size_t n, rt_hit* hits, rt_side* sides);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation once the scene's table exists.  pts and hits must be 16-byte aligned, sides 8-byte aligned; otherwise
 * RT_ERR_INVALID. */
int  rt_tracer_signed_distance_device(rt_tracer* t, const float* pts, size_t n, rt_hit* hits, rt_side* sides, void* stream);
/* The sides of records the caller already has: hits holds n * per_point records, row i (hits + i * per_point) those of point i
 * -- per_point = 1 for rt_tracer_closest_point's answers, max_hits for rt_tracer_closest_all's rows, whose unfilled records
 * {0, 0, 0, RT_PRIM_NONE} come back as {0, RT_FEATURE_NONE}.  per_point outside 1 .. RT_MAX_HITS is RT_ERR_INVALID.  Only prim
 * of a record is read; sides[j] is what rt_tracer_signed_distance defines for (point j / per_point, hits[j].prim).
 * Host arrays: pts n*4, hits n*per_point, sides n*per_point. */
int  rt_tracer_closest_sides(rt_tracer* t, const float* pts, const rt_hit* hits, size_t n, uint32_t per_point, rt_side* sides);
/* Device pointers, as rt_tracer_signed_distance_device. */
int  rt_tracer_closest_sides_device(rt_tracer* t, const float* pts, const rt_hit* hits, size_t n, uint32_t per_point, rt_side* sides,
                                    void* stream);

/* ---- region queries ------------------------------------------------------------------------------
 * Which primitives of the tracer's scene touch an axis-aligned box (surface voxelisation, the broad phase of box colliders,
 * "select everything inside this volume", building a grid over the scene).
 *   boxes       n x 8 floats: lo.x lo.y lo.z _ hi.x hi.y hi.z _ (two 16-byte loads, like a segment).  The two pad floats are
 *               never read into any arithmetic: NaNs there change nothing.
 *   max_hits    0 .. RT_MAX_HITS; above that RT_ERR_INVALID.  With 0 only the counts are produced and prims may be NULL.
 *   after       optional (NULL: none): n cursors.  Where after[i] != RT_PRIM_NONE a primitive of box i is accepted only if
 *               prim > after[i], compared as int32.
 *   prims       n * max_hits int32.  Row i (prims + i * max_hits) holds the min(counts[i], max_hits) LOWEST accepted prims in
 *               ascending order, then RT_PRIM_NONE.  Numbering as in the other queries: a triangle's upload index, n_tris + i
 *               for sphere i.
 *   counts      counts[i] = the TOTAL number of accepted primitives of box i behind its cursor, not capped.  counts[i] >
 *               max_hits means exactly "there are more": call again with after[i] = the row's last prim; nothing repeats and
 *               nothing is lost.  (The total is free: the order names the lowest prims, so every overlapping leaf is visited.)
 *   triangle    one arithmetic in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation, dot
 *               products are (x*x' + y*y') + z*z', cross products (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y);
 *               min and max are IEEE minNum / maxNum (a NaN operand is dropped).  On the record the renderer intersects
 *               (v0, e1, e2; for edge-format scenes the uploaded rows), with corners A = v0, B = fl(v0 + e1), C = fl(v0 + e2):
 *                 1. Box step.  Per axis: tmin = min(min(A, B), C), tmax = max(max(A, B), C).  Accepted only if, on all three
 *                    axes, lo <= hi, neither B nor C is a NaN (a NaN A makes both one), tmin <= hi and tmax >= lo.  Plain
 *                    comparisons, closed: touching counts.  So a NaN anywhere in the box bounds or the record, or lo > hi on an
 *                    axis, rejects.
 *                 2. Plane step.  c = 0.5*lo + 0.5*hi,  h = 0.5*hi - 0.5*lo  per axis;  n = e1 x e2;  a = A - c;
 *                    s = n.a,  r = h.|n|  (|n| per component).  Separated when |s| > r.
 *                 3. The nine axes unit_k x f of Akenine-Moller's separating-axis test.  With a = A - c, b = B - c, c' = C - c:
 *                      f = e1       on the corners P = a, Q = c'
 *                      f = c' - b   on the corners P = a, Q = b
 *                      f = a - c'   on the corners P = a, Q = b
 *                    (the two corners whose projections differ in exact arithmetic) and for each f, with p(V) on V = P, Q:
 *                      k = x:  p = f.y*V.z - f.z*V.y,  r = h.y*|f.z| + h.z*|f.y|
 *                      k = y:  p = f.z*V.x - f.x*V.z,  r = h.x*|f.z| + h.z*|f.x|
 *                      k = z:  p = f.x*V.y - f.y*V.x,  r = h.x*|f.y| + h.y*|f.x|
 *                    Separated on an axis when  p(P) > r && p(Q) > r  or  p(P) < -r && p(Q) < -r.
 *               A triangle is accepted when step 1 accepts and nothing in steps 2-3 is separated.  Steps 2-3 reject only when a
 *               "separated" is TRUE, so a NaN there (products overflow for boxes near FLT_MAX: inf - inf) never rejects.  A
 *               zero-area triangle gets what this arithmetic gives it (n = 0: the plane step never separates); it is not
 *               special-cased.
 *   sphere      a sphere is its surface, as in the point queries.  Centre s, radius r, per axis a = lo - s, b = s - hi:
 *                 g = max(max(a, b), 0),  f = max(|a|, |b|);  d2min = (gx*gx + gy*gy) + gz*gz,  d2max = (fx*fx + fy*fy) + fz*fz.
 *               Accepted when lo <= hi on every axis and d2min <= r*r && r*r <= d2max.  A box wholly inside the ball touches
 *               nothing, just as a box inside a closed mesh touches no triangle.
 *   infinite    bounds on the right side (lo = -inf and / or hi = +inf: a half space, a slab, all of space) are valid boxes: steps
 *               2-3 then compute with inf and NaN and never separate, so exactly what step 1 accepts is accepted.  lo = +inf or
 *               hi = -inf is lo > hi: nothing.
 *   accuracy    as measured (tests/test_overlap_expect.py): against the 13-axis separating-axis test in float64
 *               on the same fp32 corners, the largest disagreement margin seen is "none in 2 000 000 pairs" of random triangles
 *               and boxes, and none in 2 000 000 pairs of the same inputs snapped to multiples of 1/4, where touching is exact.
 * No scene: every count is 0; spheres alone can answer; n = 0 is a no-op; NULL boxes or counts with n > 0, or NULL prims with
 * max_hits > 0, is RT_ERR_INVALID, and the outputs are then untouched.
 * Scheduling is that of the other queries: never cancels or joins a running Trace, serialised with the other calls, on the query
 * stream or the caller's, waited for by uploads and destroy; a multi-device handle answers from its first band, a band tracer
 * locally.
 * RT_QUERY_SCAN (default): every box tests every primitive.  RT_QUERY_BVH: the ray queries' tree (built, or under RT_ACCEL_REFIT
 * refitted, by the first query after an upload).  A child is entered when its box and the query box overlap -- clo <= hi &&
 * chi >= lo per axis, the same closed comparisons, NO inflation -- and the result is bit for bit the scan's rows and counts for
 * every input whatsoever.  rt_dbg_query_accel_slack has no effect on this query.  Why scan and tree agree:
 *   - a leaf record's tree box is the box of the corners v0, v0 + e1, v0 + e2 evaluated in double and rounded outward; the fp32
 *     corners fl(v0 + e) lie between the exact sum rounded down and rounded up;
 *   - so step 1's [tmin, tmax] lies inside the record's tree box, which lies inside every ancestor's child box: a child the
 *     walk skips holds only triangles step 1 rejects;
 *   - acceptance is a pure function of (box, record, cursor), and a walk visits every record at most once;
 *   - triangles with a non-finite record sit in the always-tested list and go through the same rule; spheres are never in the
 *     tree and are scanned after the triangles;
 *   - a walk whose stack overflowed recomputes from every leaf record, restarting the list and the count.
 * Range.  The triangle rule compares projections on cross products (cubes of a length) and the sphere rule squares: a scene and
 * its boxes multiplied by 2^k answer the same rows for k = -62 .. 63 on inputs of order 1; beyond, separations are lost (rows
 * gain prims) as the products reach +inf or 0.  Scan and tree agree at every scale. */
/* Host arrays: boxes n*8, after n or NULL, prims n*max_hits (NULL allowed when max_hits = 0), counts n.  Returns with the
 * results in host memory. */
int  rt_tracer_overlap(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                       uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  boxes must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_overlap_device(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                              uint32_t* counts, void* stream);
/* Which primitives of the tracer's scene touch a TRIANGLE (the narrow phase of mesh against mesh, a portal given as two
 * triangles, a scene's own self-intersections; for a cut PLANE see rt_tracer_section, under section queries).
 *   tris        n x 12 floats: P0.x P0.y P0.z _ P1.x P1.y P1.z _ P2.x P2.y P2.z _ (three 16-byte loads).  The three pad floats
 *               are never read into any arithmetic: NaNs there change nothing.
 *   max_hits, after, prims, counts
 *               exactly as in rt_tracer_overlap: max_hits 0 .. RT_MAX_HITS (above that RT_ERR_INVALID; 0: counts only, prims
 *               may be NULL); row i holds the min(counts[i], max_hits) LOWEST accepted prims in ascending order, then
 *               RT_PRIM_NONE; counts[i] is the TOTAL behind the cursor, not capped; after[i] = the row's last prim continues:
 *               nothing repeats and nothing is lost.
 *   triangle    one arithmetic in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation, dot
 *               products are (x*x' + y*y') + z*z', cross products (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y);
 *               min and max are IEEE minNum / maxNum.  On the record the renderer intersects (v0, e1, e2; for edge-format scenes
 *               the uploaded rows), with corners A = v0, B = fl(v0 + e1), C = fl(v0 + e2):
 *                 1. Box step.  All nine query coordinates are finite: otherwise the query accepts NOTHING, spheres included.
 *                    Neither B nor C is a NaN (a NaN A makes both one).  Per axis, with tmin = min(min(A, B), C),
 *                    tmax = max(max(A, B), C), qmin = min(min(P0, P1), P2), qmax = max(max(P0, P1), P2): tmin <= qmax and
 *                    tmax >= qmin.  Plain comparisons, closed: touching counts.
 *                 2. Move by -P0.  a = A - P0, b = B - P0, c = C - P0, p1 = P1 - P0, p2 = P2 - P0 per component; the query's own
 *                    corner P0 is the literal 0.
 *                 3. Seventeen axes.  With f = {e1, c - b, a - c}, g = {p1, p2 - p1, p2}, n = e1 x e2 and m = p1 x p2:
 *                      n;  m;  the nine f_i x g_j;  the three n x f_i;  the three m x g_j
 *                    (the last six lie in the two triangles' planes: they are what decides a coplanar pair).  On an axis x the
 *                    record projects to x.a, x.b, x.c and the query to 0, x.p1, x.p2.  Separated on x when EVERY record
 *                    projection is > EVERY query projection, or every one is <: nine plain comparisons each way, so a NaN
 *                    projection makes its comparisons false and the axis never separates.
 *               A triangle is accepted when step 1 accepts and no axis separates.  All six points are projected on every axis
 *               (this is not the two-corner shortcut of rt_tracer_overlap), which buys a guarantee: a query corner that is
 *               bit-equal to A, B or C of a record makes that record accepted, whatever the rounding elsewhere -- the shared
 *               point's projections are the same fp32 operations on the same operands on both sides, so on no axis is every
 *               record projection strictly beyond every query projection, and step 1 is closed.  (P0 against A, B or C: the
 *               moved corner is the difference of equal numbers, +0, against the literal 0.)  Zero-area triangles on either
 *               side get what this arithmetic gives them (a zero axis projects everything to 0 and never separates); they are
 *               not special-cased.
 *   sphere      a sphere of the scene is its surface, as in rt_tracer_overlap.  Centre S, radius r:  d2min = the t of
 *               rt_tracer_closest_point's triangle rule for the point S on the query's own record (v0 = P0, e1 = p1, e2 = p2);
 *               d2max = max(max(w0.w0, w1.w1), w2.w2) with w_i = P_i - S.  Accepted when the query is finite and
 *               d2min <= r*r && r*r <= d2max.  A triangle wholly inside the ball touches nothing.
 *   accuracy    as measured (tests/test_trioverlap_expect.py): against an independently written separating-axis
 *               test in float64 on the same fp32 corners, and against an edge-through-triangle test in float64.
 * Everything else -- no scene, spheres alone, n = 0, NULL arrays (RT_ERR_INVALID, outputs untouched), scheduling, multi-device
 * handles, RT_ACCEL_REFIT -- is rt_tracer_overlap's.
 * RT_QUERY_BVH: a child is entered when its box and the query triangle's BOUNDING BOX [qmin, qmax] overlap -- clo <= qmax &&
 * chi >= qmin per axis, the same closed comparisons, NO inflation -- and the result is bit for bit the scan's rows and counts for
 * every input whatsoever, by the argument above: step 1's [tmin, tmax] lies inside the record's tree box, a child the walk skips
 * holds only triangles step 1 rejects, acceptance is a pure function of (query, record, cursor), non-finite records go through
 * the always-tested list, and a walk whose stack overflowed recomputes from every leaf record, restarting the list and the count.
 * There is no rho, no slack and no conditioning clause: rt_dbg_query_accel_slack has no effect on this query either.
 * Range.  The rows of a scene and its query triangles multiplied by 2^k are the same rows for k = -36 .. 31 on inputs of order 1
 * (the sphere rule goes through closest_triangle's fourth powers; the axes' cubes reach further); beyond, separations are lost. */
/* Host arrays: tris n*12, after n or NULL, prims n*max_hits (NULL allowed when max_hits = 0), counts n.  Returns with the
 * results in host memory. */
int  rt_tracer_overlap_triangles(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                 uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  tris must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_overlap_triangles_device(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits,
                                        int32_t* prims, uint32_t* counts, void* stream);
/* Which primitives of the tracer's scene touch a HEXAHEDRON: the convex hull of eight corners in a box-like order.  An oriented
 * or sheared box, a frustum (a rectangle of pixels between near and far, what a camera, light or portal sees, a froxel), a
 * pyramid (the near corners all at the apex), a wedge, an axis-aligned box and a segment (near corners equal, far corners equal)
 * are all instances.
 *   hexa        n x 32 floats: eight rows C_k.x C_k.y C_k.z _, k = 0 .. 7 (eight 16-byte loads).  The eight pad floats are never
 *               read into any arithmetic: NaNs there change nothing.  The corner order is box-like: bit 0 of k is the side along
 *               the region's first direction, bit 1 along the second, bit 2 along the third; C0 .. C3 are one cap (a frustum's
 *               near rectangle) and C4 .. C7 the other.
 *   max_hits, after, prims, counts
 *               exactly as in rt_tracer_overlap: max_hits 0 .. RT_MAX_HITS (above that RT_ERR_INVALID; 0: counts only, prims
 *               may be NULL); row i holds the min(counts[i], max_hits) LOWEST accepted prims in ascending order, then
 *               RT_PRIM_NONE; counts[i] is the TOTAL behind the cursor, not capped; after[i] = the row's last prim continues:
 *               nothing repeats and nothing is lost.
 *   triangle    one arithmetic in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation, dot
 *               products are (x*x' + y*y') + z*z', cross products (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y);
 *               min and max are IEEE minNum / maxNum.  On the record the renderer intersects (v0, e1, e2; for edge-format scenes
 *               the uploaded rows), with corners A = v0, B = fl(v0 + e1), C = fl(v0 + e2):
 *                 1. Box step.  All 24 corner coordinates are finite: otherwise the query accepts NOTHING, spheres included.
 *                    Neither B nor C is a NaN (a NaN A makes both one).  Per axis, with tmin = min(min(A, B), C),
 *                    tmax = max(max(A, B), C), qmin = min_k C_k, qmax = max_k C_k: tmin <= qmax and tmax >= qmin.  Plain
 *                    comparisons, closed: touching counts.
 *                 2. Move by -C0.  a = A - C0, b = B - C0, c = C - C0, h_k = C_k - C0 per component; the region's own corner
 *                    C0 is the literal 0 (h_0 = 0: h_k - h_0 below is h_k).
 *                 3. Forty-three axes.  With f = {e1, c - b, a - c}:
 *                      the record's normal e1 x e2;
 *                      six face normals, each the cross product of the face's two diagonals, (h_d - h_a) x (h_c - h_b), for the
 *                      faces (a, b, c, d) = (0,2,4,6), (1,3,5,7), (0,1,4,5), (2,3,6,7), (0,1,2,3), (4,5,6,7);
 *                      the 36 crosses f_i x g_e, g_e = h_j - h_i for the twelve edges (i, j) = (0,1), (2,3), (4,5), (6,7),
 *                      (0,2), (1,3), (4,6), (5,7), (0,4), (1,5), (2,6), (3,7).
 *                 4. Projection.  On an axis x the record projects to x.a, x.b, x.c and the region to 0, x.h_1 .. x.h_7.  The
 *                    axis separates when the record's minimum is > the region's maximum, or its maximum < the region's
 *                    minimum, and none of the ten projections is a NaN: a NaN projection never separates.  A degenerate face
 *                    or edge gives a zero axis, which projects everything to 0 and separates nothing.
 *               A triangle is accepted when step 1 accepts and no axis separates.  The region's own projections on its six face
 *               normals do not depend on the record; an implementation may compute them once per query (the same operations
 *               on the same operands).
 *               What this promises.  For a region with volume whose faces are planar the 43 axes are the complete set of
 *               separating axes of two convex polyhedra (face normals of both, edge crosses): this is the exact closed touching
 *               test, up to fp32 rounding.  For ANY eight finite corners it is a pure function of (corners, record, cursor),
 *               identical in scan and tree.  A region WITHOUT volume (all corners in one plane, or on one line) that lies in a
 *               record's own plane may be accepted though the two are apart: the in-plane edge normals of a flat region are
 *               not among the axes.  A non-planar face is read as its two diagonals' cross product; the test then answers for
 *               a region close to, not exactly, the hull.
 *   sphere      a sphere of the scene is its surface, as in rt_tracer_overlap.  Centre S, radius r, s = S - C0:
 *                 inside = none of the six face normals x separates s from the corners: !(x.s > max(0, x.h_k) or
 *                          x.s < min(0, x.h_k)), the region's projections as in step 4, a NaN never separating;
 *                 d2min  = inside ? 0 : the smallest (minNum) t of rt_tracer_closest_point's triangle rule for the point S over
 *                          the twelve face triangles (a, b, d) and (a, d, c) of each face above, each as the record
 *                          v0 = C_a, e1 = C_b - C_a, e2 = C_d - C_a (resp. C_d - C_a, C_c - C_a), on the corners as given;
 *                 d2max  = max_k (C_k - S).(C_k - S).
 *               Accepted when the query is finite and d2min <= r*r && r*r <= d2max.  A sphere wholly inside the region is
 *               accepted (the region is a solid); a region wholly inside the ball touches nothing.  A region WITHOUT volume
 *               (a segment, a flat quadrilateral) has face normals that are all zero or all parallel, which separate no
 *               centre, or only along one direction: every centre counts as inside a segment, and a sphere is then accepted
 *               whenever the region's farthest corner is outside the ball, though the two may be apart.
 *   accuracy    as measured (tests/test_hexoverlap_expect.py): against an independently written separating-axis
 *               test in float64 on the same fp32 corners, against a float64 clipping of the record by the six face planes, and
 *               for segments against a float64 segment-through-triangle test.
 * Everything else -- no scene, spheres alone, n = 0, NULL arrays (RT_ERR_INVALID, outputs untouched), scheduling, multi-device
 * handles, RT_ACCEL_REFIT -- is rt_tracer_overlap's.
 * RT_QUERY_BVH: a child is entered when its box and the region's BOUNDING BOX [qmin, qmax] overlap -- clo <= qmax &&
 * chi >= qmin per axis, the same closed comparisons, NO inflation -- and the result is bit for bit the scan's rows and counts for
 * every input whatsoever: step 1's [tmin, tmax] lies inside the record's tree box, a child the walk skips holds only triangles
 * step 1 rejects, acceptance is a pure function of (corners, record, cursor), non-finite records go through the always-tested
 * list, and a walk whose stack overflowed recomputes from every leaf record, restarting the list and the count.  There is
 * no rho, no slack and no conditioning clause: rt_dbg_query_accel_slack has no effect on this query either.
 * Range.  The rows of a scene and its regions multiplied by 2^k are the same rows for k = -32 .. 30 on inputs of order 1 (the
 * sphere rule's d2min goes through closest_triangle's fourth powers, on coordinates up to 2.25 in the measured lattice); beyond,
 * separations are lost. */
/* Host arrays: hexa n*32, after n or NULL, prims n*max_hits (NULL allowed when max_hits = 0), counts n.  Returns with the
 * results in host memory. */
int  rt_tracer_overlap_hexahedra(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                 uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  hexa must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_overlap_hexahedra_device(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits,
                                        int32_t* prims, uint32_t* counts, void* stream);

/* ---- one frame sharded over several GPUs --------------------------------------
 * The reference builds ONE rt::RayTracer pinned to device 0 (OpenGLView/MainFrame.cpp:44-45,
 * OpenGLView/GLCanvas.cpp:259-260).  Pixels are independent and a pixel's RNG stream is keyed by its
 * global index (Random.cu:21-27), so the frame splits into contiguous row bands -- band k of n owns the rows
 * [k*H/n, (k+1)*H/n) -- that are traced with no exchange; the finished BGRA8 tiles are gathered to the
 * root (the device of band 0) with RCCL over xGMI (grouped ncclSend / ncclRecv; tiles of bands on the root
 * device are written in place by the trace kernel) and handed to the host from there. */

/* ---- swept queries -------------------------------------------------------------------------------
 * A sphere of radius r moves from o along d: when and where does it first touch the tracer's scene (collision of a moving body --
 * a camera or character controller, a projectile with a size; clearance along a path; sphere-trace style marching against a mesh).
 *   sweeps      n x 8 floats with the slots of an rt_tracer_occluded segment: origin xyz, direction xyz (used as given, NOT
 *               normalised), the RADIUS r in the tmin slot, tmax.  The sphere's centre is c(t) = o + t*d for 0 <= t <= tmax.
 *               Accepted: r >= 0 and finite, tmax >= 0 (+inf allowed).  A NaN, negative or infinite r, or a NaN or negative tmax,
 *               accepts nothing.  NaN, infinite or zero directions and origins get whatever the arithmetic below gives.
 *   hits        hits[i] = rt_hit with t = the time of first contact, u, v = the barycentrics of the contact point (the nearest
 *               point of the winning triangle to c(t): v0 + u*e1 + v*e2 of its record; 0, 0 for a sphere), prim as in the other
 *               queries (a triangle's upload index; n_tris + i for sphere i).  No contact: {0, 0, 0, RT_PRIM_NONE}.
 *   sides       contact is two-sided: no winding, no culling, no hit rule (RT_FLAG_NEAREST_HIT plays no part), as in the point
 *               queries.  A zero-area triangle collides as the segment or point it is.
 *   arithmetic  one in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation, division and sqrt
 *               correctly rounded, dot products (x*x' + y*y') + z*z', cross products (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x,
 *               a.x*b.y - b.x*a.y), min is IEEE minNum.  "closest(p)" below is the triangle rule of rt_tracer_closest_point on the
 *               same record, giving (t, u, v).
 *   triangle    on the record the renderer intersects (v0, e1, e2; for edge-format scenes the uploaded rows), with rr = r*r,
 *               dd = d.d, w = o - v0, wb = w - e1, wc = w - e2:
 *                 1. Start overlap.  closest(o).t <= rr: the contact is t = 0 with that evaluation's (u, v).
 *                 2. Otherwise the smallest of seven entry roots, each +inf where its conditions fail (any NaN fails them):
 *                    ball(m, g, a, q), the line m + t*g against the ball of squared radius q about the origin, a = g.g:
 *                        b = -(m.g),  l = m + (b/a)*g per component,  disc = q - l.l,  t = (m.m - q) / (b + sqrt(a*disc));
 *                        conditions  b > 0 && disc >= 0 && t > 0.
 *                    cyl(m, e), the cylinder of radius r about the edge from m's origin along e:
 *                        ee = e.e,  s0 = (m.e)/ee,  sd = (d.e)/ee,  m' = m - s0*e,  d' = d - sd*e per component,
 *                        t = ball(m', d', d'.d', rr),  s = s0 + t*sd;  conditions  0 <= s && s <= 1.
 *                    face, the triangle moved by r along its unit normal to the side the origin is on:
 *                        n = e1 x e2,  nn = n.n,  h = n.w,  dn = n.d,  num = |h| - r*sqrt(nn),  den = (h >= 0 ? -dn : dn),
 *                        t = num/den,  q = w + t*d per component,  u = ((q x e2).n)/nn,  v = ((e1 x q).n)/nn;
 *                        conditions  num > 0 && den > 0 && t > 0 && u >= 0 && v >= 0 && u + v <= 1.
 *                    t = min(face, cyl(w, e1), cyl(w, e2), cyl(wb, e2 - e1), ball(w, d, dd, rr), ball(wb, d, dd, rr),
 *                    ball(wc, d, dd, rr)).  The union's first entry is the minimum over the pieces; the prism's side faces and the
 *                    cylinders' caps lie inside the edge and vertex pieces and need no test.  t = +inf: no contact.
 *                 3. Certification.  c = o + t*d per component (the product, then the sum); s = RT_SWEEP_SLACK * (max|c_i| + r);
 *                    accepted only if closest(c).t <= (r + s)*(r + s); (u, v) are that evaluation's.  A triangle whose smallest
 *                    root fails yields no contact; its later roots are not tried.
 *                 4. t <= tmax.
 *   sphere      a sphere of the scene is its surface, as in rt_tracer_overlap.  Centre C, radius R, w = o - C, ww = w.w,
 *               dist = sqrt(ww), s0 = |dist - R|:
 *                 start overlap when s0*s0 <= rr (t = 0);
 *                 else when dist > R: t = ball(w, d, dd, (R + r)*(R + r));
 *                 else when dist < R && r < R, the EXIT root against ri = R - r: b, l as in ball, disc = ri*ri - l.l,
 *                   sq = sqrt(dd*disc), t = (b > 0 ? (b + sq)/dd : (ri*ri - ww)/(sq - b)); conditions disc >= 0 && t > 0;
 *                 certified by c and s as above and  s1 = |sqrt((c - C).(c - C)) - R|,  s1*s1 <= (r + s)*(r + s);  then t <= tmax.
 *   winner      the accepted contact with the smallest (t, prim): equal t (==) goes to the lowest prim.  No visiting order is named.
 *   slack       RT_SWEEP_SLACK is part of the contract: a reported contact is never farther than s from touching (by the point
 *               query's own arithmetic at c); a graze within s may be reported as a miss.  It is the smallest power of two at least
 *               four times the largest residual measured (tests/test_spherecast_expect.py measures it again).
 * No scene: every answer is RT_PRIM_NONE; spheres alone can answer; n = 0 is a no-op; a NULL array with n > 0 is RT_ERR_INVALID.
 * Scheduling is that of the other queries: never cancels or joins a running Trace, serialised with the other calls, on the query
 * stream or the caller's, waited for by uploads and destroy; a multi-device handle answers from its first band, a band tracer
 * locally.
 * RT_QUERY_SCAN (default): every sweep tests every primitive.  RT_QUERY_BVH: the ray queries' tree (built, or under RT_ACCEL_REFIT
 * refitted, by the first query after an upload), walked nearest box first, bit for bit the scan's answer with NO conditioning
 * clause: an accepted contact is certified to lie within r + s of its record, so the line's span through a child's box grown by
 * r + 4*RT_SWEEP_SLACK*(cmax + r) + rho_s*(max|o| + cmax + r) contains its t, however ill conditioned the root was; a child is
 * skipped only when that span is empty, ends before t = 0 or begins STRICTLY after min(best t, tmax).  A sweep with a non-finite
 * component or a zero direction takes no pruning decision (rt_dbg_query_accel_slack scales the allowance beyond r).
 * That holds at the ends of fp32's range too, by a guard computed once per sweep: the box is grown by 2^-72 more than stated
 * (r*r, (r + s)^2 and the squared distances they are compared with round to multiples of 2^-149 below 2^-126, which can accept
 * a record up to 2^-74 beyond r + s), and a sweep with max|o| + (the largest |coordinate| of the tree) + r >= 2^62 takes no
 * pruning decision (there r*r or (r + s)^2 may be +inf, and inf <= inf accepts at any distance).
 * Range.  No absolute constant enters an answer: a scene and its sweeps multiplied by 2^k answer the same u, v and prim, and t
 * times 2^k when d is kept, the same t when d is multiplied too -- while the fourth powers of a length the roots and the point
 * arithmetic form (|e1 x e2|^2, a * disc, va, vb, vc) stay within fp32: for inputs of order 1, k = -31 .. 31 (-30 with d
 * multiplied).  Beyond, the face root is the first to go (n.n overflows or underflows: contacts with a face's interior are
 * reported by an edge or vertex root or not at all), then certification; scan and tree still agree bit for bit. */
/* Host arrays: sweeps n*8, hits n.  Returns with the answers in host memory. */
int  rt_tracer_sphere_cast(rt_tracer* t, const float* sweeps, size_t n, rt_hit* hits);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  sweeps and hits must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_sphere_cast_device(rt_tracer* t, const float* sweeps, size_t n, rt_hit* hits, void* stream);
#define RT_SWEEP_SLACK 0.00048828125f   /* 2^-11 */
/* (The swept queries stand behind the banner of the sharded frame and before its entry points: what lies between the region
 * queries' banner and that banner is the region queries' text alone, which tests/test_overlap_abi.py reads as one section.) */

/* ---- proximity of triangles ------------------------------------------------------------------------
 * How far is a TRIANGLE from the tracer's scene, and where (clearance and tolerance between parts, a collision margin before
 * contact, the nearest pair between a tool mesh and the scene, a one-sided mesh distance that cannot miss a minimum in the
 * interior of a face or an edge).  The triangle counterpart of rt_tracer_closest_point.
 *   tris        n x 12 floats: P0.x P0.y P0.z d2max P1.x P1.y P1.z _ P2.x P2.y P2.z _ (rt_tracer_overlap_triangles' layout; the
 *               first pad float carries the SQUARED search radius, +inf = unbounded, as the point query's fourth column does).
 *               The other two pad floats are never read into any arithmetic.  A query accepts NOTHING, spheres included, when any
 *               of its nine coordinates is non-finite or when d2max is a NaN or negative.
 *   hits        hits[i] = rt_hit exactly as rt_tracer_closest_point's: t = the squared distance, u, v = the barycentrics of the
 *               nearest point ON THE SCENE'S record (v0 + u*e1 + v*e2; 0, 0 for a sphere), prim.  No winner: {0, 0, 0,
 *               RT_PRIM_NONE}.
 *   witness     witness[i] = rt_witness {x, y, z, where}: the winning point ON THE QUERY triangle and the index k of the candidate
 *               below that produced it.  No winner: {0, 0, 0, -1}.
 *   arithmetic  one in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation, division and sqrt
 *               correctly rounded, dot products (x*x' + y*y') + z*z', cross products (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x,
 *               a.x*b.y - b.x*a.y), min and max IEEE minNum / maxNum, clamp(x) = min(max(x, 0), 1) (a NaN becomes 0).
 *               "closest(x) on (v0, e1, e2)" is the triangle rule of rt_tracer_closest_point, giving (t, u, v).
 *   per query   p1 = P1 - P0, p2 = P2 - P0, m = p1 x p2; the edges G_j -> G_j+1 of the corners (P0, P1), (P1, P2), (P2, P0) with
 *               d_j = G_j+1 - G_j (d_0 is p1) and a_j = d_j.d_j; qmin, qmax per axis as rt_tracer_overlap_triangles' step 1
 *               computes them; qabs = the largest |coordinate| of the three corners.
 *   triangle    on the record the renderer intersects (v0, e1, e2), A = v0, B = fl(v0 + e1), C = fl(v0 + e2), n = e1 x e2, the
 *               record's edges R_i -> R_i+1 of (A, B), (B, C), (C, A) with r_i = R_i+1 - R_i.  21 candidate points x_k on the query:
 *                 k = 0..2    the corners P0, P1, P2.
 *                 k = 3..5    proj(A), proj(B), proj(C), where proj(Y): (t', u', v') = closest(Y) on (P0, p1, p2), then
 *                             x = (P0 + u'*p1) + v'*p2 per component.
 *                 k = 6+3i+j  the point of query edge j nearest to record edge i (Ericson, closest points of two segments, with
 *                             the query edge as the first segment): w = G_j - R_i, a = a_j, e = r_i.r_i, f = r_i.w, c = d_j.w,
 *                             b = d_j.r_i, denom = a*e - b*b; s0 = clamp((b*f - c*e)/denom), but 0 when denom == 0;
 *                             tnom = b*s0 + f; s = clamp(-c/a) when tnom < 0 || e == 0, else clamp((b - c)/a) when tnom > e, else
 *                             s0; and s = 0 when a == 0.  x = G_j + s*d_j per component (the product, then the sum).
 *                 k = 15+j    where query edge j crosses the record's plane: da = n.(G_j - A), db = n.(G_j+1 - A); PRESENT only when
 *                             da*db <= 0 && da != db; s = clamp(da/(da - db)), x = G_j + s*d_j.
 *                 k = 18+i    where record edge i crosses the query's plane: da = m.(R_i - P0), db = m.(R_i+1 - P0), present as
 *                             above, Y = R_i + s*r_i, x = proj(Y).
 *               A candidate that is absent or has a NaN coordinate is not considered.  Then every x_k is clamped per axis into
 *               [qmin, qmax] (max with qmin, then min with qmax: exact; a query collapsed to a point makes every candidate that
 *               point).  t_k, u_k, v_k = closest(x_k) on the record.  The pair's answer is the smallest t_k (a NaN t_k never), equal
 *               t going to the lowest k, with that evaluation's (u, v); no candidate left: no answer.
 *   sphere      a sphere of the scene is its surface; prim = n_tris + i.  Centre S, radius r.  Four candidates: where = 0..2 the
 *               corners, where = 3 proj(S), considered and clamped as above; t_k = s*s with s = |sqrt(w.w) - r|, w = x_k - S (the
 *               point query's sphere rule); the smallest, equal t to the lowest k.  When rt_tracer_overlap_triangles' sphere
 *               condition holds (d2min <= r*r && r*r <= d2max in its arithmetic), t = 0 at that same candidate.  u = v = 0.
 *   winner      a pair is accepted when t <= d2max (plain fp32; a NaN never).  The winner is the accepted pair with the smallest
 *               (t, prim): equal t (==) goes to the lowest prim.  No visiting order is named.
 *   what it means
 *               (t, u, v) is, bit for bit, closest(witness.xyz) on record prim: the answer can be checked with
 *               rt_tracer_closest_point, and t is an upper bound of the true squared distance up to the point query's rounding -- a
 *               reported pair is really that close.  From below it is as accurate as measured (DESIGN.md 4.3m;
 *               tests/test_tridistance_expect.py): with scale = qabs + the largest |vertex coordinate| and eps = 2^-24,
 *               sqrt(t) >= D - K*eps*scale for every pair and |sqrt(t) - D| <= K*eps*scale where both triangles are well shaped
 *               (smallest corner-angle sine >= 2^-6), K = 8 (measured 1.98), D the float64 distance of the fp32 corners.
 *               t == 0 is guaranteed where a query corner is bit-equal to a record's v0, not for every intersecting pair:
 *               rt_tracer_overlap_triangles is the touching verdict.
 * No scene, spheres alone, n = 0, NULL arrays (RT_ERR_INVALID, outputs untouched), scheduling, multi-device handles and
 * RT_ACCEL_REFIT are rt_tracer_closest_point's.
 * RT_QUERY_BVH: the ray queries' tree, walked nearest box first.  Per child box [lo, hi] with cmax its largest |coordinate|:
 *     pad = rho_c * (qabs + cmax);  g = max(max(lo - qmax, qmin - hi, 0) - pad, 0) per axis;
 *     lb = ((gx*gx + gy*gy) + gz*gz) * (1 - 2^-21)
 * with rho_c the point query's.  A child is skipped only when lb > best STRICTLY, at the visit and again when it is taken from the
 * stack; best starts at d2max; a NaN lb takes no pruning decision.  The always-tested list and the spheres follow the walk; a walk
 * whose stack overflowed recomputes from every leaf record.  The answer is bit for bit the scan's two arrays under the point
 * query's own invariant (its sliver premise included): every x_k lies in [qmin, qmax], and for every x there each
 * term above is, by the monotonicity of fp32 subtraction, multiplication and max, at most the term the point query computes for
 * x -- so lb is at most the point query's bound, which every record inside the child answers with a t at least as large.
 * Range: the point query's fourth powers (closest_triangle, and a * e - b * b of the segment pairs): a scene and its query
 * triangles multiplied by 2^k answer the same u, v, prim and `where`, t times 2^2k and the witness times 2^k, for k = -31 .. 31
 * on inputs of order 1; beyond, interior and crossing candidates answer NaN first.  Scan and tree agree at every scale. */
typedef struct rt_witness { float x, y, z; int32_t where; } rt_witness;
/* Host arrays: tris n*12, hits n, witness n.  Returns with the answers in host memory. */
int  rt_tracer_triangle_distance(rt_tracer* t, const float* tris, size_t n, rt_hit* hits, rt_witness* witness);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  tris, hits and witness must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_triangle_distance_device(rt_tracer* t, const float* tris, size_t n, rt_hit* hits, rt_witness* witness, void* stream);

/* ---- section queries ------------------------------------------------------------------------------
 * The region query for a plane or a slab, and where the plane cuts what it returned.  Both follow the conventions of the region
 * queries (rt_tracer_overlap): host and _device forms, the cursor, scheduling -- a query never cancels or joins a running Trace --
 * and a multi-device handle answers from its first band. */
/* Which primitives of the tracer's scene a PLANE or a SLAB cuts (a cross-section, a contour slice, clipping by a half-space, the
 * layer between two heights): the region d0 <= n.x <= d1, a plane when d0 == d1, a half-space when one end is infinite.
 *   planes      n x 8 floats: nx ny nz d0 d1 _ _ _ (two 16-byte loads).  The three pad floats are never read into any arithmetic:
 *               NaNs there change nothing.  n is used as given, NOT normalised.  The query is valid when nx, ny, nz are finite
 *               and d0 <= d1 as a plain comparison (-inf and +inf ends are allowed); any other query -- a NaN anywhere among
 *               the five, an infinite normal component, d0 > d1 -- accepts NOTHING, spheres included.  n = 0 is not special: it
 *               gets what the arithmetic gives (every projection is 0, so everything is accepted when d0 <= 0 <= d1).
 *   max_hits, after, prims, counts
 *               exactly as in rt_tracer_overlap: max_hits 0 .. RT_MAX_HITS (above that RT_ERR_INVALID; 0: counts only, prims
 *               may be NULL); row i holds the min(counts[i], max_hits) LOWEST accepted prims in ascending order, then
 *               RT_PRIM_NONE; counts[i] is the TOTAL behind the cursor, not capped; after[i] = the row's last prim continues:
 *               nothing repeats and nothing is lost.
 *   triangle    one arithmetic in RT_MATH_FMA and RT_MATH_STRICT: every operation is one separately rounded fp32 operation; min
 *               and max are IEEE minNum / maxNum.  On the record the renderer intersects (v0, e1, e2; for edge-format scenes the
 *               uploaded rows), with corners A = v0, B = fl(v0 + e1), C = fl(v0 + e2), and
 *                 p(X) = (nx*X.x + ny*X.y) + nz*X.z
 *               the triangle is accepted when the query is valid, none of p(A), p(B), p(C) is a NaN,
 *                 min(min(p(A), p(B)), p(C)) <= d1  and  max(max(p(A), p(B)), p(C)) >= d0.
 *               Plain comparisons, closed: touching counts.  There is no second step: a triangle meets a slab exactly when its
 *               corners' projections meet the interval.
 *   sphere      a sphere of the scene is its surface.  Centre S, radius r:  pc = p(S), rn = r * sqrt((nx*nx + ny*ny) + nz*nz), the
 *               square root correctly rounded.  Accepted when the query is valid, pc - rn <= d1 and pc + rn >= d0.  A slab is
 *               unbounded, so the ball touches it exactly when the surface does.
 * Everything else -- no scene, spheres alone, n = 0, NULL arrays (RT_ERR_INVALID, outputs untouched), scheduling, multi-device
 * handles, RT_ACCEL_REFIT -- is rt_tracer_overlap's.
 * RT_QUERY_BVH: for a child box [lo, hi] take per axis xlo = (n_axis >= 0 ? lo : hi) and xhi the other end, and pmin = p(xlo),
 * pmax = p(xhi) by the same expression.  The child is skipped only when pmin > d1 or pmax < d0 (a NaN never skips); there is NO
 * inflation, and the result is bit for bit the scan's rows and counts for every input whatsoever.  Why: rounding is monotone --
 * x -> fl(n_axis * x) is monotone in the direction of n_axis's sign, fl(a + b) is monotone in both operands, and flushing
 * denormals keeps both -- so for every fp32 point P with lo <= P <= hi componentwise pmin <= p(P) <= pmax whenever no value is
 * a NaN; A, B and C lie inside the record's tree box (rt_tracer_overlap, above) and inside every ancestor's child box, so a
 * skipped child holds only records the rule rejects.  Non-finite records go through the always-tested list, and a walk whose
 * stack overflowed recomputes from every leaf record.  rt_dbg_query_accel_slack has no effect on this query.
 * Range.  Only second powers enter (a product of a normal component and a coordinate, the sphere rule's dot(n, n)): the rows of
 * a scene and its planes multiplied by 2^k -- every length and the normal times s, d0 and d1 times s*s -- are the same rows for
 * k = -61 .. 62 on inputs of order 1 (tests/test_section_range.py); beyond, the products reach +inf or the subnormals.  Scan and
 * tree agree at every scale. */
/* Host arrays: planes n*8, after n or NULL, prims n*max_hits (NULL allowed when max_hits = 0), counts n.  Returns with the
 * results in host memory. */
int  rt_tracer_section(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                       uint32_t* counts);
/* Device pointers on the tracer's device: only enqueues on `stream` (a hipStream_t; NULL is HIP's default stream), no host
 * synchronisation.  planes must be 16-byte aligned; otherwise RT_ERR_INVALID. */
int  rt_tracer_section_device(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                              uint32_t* counts, void* stream);
/* WHERE the plane n.x = d0 (side = 0) or n.x = d1 (side = 1) cuts the primitives rt_tracer_section returned: a post-pass over its
 * rows, one record per prim.
 *   planes      the n planes of the section query, as above.
 *   prims       n * per_plane int32, record j belongs to plane j / per_plane: a row of rt_tracer_section with max_hits =
 *               per_plane, or any prims of the caller's.  per_plane 1 .. RT_MAX_HITS and side 0 or 1; otherwise RT_ERR_INVALID.
 *   cuts        n * per_plane rt_cut.  One arithmetic in both math modes, every operation rounded separately, the division and
 *               the square roots correctly rounded.  With d the chosen offset and sX = p(X) - d for X = A, B, C (the sign of an
 *               fp32 difference is exact) a corner is above (s > 0), below (s < 0) or on the plane (s == 0).
 *     RT_CUT_NONE      the prim is RT_PRIM_NONE or outside the scene (nothing is read), the plane is invalid, some s is a NaN, or
 *                      all corners are strictly on one side.  The record is all zeros.
 *     RT_CUT_COPLANAR  all three corners are on the plane.  The points are zero.
 *     RT_CUT_TOUCH     no corner is above, or none is below, and one or two corners are on the plane.  p0, p1 are the on-corners,
 *                      bit for bit; one on-corner: both points are that corner; two: in the order of the walk A -> B -> C -> A
 *                      (A, B), (B, C) or (C, A).
 *     RT_CUT_SEGMENT   at least one corner above and one below.  The endpoints are the on-corner (bit for bit), if there is one,
 *                      and the crossings of the edges whose ends are strictly opposite.  A crossing is always computed from the
 *                      below end L towards the above end U:  t = sL / (sL - sU),  X = L + t*(U - L) per component (a
 *                      subtraction, a product, a sum).  Two records that share an edge with bit-equal corners therefore give
 *                      bit-equal points, whichever way each one walks the edge.  p0 is where the walk A -> B -> C -> A leaves the
 *                      above side, p1 where it enters it: the segment p0 -> p1 runs along n x (e1 x e2), so the contour of an
 *                      outward-wound solid runs counter-clockwise seen from the tip of n, holes clockwise.
 *     features         f0 | f1 << 8, f0 of p0 and f1 of p1: 0 / 1 / 2 the edge AB / BC / CA, 4 / 5 / 6 the corner A / B / C.  A
 *                      caller with adjacency can chain contours without comparing floats.  0 for NONE, COPLANAR and CIRCLE.
 *     RT_CUT_CIRCLE    a sphere (centre S, radius r) with |pc - d| <= rn, pc and rn as in the section rule, nn = dot(n, n):
 *                      p0 = S + ((d - pc) / nn) * n, the circle's centre; p1 = {sqrt(max(r*r - ((d - pc)*(d - pc)) / nn, 0)), 0, 0},
 *                      its radius.  Otherwise RT_CUT_NONE.
 * No tree is walked and no scene is needed (every record is then RT_CUT_NONE); n = 0 is a no-op; a NULL array with n > 0 is
 * RT_ERR_INVALID.  Chaining segments into polylines with a tolerance, capping cut solids and regions bounded by several planes
 * are not offered: corners of neighbouring records need not be bit-equal in general, because B = fl(v0 + e1). */
#define RT_CUT_NONE     0
#define RT_CUT_SEGMENT  1
#define RT_CUT_TOUCH    2
#define RT_CUT_COPLANAR 3
#define RT_CUT_CIRCLE   4
typedef struct rt_cut { float p0[3]; int32_t kind; float p1[3]; int32_t features; } rt_cut;   /* 32 bytes */
/* Host arrays: planes n*8, prims n*per_plane, cuts n*per_plane. */
int  rt_tracer_section_segments(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane, uint32_t side,
                                rt_cut* cuts);
/* Device pointers on the tracer's device: only enqueues on `stream`.  planes and cuts must be 16-byte aligned; otherwise
 * RT_ERR_INVALID. */
int  rt_tracer_section_segments_device(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane,
                                       uint32_t side, rt_cut* cuts, void* stream);

/* ---- one frame sharded over several GPUs, continued: the entry points --------------------------- */
/* Same constructor, device list added: band k runs on devices[k] (ordinals may repeat: several bands per
 * device).  The handle is an rt_tracer like any other -- Trace / Stop / Resize / SetCameraParameters /
 * RotateCamera / UploadScene / callbacks keep their meaning, the callbacks receive the WHOLE frame (pinned
 * host memory) once per update, from one render thread, as in RayTracerImpl.cu:256-305; every device gets
 * its own host thread for the launches.  rt_tracer_read_buffer returns whole-frame buffers (RT_BUF_IMAGE =
 * the gathered frame), rt_tracer_trace_enqueue / rt_tracer_launch* include the gather,
 * rt_tracer_kernel_time reports the first band.  options->device / full_height / row_begin are not used
 * (full_height must be 0); results are bit-identical to a single tracer on the whole frame. */
int  rt_tracer_create_multi(const uint32_t imageSize[2], const float cameraPosition[3],
                            const float cameraAngles[2], float fov, float focalLength, float aperture,
                            const rt_options* options, const int32_t* devices, uint32_t n_bands,
                            rt_tracer** out);
/* One process per GPU instead (torch.distributed.run, MPI ...): every rank creates the tracer of ITS band
 * (rt_options.full_height / row_begin, rows of rank r of n = [r*H/n, (r+1)*H/n)) and joins the group with the
 * id rank 0 made and the launcher's own rendezvous distributed (collective: every rank calls it).  From then
 * on an emitting rt_tracer_trace_enqueue / rt_tracer_launch* of a member is followed by the gather of its
 * tile to rank 0, on a stream of its own, ordered by events; rt_tracer_sync waits for it as well, and rank 0
 * reads the gathered frame as RT_BUF_FRAME.  n_ranks == 1 needs no id. */
int  rt_group_unique_id(uint8_t id[RT_GROUP_ID_BYTES]);
int  rt_tracer_join_group(rt_tracer* t, uint32_t n_ranks, uint32_t rank, const uint8_t id[RT_GROUP_ID_BYTES]);
int  rt_tracer_leave_group(rt_tracer* t);
/* The same with an explicit partition: row_begin[0..n_ranks] ascending, row_begin[0] = 0, row_begin[n_ranks] =
 * full_height; rank r owns the rows [row_begin[r], row_begin[r+1]) (its tracer must have been created on, or
 * moved to -- rt_tracer_set_band -- exactly those rows). */
int  rt_tracer_join_group_bands(rt_tracer* t, uint32_t n_ranks, uint32_t rank, const uint8_t id[RT_GROUP_ID_BYTES],
                                const uint32_t* row_begin);
/* Load balance.  The reference scans every triangle for every ray, so equal rows are equal work there; with the
 * per-tile classification a band costs what its tiles' candidate lists cost, and equal rows leave the bands of a dense
 * scene uneven (C5 in 8 bands: mean/max = 0.83).  rt_balance_rows: from each band's measured cost, boundaries (multiples
 * of `granule` rows; the kernel's tiles are 8 rows high) that equalise it, assuming the cost is spread evenly inside a
 * band.  rt_tracer_rebalance applies it to a multi-device tracer from its bands' own kernel times since the last
 * rt_tracer_kernel_time reset; rt_tracer_set_band moves a band tracer of a multi-process job.  Like Resize, both
 * re-create the buffers and the RNG states of the bands (RayTracerImpl.cu:94-103); the image a Trace produces does not
 * depend on the partition. */
int  rt_balance_rows(uint32_t n_bands, const uint32_t* row_begin, const double* cost, uint32_t granule,
                     uint32_t* new_row_begin);
int  rt_tracer_rebalance(rt_tracer* t);
int  rt_tracer_set_band(rt_tracer* t, uint32_t row_begin, uint32_t rows);
/* Device time of the gathers since the last reset (root only; HIP events on the root's gather stream around
 * the exchange) and their number.  Zero for a frame whose bands all live on the root device. */
int  rt_tracer_gather_time(rt_tracer* t, double* total_ms, uint64_t* gathers, int reset_after);
/* One more exchange of the tiles as they are, without tracing: what the gather costs on its own (read it with
 * rt_tracer_gather_time).  A multi-device tracer or a group member (collective: every rank calls it). */
int  rt_tracer_gather_only(rt_tracer* t);
/* What the group is made of, as JSON text: transport ("rccl" | "peer" | "local" | "none"), ranks, the band -> rank map, the local
 * devices, and for an RCCL transport the library's version and per communicator its rank, ncclCommCount and device. */
int  rt_tracer_group_info(rt_tracer* t, char* json, size_t capacity);
/* Bands of the handle (1 for a plain tracer) and where band k runs: out = {device, first row, rows, rank}. */
int  rt_tracer_band_count(rt_tracer* t);
int  rt_tracer_band_info(rt_tracer* t, uint32_t band, uint32_t out[4]);

/* ---- single-function device harnesses (parity tests) ---------------------------------- */
/* n independent (ray, triangle) pairs through the device HitTriangle: rays n*6 (origin,
 * un-normalised direction -> rt::Ray(o, d, true)), tris n*9 (a, b, c).  eps_mode 0 =
 * kernel epsilon 1e-10f, 1 = unit-test epsilon FLT_EPSILON.  Outputs: hit n, tuv n*3,
 * normal n*3 = normalize(cross(b-a, c-a)), point n*3 = ray.point(t). */
int rt_dbg_hit_triangle(int device, uint32_t math_mode, uint32_t n, const float* rays,
                        const float* tris, int eps_mode, int32_t* hit, float* tuv, float* normal,
                        float* point);
int rt_dbg_sincos(int device, uint32_t n, const float* x, float* s, float* c);
/* 256-thread blocks of the default trace kernel (K = samples_in_flight) the occupancy API admits
 * per CU with lds_bytes of dynamic LDS (measurement aid). */
int rt_dbg_trace_occupancy(int device, int samples_in_flight, uint32_t lds_bytes);
/* fp32 VALU calibration on this device: attainable lane-FMA/s (8 fma chains per lane,
 * 8 waves per SIMD, every CU) and the shader clock held meanwhile.  Measurement aid only. */
int rt_dbg_valu_peak(int device, double* lane_fma_per_s, double* clock_ghz);
/* Exhaustive device check of the mid-range sqrt / reciprocal fast paths used by normalize: every float in
 * [2^-96, 2^96] against the generic correctly rounded expansions.  out = {values checked, sqrt mismatches,
 * reciprocal mismatches, bit pattern of a mismatching operand or 0}. */
int rt_dbg_check_midrange(int device, uint64_t out[4]);
/* Dense scenes: the header words (candidate count; 0xFFFFFFFF = the list overflowed its capacity and the tile tests its macro
 * tile's list) of the per-wave lists in HBM as the last launch left them; half 0 = an unsplit launch or the upper half of a split
 * one, 1 = the lower half.  Measurement aid and tests. */
int rt_dbg_wave_list_counts(rt_tracer* t, int half, uint32_t* dst, size_t capacity_tiles, uint32_t* n_tiles, uint32_t* capacity_per_tile);
/* The stored tile candidate lists of a small-scene tracer (after a launch that stored them): per 8x8 wave tile, in grid
 * order (4 per 32x8 block), *words_per_tile words: count | winner << 10 | certain-winner << 31, then the triangle indices. */
int rt_dbg_read_tile_lists(rt_tracer* t, uint32_t* dst, size_t capacity_words, uint32_t* words_per_tile);
/* The focal box each 8x8 wave tile of a trace launch classifies with (full tiles: the four corner pixels' focal points
 * widened by a curvature term; partial tiles: every in-image lane) and the focal points of the band's pixels as the rays
 * use them.  boxes: 8 floats per tile in grid order (4 per 32x8 block): lo[3], hi[3], corner path taken, usable;
 * focal: 3 floats per pixel.  curv_scale multiplies the curvature term for THIS launch only (1 = product; the test's
 * teeth: with 0 some pixel's focal point must fall outside its box). */
int rt_dbg_focal_boxes(rt_tracer* t, float curv_scale, float* boxes, size_t boxes_capacity, float* focal, size_t focal_capacity);
/* The conservative classification verdict by verdict (tests/test_gpu_classification.py, CLASSIFICATION.md): for each of
 * n_regions regions of the band -- level 0: the 8x8 wave tile at pixel (regions[2i], regions[2i+1]) (x a multiple of 8, band-local
 * row a multiple of 8), bounded exactly as a trace wave bounds it; level 1: the 32x8 block (x a multiple of 32), the union of
 * its four wave tiles; level 2: the 128x64 macro tile; level 3: the 32x16 region of the small scenes' two-level list builder
 * (x a multiple of 32, row a multiple of 16), the union of its eight tiles' boxes -- and for EVERY triangle of the scene, what tile_misses_triangle decides
 * and the interval ends it decides from, with every rounding allowance multiplied by slack_milli / 1000 (1000 = the product;
 * 300, 100, 30, 10, 0 exist so that the margin can be measured in the shipped library).
 *   out[region] = 16 floats: focal box lo[3], hi[3], lmin, lmax of |F - o|, usable (1) + 2 when the focal bounds of the list
 *   builder and of a large-scene trace wave (focal_bounds) agree bit for bit, + 4 when the host vouches for the corner bound (the
 *   two-level list builder is in use; level 3 is meaningless otherwise), lens radius A, orad[3], fc[3], followed by
 *   n_tris records.  forms == 0 (small-scene instantiation), 12 floats: flags (1 = kept, 2 = certainly hit by every ray of the
 *   family), det_lo, det_hi, U_lo, U_hi, V_lo, V_hi (bounds of det', U', V' = the reference's det, U = dot(tv, pv), V = dot(dir, qv)
 *   of Kernels.cuh:40,50,57 times |F - o|), q_lo, q_hi (bounds of t / |F - o|, t of Kernels.cuh:63), S_lo, S_hi (bounds of det' - U' - V'), 0.
 *   forms != 0 (large-scene instantiation with the per-sample forms), 32 floats: flags (1 = kept), the six ends, S_lo, S_hi, 3 x 0, then the
 *   forms {F1.c0, cx, cy, F2..., F3..., g1.xyz, g2.xyz, g3.xyz} each form scaled by its power of two, the gradients the fp16 values the kernel stores, 2 x 0. */
int rt_dbg_classify(rt_tracer* t, uint32_t level, uint32_t forms, uint32_t slack_milli, const uint32_t* regions, uint32_t n_regions,
                    float* out, size_t capacity_floats);
/* The BVH builder of RT_QUERY_BVH on its own; needs no device.  rows: count float4 as rt_tracer_upload_scene takes them, or
 * (edges_layout != 0) as rt_tracer_upload_scene_edges does.  Writes the node array and the record array exactly as a tracer
 * uploads them; info = {depth bound the traversal stack is sized from, 1, nodes, leaves, max depth, always-tested, build us,
 * bytes}.  With both capacities 0 only info is written (nodes * 128 and count / 3 * 48 bytes are needed).
 *   node, 128 bytes:   float lo_x[4], lo_y[4], lo_z[4], hi_x[4], hi_y[4], hi_z[4] (the four children's boxes); uint32 child[4];
 *                      float cmax[4] (largest |coordinate| of the child's box).  child: 0xFFFFFFFF = none (lo = +inf, hi = -inf);
 *                      bit 31 set = leaf, bits 28-29 = triangles - 1 (1..4), bits 0-27 = its first record; else a node index.
 *                      Node 0 is the root; no node at all when no triangle is finite.
 *   record, 48 bytes:  float e2[3], e1[3], v0[3]; uint32 upload index; 2 x uint32 0.  The leaves' records come first (a leaf's
 *                      ascending by upload index), then the always-tested list: the triangles with a non-finite record, which
 *                      are in no box and which every ray tests. */
int rt_dbg_bvh_build(const rt_float4* rows, size_t count, int edges_layout, void* nodes, size_t node_capacity_bytes,
                     void* leaf_records, size_t leaf_capacity_bytes, uint64_t info[8]);
/* The feature table of the signed point queries on its own; needs no device.  rows as rt_dbg_bvh_build takes them.  Writes
 * count / 3 * 7 float4 (112 bytes per triangle) exactly as a tracer uploads them; info = {triangles, welded vertices, undirected
 * edges, contributing triangles, build us, bytes, 0, 0}.  With capacity_bytes 0 only info is written. */
int rt_dbg_feature_normals(const rt_float4* rows, size_t count, int edges_layout, void* out, size_t capacity_bytes, uint64_t info[8]);
/* The rays of rt_tracer_exposure on their own: segs_out receives the n * n_dirs segments {origin, d_ij, tmin_i, tmax_i} (8 floats
 * each, point-major: segment i * n_dirs + j) that the query traces for these arguments, from the function its kernels call.  With
 * a tracer a device kernel evaluates it (on the tracer's device, scheduled as a query; n * n_dirs < 2^31); with t == NULL the
 * host does and no device is needed.  Host arrays; n_dirs and flags as rt_tracer_exposure checks them; n = 0 is a no-op. */
int rt_dbg_exposure_rays(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags,
                         float* segs_out);
/* rtb::refit on its own, the reference of the device refit; needs no device.  nodes (node_bytes = nodes * 128), leaf_records
 * (record_bytes = count / 3 * 48) and info are arrays rt_dbg_bvh_build (or this call) wrote for a scene of as many triangles; rows
 * are the new scene.  In place: the records take the new triangles by upload index, every box and cmax is recomputed, child[] and
 * info stay.  RT_ERR_STATE when the partition rule fails (nothing is written); RT_ERR_INVALID for arrays that are no such tree. */
int rt_dbg_bvh_refit(const rt_float4* rows, size_t count, int edges_layout, void* nodes, size_t node_bytes, void* leaf_records,
                     size_t record_bytes, uint64_t info[8]);
/* rtb::tree_cost of a node array in rt_dbg_bvh_build's layout: the cost rt_tracer_query_accel_update_info reports, computed on
 * the host.  0 for no nodes (or a NULL array). */
double rt_dbg_bvh_tree_cost(const void* nodes, size_t node_bytes);
/* The tracer's current device tree as the queries walk it, in rt_dbg_bvh_build's layouts and with its info.  With both
 * capacities 0 only info is written.  RT_ERR_STATE while no valid tree exists. */
int rt_dbg_query_tree_read(rt_tracer* t, void* nodes, size_t node_capacity_bytes, void* records, size_t record_capacity_bytes,
                           uint64_t info[8]);
/* Multiplies the box test's inflation rho for this tracer's following queries in RT_QUERY_BVH mode (1000 = the product; 300,
 * 100, 30, 10, 0 exist so that the margin can be measured in the shipped library, tools/bvh_margin.py). */
int rt_dbg_query_accel_slack(rt_tracer* t, uint32_t slack_milli);
/* Test-only: an upper limit on the entries per lane of the traversal stack of this tracer's following queries in RT_QUERY_BVH
 * mode.  The walks run with min(3 x the tree's depth, cap) entries; UINT32_MAX (the default) is the product.  The limit can
 * only lower the capacity -- the stack's LDS is sized from the lowered number, and 0 launches without any -- so that a lane
 * whose walk wants one entry more takes the kernels' overflow path: its answer is recomputed from every leaf record and obeys
 * the same contract.  It exists so that the tests can run that path, which a tree of the builder never takes on its own. */
int rt_dbg_query_stack_cap(rt_tracer* t, uint32_t cap);
/* states n*6 {d,v0..v4} advanced in place, out n*m uniforms in (0,1] */
int rt_dbg_uniform(int device, uint32_t n, uint32_t m, uint32_t* states, float* out);
/* thin-lens rays of the tracer's current camera for n (x, y) pixels with given RNG states */
int rt_dbg_get_ray(rt_tracer* t, uint32_t n, const uint32_t* pixels, uint32_t* states, float* rays);
/* host: curand_init(seed, subsequence, 0) restated -> state[6] */
void rt_dbg_rng_init_host(uint64_t seed, uint64_t subsequence, uint32_t state[6]);
/* host: the xorshift words v0..v4 advanced in place by n draws -- through the window table of T^n (use_table != 0: the
 * product the settle kernel forms) or by n single steps */
void rt_dbg_rng_advance_host(uint32_t state[5], uint32_t n, int use_table);
/* the same for count states of 5 words each, the table built once */
void rt_dbg_rng_advance_host_n(uint32_t* states, uint32_t count, uint32_t n, int use_table);
/* the draws a plain tracer owes to its certain-winner tiles: out = {owed draws, owing launches since the last settle,
 * settle kernels enqueued so far, device tables held} */
int rt_dbg_owed_state(rt_tracer* t, uint64_t out[4]);
/* the runtime calls the enqueue path of a plain tracer's trace launches has issued since the last call (reading clears them):
 * out = {trace launches (steps) enqueued, kernel launches, event records, stream waits, list_ready events recorded as a call of
 * their own, list_free events recorded as a call of their own, events a kernel launch carried as its stop event instead, 0} */
int rt_dbg_enqueue_calls(rt_tracer* t, uint64_t out[8]);
/* the tile-list builds of a plain tracer's small scenes (up to 256 triangles) since it was created, by the builder kernel that
 * ran: out = {region pairs (<= 32 triangles, corner-bounded tiles), regions (33..256, corner-bounded tiles), one-level tiles
 * (<= 32), one-level tiles (33..256)}.  Which one runs depends on the scene's size and on the frame's height and lens
 * ("The small-scene kernels' options, tested"); reading clears nothing */
int rt_dbg_list_builds(rt_tracer* t, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
