// rt_query_api.hpp -- the query entry points of include/rt_mi355x.h.  Included by rt_tracer.hip.
//
// Every query that takes arrays has a host form and a _device form, and both are one call of run_query with the query's
// description: where the call runs (QueryWhere), its input and output arrays (QueryIn, QueryOut: pointer, bytes, the alignment
// the _device form demands, whether it may be null), the _device form's alignment message, the query's own argument check,
// what it prepares (the signed queries' feature table) and what it enqueues on device pointers.  run_query is the path: the
// checks in one order, all before the lock; query_entry (api_mu, a sharded handle forwarded to its first band); the rest under
// guarded() -- n = 0 returns, the device made current, the preparation, for the host form the caller's arrays staged through
// QueryState::in / ::out in the order of the description, the enqueue, and for the host form the copies back and the one wait.
// rt_tracer_pick, which checks its pixels under the lock, uses the same checks and the same body (query_body).
//
// A query is not an exclusive() entry point: it never cancels or joins a running Trace.  It is serialised with the other API
// calls by api_mu, reads only the scene and a snapshot of the camera (params(), under state_mu), and runs on a stream of its
// own (QueryState::stream_q, created by the first query) or on the caller's.  QueryState::done, recorded behind every query, is what the scene
// uploads and destroy wait for before they touch the records a query may still read: every launch goes through enqueue_launch,
// the one place that waits for and records it.  The entry points that take no arrays are query_call (or, with a check of their
// own, query_entry).
#pragma once
#include <cmath>
#include <initializer_list>

#include "rt_bvh_host.hpp"
#include "rt_features_host.hpp"

namespace rtr {

constexpr size_t kQueryMaxRays = 0xFFFFFFFFu;

// K rays per lane: 4 once a batch fills the GPU's resident blocks at K = 4 (256 CUs x 4 blocks of 256 lanes), 2 once it
// does so at K = 2, else 1 -- a pick of one pixel is one block with K = 1.  rt_options.samples_in_flight forces it.
inline int query_k(const rt_tracer* t, size_t n) {
  if (t->k_req == 1 || t->k_req == 2 || t->k_req == 4) return static_cast<int>(t->k_req);
  constexpr size_t kResidentLanes = 256u * 4u * 256u;
  return n >= 4u * kResidentLanes ? 4 : n >= 2u * kResidentLanes ? 2 : 1;
}

// Where a query call runs.  The host form takes host arrays, stages them on the query stream and waits for it; the _device
// form takes device pointers and enqueues on the caller's stream, of which null is a legitimate one: hence the tag.
struct QueryWhere { bool device; hipStream_t stream; };
inline QueryWhere on_host() { return {false, nullptr}; }
inline QueryWhere on_device(void* stream) { return {true, static_cast<hipStream_t>(stream)}; }

// One array of a query call: the caller's pointer, its bytes (0: nothing to stage), the alignment its kernel's loads and stores
// need of a _device form's pointer, and whether the caller may pass null.  A call has at most two of each direction.
template <class Void>
struct QueryArray { Void* p; size_t bytes; uintptr_t align; bool optional = false; };
using QueryIn = QueryArray<const void>;
using QueryOut = QueryArray<void>;
using QueryIns = std::initializer_list<QueryIn>;
using QueryOuts = std::initializer_list<QueryOut>;

// The argument checks, made before the lock.  A batch of n != 0 needs its arrays and a count the kernels' 32-bit indices hold.
inline bool query_args_ok(rt_tracer* t, size_t n, bool arrays_present) {
  if (n == 0u) return true;
  if (!arrays_present) { t->set_error("query: null array"); return false; }
  if (n > kQueryMaxRays) { t->set_error(fmt("query: %zu rays (at most %zu)", n, kQueryMaxRays)); return false; }
  return true;
}

// ... of a described call: every array that is not optional, and for a _device form every pointer on its alignment (null is on
// any), else `misaligned`, the entry point's own sentence
inline bool query_arrays_ok(rt_tracer* t, QueryWhere w, size_t n, QueryIns in, QueryOuts out, const char* misaligned) {
  bool present = true, aligned = true;
  const auto look = [&](const void* p, uintptr_t align, bool optional) {
    present = present && (p || optional);
    aligned = aligned && reinterpret_cast<uintptr_t>(p) % align == 0u;
  };
  for (const QueryIn& a : in) look(a.p, a.align, a.optional);
  for (const QueryOut& a : out) look(a.p, a.align, a.optional);
  if (!query_args_ok(t, n, present)) return false;
  if (n != 0u && w.device && !aligned) { t->set_error(misaligned); return false; }
  return true;
}

// records per ray or point (`what`: max_hits, per_point), checked whatever n is
inline bool query_row_ok(rt_tracer* t, const char* who, const char* what, uint32_t k) {
  if (k != 0u && k <= RT_MAX_HITS) return true;
  t->set_error(fmt("%s: %s = %u (1 to %u)", who, what, k, RT_MAX_HITS));
  return false;
}
inline bool no_check(rt_tracer*) { return true; }

// An entry point on a non-null handle: its API calls serialised, a sharded handle answered by its first band (whose error text
// becomes the handle's), any other by rest().
template <class Forward, class Rest>
int query_entry(rt_tracer* t, Forward&& forward, Rest&& rest) {
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (!t->mg) return rest();
  rt_tracer* band = t->mg->bands[0];
  const int rc = forward(band);
  if (rc != RT_OK) t->set_error(band->last_error);
  return rc;
}

template <class Forward, class Body>
int query_call(rt_tracer* t, Forward&& forward, Body&& body) {
  return query_entry(t, forward, [&] { return guarded(t, body); });
}

// The host-array entry points' staging buffers (QueryState::in, ::out), grow-only: n elements of T of the caller's array into
// d on `st`, room for n results in d, n results out of d into the caller's array on `st`.
template <class T>
T* room(DevArray<unsigned char>& d, size_t n) {
  d.ensure(n * sizeof(T));
  return reinterpret_cast<T*>(d.get());
}
template <class T>
T* staged_in(DevArray<unsigned char>& d, const void* src, size_t n, hipStream_t st) {
  HIP_CHECK(hipMemcpyAsync(room<T>(d, n), src, n * sizeof(T), hipMemcpyHostToDevice, st));
  return reinterpret_cast<T*>(d.get());
}
template <class T>
void staged_out(void* dst, const DevArray<unsigned char>& d, size_t n, hipStream_t st) {
  HIP_CHECK(hipMemcpyAsync(dst, d.get(), n * sizeof(T), hipMemcpyDeviceToHost, st));
}
// what a host-array entry point starts with: the tracer's device current, the query stream made
inline hipStream_t host_query_stream(rt_tracer* t) { t->use_device(); return t->queries.stream(); }

// What a described call does under the lock once its arguments are in order.  enqueue(t, in, out, st) gets the device pointers
// of the arrays in the description's order -- the caller's own in the _device form, the staging buffers of the same index in the
// host form, null for an array that was left out or has no bytes -- and issues the launches on st.  prepare(t), if any, runs
// before anything of the call is staged or enqueued (it may wait for the queries in flight).
using DevIn = const void* const*;
using DevOut = void* const*;
template <class Enqueue>
int query_body(rt_tracer* t, QueryWhere w, size_t n, QueryIns in, QueryOuts out, void (*prepare)(rt_tracer*), const Enqueue& enqueue) {
  return guarded(t, [&] {
    if (n == 0u) return;
    QueryState& q = t->queries;
    hipStream_t st = w.stream;
    if (w.device) t->use_device(); else st = host_query_stream(t);
    if (prepare) prepare(t);
    const void* d_in[2] = {nullptr, nullptr};
    void* d_out[2] = {nullptr, nullptr};
    size_t i = 0;
    for (const QueryIn& a : in) { d_in[i] = w.device ? a.p : a.p && a.bytes ? staged_in<unsigned char>(q.in[i], a.p, a.bytes, st) : nullptr; ++i; }
    i = 0;
    for (const QueryOut& a : out) { d_out[i] = w.device ? a.p : a.p && a.bytes ? room<unsigned char>(q.out[i], a.bytes) : nullptr; ++i; }
    enqueue(t, d_in, d_out, st);
    if (w.device) return;
    i = 0;
    for (const QueryOut& a : out) { if (d_out[i]) staged_out<unsigned char>(a.p, q.out[i], a.bytes, st); ++i; }
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// The one path of a query with arrays, in either form: the null handle, the query's own check(t) (whatever n is), the arrays, then
// the lock; a sharded handle is answered by this same call on its first band.
template <class Check, class Enqueue>
int run_query(rt_tracer* t, QueryWhere w, size_t n, QueryIns in, QueryOuts out, const char* misaligned, const Check& check,
              void (*prepare)(rt_tracer*), const Enqueue& enqueue) {
  if (!t || !check(t) || !query_arrays_ok(t, w, n, in, out, misaligned)) return RT_ERR_INVALID;
  return query_entry(t, [&](rt_tracer* band) { return run_query(band, w, n, in, out, misaligned, check, prepare, enqueue); },
                     [&] { return query_body(t, w, n, in, out, prepare, enqueue); });
}

// RT_ACCEL_REFIT: the tree of an earlier upload with as many records as the scene has triangles takes the new records and
// new boxes on the device (rt_refit.hpp), all on the query stream: the gather, one launch per level from the deepest up,
// the cost, between two events; one 16-byte copy of {flag, cost} and the synchronisation the build has too.  False: a
// triangle changed between finite and non-finite (the partition rule, rt_bvh_host.hpp) -- the caller builds.
inline bool refit_query_tree(rt_tracer* t, hipStream_t st) {
  QueryState& q = t->queries;
  const uint32_t n_nodes = static_cast<uint32_t>(q.bvh_info[0]), n_always = static_cast<uint32_t>(q.bvh_info[3]);
  const uint32_t n_leaf = q.bvh_leaf_records, depth = static_cast<uint32_t>(q.bvh_info[2]);
  q.d_refit_out.ensure(2u);
  q.h_refit_out.ensure(2u);
  if (!q.refit_begin) { q.refit_begin = Event::timing(); q.refit_end = Event::timing(); }
  HIP_CHECK(hipMemsetAsync(q.d_refit_out.get(), 0, 2u * sizeof(uint64_t), st));
  HIP_CHECK(hipEventRecord(q.refit_begin, st));
  HIP_CHECK(rtk::launch_refit_gather(t->d_tri.get(), t->d_tri_b.get(), t->n_tris, q.d_bvh_records.get(), n_leaf, n_leaf + n_always,
                                     reinterpret_cast<uint32_t*>(q.d_refit_out.get()), st));
  for (uint32_t l = depth; l-- > 0u;)
    HIP_CHECK(rtk::launch_refit_level(q.d_bvh_nodes.get(), n_nodes, q.d_bvh_records.get(), n_leaf, q.d_bvh_levels.get() + q.bvh_level_begin[l],
                                      q.bvh_level_begin[l + 1u] - q.bvh_level_begin[l], st));
  HIP_CHECK(rtk::launch_refit_cost(q.d_bvh_nodes.get(), n_nodes, reinterpret_cast<double*>(q.d_refit_out.get() + 1), st));
  HIP_CHECK(hipEventRecord(q.refit_end, st));
  HIP_CHECK(hipMemcpyAsync(q.h_refit_out.get(), q.d_refit_out.get(), 2u * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (static_cast<uint32_t>(q.h_refit_out.get()[0]) != 0u) { q.refit_fallbacks++; return false; }
  float ms = 0.0f;
  HIP_CHECK(hipEventElapsedTime(&ms, q.refit_begin, q.refit_end));
  q.refit_us = static_cast<uint64_t>(ms * 1000.0f + 0.5f);
  memcpy(&q.bvh_cost, q.h_refit_out.get() + 1, sizeof(double));
  q.refits++;
  q.bvh_scene = t->scene_generation;
  return true;
}

// RT_QUERY_BVH: the tree of the current scene, built on the host from the records the kernel intersects (read back from the
// device: for either upload layout they are what prep_triangles_kernel stored) and uploaded, all on the query stream -- the
// upload that made the records has returned, so the build waits for no Trace.  Queries in flight may still read the old
// tree: they are waited for before its buffers are rewritten.  Under RT_ACCEL_REFIT a tree of the same record count is
// refitted instead (refit_query_tree).
inline void ensure_query_tree(rt_tracer* t) {
  QueryState& q = t->queries;
  if (q.bvh_valid(t->scene_generation)) return;
  const hipStream_t st = q.stream();
  t->wait_queries();
  const size_t n = t->n_tris;
  if (n > rtb::kBvhMaxTris) throw HipFail{fmt("RT_QUERY_BVH: %zu triangles (at most %zu)", n, rtb::kBvhMaxTris)};
  if (q.accel_update == RT_ACCEL_REFIT && q.bvh_built && n != 0u && size_t(q.bvh_leaf_records) + q.bvh_info[3] == n &&
      refit_query_tree(t, st)) return;
  q.bvh_built = false;                                                  // (a failure below leaves no tree to refit)
  std::vector<float> a(n * 8u), b(n);
  if (n != 0u) {
    HIP_CHECK(hipMemcpyAsync(a.data(), t->d_tri.get(), n * 8u * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(b.data(), t->d_tri_b.get(), n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  const std::vector<float> rec = rtb::records_of_device(a.data(), b.data(), n);
  const rtb::Tree tree = rtb::build(rec.data(), n);
  q.d_bvh_nodes.ensure(std::max<size_t>(tree.nodes.size(), 1u) * 8u);
  q.d_bvh_records.ensure(std::max<size_t>(tree.records.size(), 1u) * 3u);
  q.d_bvh_levels.ensure(std::max<size_t>(tree.level_nodes.size(), 1u));
  if (!tree.nodes.empty()) HIP_CHECK(hipMemcpyAsync(q.d_bvh_nodes.get(), tree.nodes.data(), tree.nodes.size() * sizeof(rtb::Node), hipMemcpyHostToDevice, st));
  if (!tree.records.empty()) HIP_CHECK(hipMemcpyAsync(q.d_bvh_records.get(), tree.records.data(), tree.records.size() * sizeof(rtb::Record), hipMemcpyHostToDevice, st));
  if (!tree.level_nodes.empty()) HIP_CHECK(hipMemcpyAsync(q.d_bvh_levels.get(), tree.level_nodes.data(), tree.level_nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));                                   // (the host vectors go away; a caller's stream may run the query)
  q.bvh_info[0] = tree.nodes.size(); q.bvh_info[1] = tree.leaves; q.bvh_info[2] = tree.depth; q.bvh_info[3] = tree.always;
  q.bvh_info[4] = tree.build_us; q.bvh_info[5] = tree.bytes();
  q.bvh_leaf_records = static_cast<uint32_t>(tree.records.size() - tree.always);
  q.bvh_level_begin = tree.level_begin;
  if (q.bvh_level_begin.empty()) q.bvh_level_begin.push_back(0u);
  q.bvh_cost = q.bvh_cost_built = rtb::tree_cost(tree.nodes);
  q.refits = 0;
  q.bvh_scene = t->scene_generation;
  q.bvh_built = true;
}

// the valid tree (ensure_query_tree) as the traversal kernels take it
inline rtk::BvhParams query_bvh_params(const rt_tracer* t) {
  const QueryState& q = t->queries;
  rtk::BvhParams b;
  b.nodes = q.d_bvh_nodes.get(); b.records = q.d_bvh_records.get();
  b.n_nodes = static_cast<uint32_t>(q.bvh_info[0]); b.n_leaf_records = q.bvh_leaf_records;
  b.n_always = static_cast<uint32_t>(q.bvh_info[3]);
  // (rt_dbg_query_stack_cap can only lower it: the kernels' sp < stack_cap keeps every store inside the LDS sized from it)
  b.stack_cap = std::min(rtb::stack_capacity(static_cast<uint32_t>(q.bvh_info[2])), q.stack_cap);
  b.rho = RT_BVH_RHO * (static_cast<float>(q.slack_milli) / 1000.0f);
  return b;
}

// One launch of a query on `st`, behind every earlier query: QueryState::done then covers this one and all before it.  launch(p, b)
// gets the launches' camera snapshot and scene with p.flags = flags, and the valid tree under RT_QUERY_BVH when the query
// walks one (uses_tree), else b = nullptr: the scan.
template <class Launch>
void enqueue_launch(rt_tracer* t, hipStream_t st, uint32_t flags, bool uses_tree, Launch&& launch) {
  rtk::TraceParams p = t->params(1);
  p.flags = flags;
  const bool bvh = uses_tree && t->queries.accel == RT_QUERY_BVH;
  if (bvh) ensure_query_tree(t);
  if (!t->queries.done) t->queries.done = Event(hipEventDisableTiming);
  else HIP_CHECK(hipStreamWaitEvent(st, t->queries.done, 0));
  if (bvh) {
    const rtk::BvhParams b = query_bvh_params(t);
    HIP_CHECK(launch(p, &b));
  } else {
    HIP_CHECK(launch(p, static_cast<const rtk::BvhParams*>(nullptr)));
  }
  HIP_CHECK(hipEventRecord(t->queries.done, st));
}

// the point queries' slack on the box distance: rho_c takes the ray queries' (rt_dbg_query_accel_slack)
inline float closest_rho(const rt_tracer* t) { return RT_CLOSEST_RHO * (static_cast<float>(t->queries.slack_milli) / 1000.0f); }

// rays (or pixels) -> hits, under the tracer's hit rule
inline void enqueue_query(rt_tracer* t, size_t n, const float* rays, const uint32_t* pixels, float* rays_out, float4* hits,
                          hipStream_t st) {
  enqueue_launch(t, st, t->nearest_hit ? rtk::TRACE_NEAREST_HIT : 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
    return rtk::launch_query(p, b, t->fma, query_k(t, n), static_cast<uint32_t>(n), rays, pixels, rays_out, hits, st);
  });
}

// the direction count and the flags of the exposure entry points, checked whatever n is; t may be null (rt_dbg_exposure_rays)
inline bool exposure_args_ok(rt_tracer* t, const char* who, uint32_t n_dirs, uint32_t flags) {
  std::string msg;
  if (n_dirs == 0u || n_dirs > RT_MAX_DIRS) msg = fmt("%s: n_dirs = %u (1 to %u)", who, n_dirs, RT_MAX_DIRS);
  else if ((flags & ~RT_EXPOSURE_WORLD) != 0u) msg = fmt("%s: unknown flags 0x%x", who, flags);
  else return true;
  if (t) t->set_error(msg); else set_global_error(msg);
  return false;
}

// points -> one record per point.  One arithmetic for both math modes and no hit rule: the flags stay 0.  The tree is the ray
// queries' (ensure_query_tree, so RT_ACCEL_REFIT applies).
inline void enqueue_closest(rt_tracer* t, size_t n, const float* pts, float4* hits, hipStream_t st) {
  enqueue_launch(t, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
    return rtk::launch_closest(p, b, closest_rho(t), static_cast<uint32_t>(n), pts, hits, st);
  });
}

// What the entry points of one region shape (boxes, query triangles, hexahedra) differ in: the floats per query, the array's name in
// the alignment message and the launch function.
struct RegionShape {
  size_t floats;
  const char* array;
  hipError_t (*launch)(const rtk::TraceParams&, const rtk::BvhParams*, uint32_t, const float*, const int*, uint32_t, int*, uint32_t*,
                       hipStream_t);
};

static_assert(RT_SWEEP_SLACK == rtk::kSweepSlack, "include/rt_mi355x.h and rt_kernels.hpp state one slack");

// The signed queries' feature table (rt_features_host.hpp) of the current scene: built on the host from the
// tracer's copy of the rows of its last upload by the first signed query after that upload, keyed to scene_generation as
// ensure_query_tree keys the tree, and uploaded once on the query stream.  Queries in flight may still read the old table: they
// are waited for before its buffer is rewritten.  RT_ACCEL_REFIT does not apply: the table is rebuilt.
inline void ensure_feature_table(rt_tracer* t) {
  QueryState& q = t->queries;
  if (q.features_valid(t->scene_generation)) return;
  const hipStream_t st = q.stream();
  t->wait_queries();
  q.features_built = false;
  const size_t n = t->n_tris;
  if (q.scene_rows.size() != n * 12u) throw HipFail{fmt("signed query: the host copy of the scene holds %zu floats, the scene %zu triangles", q.scene_rows.size(), n)};
  const rtf::Table tab = rtf::build(q.scene_rows.data(), n, q.scene_rows_edges);
  q.d_features.ensure(std::max<size_t>(n * rtf::kFeaturesPerTri, 1u));
  if (n != 0u) {
    HIP_CHECK(hipMemcpyAsync(q.d_features.get(), tab.normals.data(), tab.bytes(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                                 // (the host vector goes away; a caller's stream may run the query)
  }
  q.features_info[0] = n; q.features_info[1] = tab.vertices; q.features_info[2] = tab.edges; q.features_info[3] = tab.contributing;
  q.features_info[4] = tab.build_us; q.features_info[5] = tab.bytes();
  q.features_scene = t->scene_generation;
  q.features_built = true;
}

// points and n * per_point records of them -> as many rt_side; no tree.  The table is valid (ensure_feature_table, called
// before anything of this query was enqueued: it may wait for the queries in flight).
inline void enqueue_sides(rt_tracer* t, size_t n, uint32_t per_point, const float* pts, const float4* hits, void* sides, hipStream_t st) {
  enqueue_launch(t, st, 0u, false, [&](const rtk::TraceParams& p, const rtk::BvhParams*) {
    return rtk::launch_sides(p, t->queries.d_features.get(), static_cast<uint32_t>(n), per_point, pts, hits, sides, st);
  });
}

}  // namespace rtr

extern "C" {

int rt_tracer_set_query_accel(rt_tracer* t, uint32_t mode) {
  if (!t) return RT_ERR_INVALID;
  if (mode != RT_QUERY_SCAN && mode != RT_QUERY_BVH) { t->set_error(fmt("rt_tracer_set_query_accel: unknown mode %u", mode)); return RT_ERR_INVALID; }
  return query_call(t, [&](rt_tracer* b) { return rt_tracer_set_query_accel(b, mode); }, [&] { t->queries.accel = mode; });
}

int rt_tracer_query_accel_info(rt_tracer* t, uint64_t out[8]) {
  if (!t || !out) return RT_ERR_INVALID;
  return query_call(t, [&](rt_tracer* b) { return rt_tracer_query_accel_info(b, out); }, [&] {
    const bool valid = t->queries.bvh_valid(t->scene_generation);
    out[0] = t->queries.accel; out[1] = valid ? 1u : 0u;
    for (int i = 0; i < 6; ++i) out[2 + i] = valid ? t->queries.bvh_info[i] : 0u;
  });
}

int rt_tracer_set_query_accel_update(rt_tracer* t, uint32_t policy) {
  if (!t) return RT_ERR_INVALID;
  if (policy != RT_ACCEL_REBUILD && policy != RT_ACCEL_REFIT) { t->set_error(fmt("rt_tracer_set_query_accel_update: unknown policy %u", policy)); return RT_ERR_INVALID; }
  // (checked before query_call takes api_mu, as every argument is)
  return query_call(t, [&](rt_tracer* b) { return rt_tracer_set_query_accel_update(b, policy); }, [&] { t->queries.accel_update = policy; });
}

int rt_tracer_query_accel_rebuild(rt_tracer* t) {
  if (!t) return RT_ERR_INVALID;
  return query_call(t, [&](rt_tracer* b) { return rt_tracer_query_accel_rebuild(b); }, [&] {
    t->queries.bvh_built = false;                                                // (the buffers stay; queries in flight may still walk them)
  });
}

int rt_tracer_query_accel_update_info(rt_tracer* t, uint64_t out[8]) {
  if (!t || !out) return RT_ERR_INVALID;
  return query_call(t, [&](rt_tracer* b) { return rt_tracer_query_accel_update_info(b, out); }, [&] {
    const bool valid = t->queries.bvh_valid(t->scene_generation);
    const double cost = valid ? t->queries.bvh_cost : 0.0, built = valid ? t->queries.bvh_cost_built : 0.0;
    out[0] = t->queries.accel_update; out[1] = t->queries.refits; out[2] = t->queries.refit_fallbacks; out[3] = t->queries.refit_us;
    memcpy(&out[4], &cost, sizeof(double)); memcpy(&out[5], &built, sizeof(double));
    out[6] = valid ? rtr::query_bvh_params(t).stack_cap : 0u;             // what the walks run with (rt_dbg_query_stack_cap lowers it)
    out[7] = 0u;
  });
}

int rt_dbg_query_accel_slack(rt_tracer* t, uint32_t slack_milli) {
  if (!t) return RT_ERR_INVALID;
  return query_call(t, [&](rt_tracer* b) { return rt_dbg_query_accel_slack(b, slack_milli); }, [&] { t->queries.slack_milli = slack_milli; });
}

int rt_dbg_query_stack_cap(rt_tracer* t, uint32_t cap) {
  if (!t) return RT_ERR_INVALID;
  return query_call(t, [&](rt_tracer* b) { return rt_dbg_query_stack_cap(b, cap); }, [&] { t->queries.stack_cap = cap; });
}

int rt_dbg_bvh_build(const rt_float4* rows, size_t count, int edges_layout, void* nodes, size_t node_capacity_bytes,
                     void* leaf_records, size_t leaf_capacity_bytes, uint64_t info[8]) {
  if (!rows || !info || count < 3u || count % 3u != 0u || count / 3u > rtb::kBvhMaxTris) return RT_ERR_INVALID;
  return guarded(nullptr, [&] {
    const size_t n = count / 3u;
    const std::vector<float> rec = rtb::records_of_rows(&rows[0].x, n, edges_layout != 0);
    const rtb::Tree tree = rtb::build(rec.data(), n);
    const size_t nb = tree.nodes.size() * sizeof(rtb::Node), rb = tree.records.size() * sizeof(rtb::Record);
    info[0] = rtb::kBvhMaxDepth; info[1] = 1u; info[2] = tree.nodes.size(); info[3] = tree.leaves; info[4] = tree.depth;
    info[5] = tree.always; info[6] = tree.build_us; info[7] = tree.bytes();
    if (node_capacity_bytes == 0u && leaf_capacity_bytes == 0u) return;  // sizes only
    if (!nodes || !leaf_records || node_capacity_bytes < nb || leaf_capacity_bytes < rb)
      throw HipFail{fmt("rt_dbg_bvh_build: the tree needs %zu + %zu bytes", nb, rb)};
    if (nb) memcpy(nodes, tree.nodes.data(), nb);
    if (rb) memcpy(leaf_records, tree.records.data(), rb);
  });
}

// what rt_dbg_bvh_refit may follow in its caller's arrays: every reference in range, children behind their parents
static bool tree_refs_ok(const rtb::Node* nodes, size_t n_nodes, const rtb::Record* recs, size_t n_leaf, size_t n) {
  for (size_t s = 0; s < n; ++s) if (recs[s].index >= n) return false;
  for (size_t i = 0; i < n_nodes; ++i)
    for (int k = 0; k < 4; ++k) {
      const uint32_t ref = nodes[i].child[k];
      if (ref == rtb::kBvhEmpty) continue;
      if (ref & rtb::kBvhLeaf) { if (size_t(ref & 0x0FFFFFFFu) + ((ref >> 28) & 3u) + 1u > n_leaf) return false; }
      else if (ref >= n_nodes || ref <= i) return false;
    }
  return true;
}

int rt_dbg_bvh_refit(const rt_float4* rows, size_t count, int edges_layout, void* nodes, size_t node_bytes, void* leaf_records,
                     size_t record_bytes, uint64_t info[8]) {
  if (!rows || !info || !leaf_records || count < 3u || count % 3u != 0u || count / 3u > rtb::kBvhMaxTris) return RT_ERR_INVALID;
  const size_t n = count / 3u, n_nodes = node_bytes / sizeof(rtb::Node);
  if (node_bytes % sizeof(rtb::Node) != 0u || record_bytes != n * sizeof(rtb::Record) || (n_nodes != 0u && !nodes)) return RT_ERR_INVALID;
  const size_t n_always = static_cast<size_t>(info[5]);
  if (n_always > n || info[2] != n_nodes) return RT_ERR_INVALID;
  rtb::Node* nd = static_cast<rtb::Node*>(nodes);
  rtb::Record* rc = static_cast<rtb::Record*>(leaf_records);
  if (!tree_refs_ok(nd, n_nodes, rc, n - n_always, n)) return RT_ERR_INVALID;
  bool ok = true;
  const int rcode = guarded(nullptr, [&] {
    const std::vector<float> rec = rtb::records_of_rows(&rows[0].x, n, edges_layout != 0);
    ok = rtb::refit(nd, n_nodes, rc, n - n_always, n_always, rec.data());
  });
  if (rcode != RT_OK) return rcode;
  if (!ok) { set_global_error("rt_dbg_bvh_refit: a triangle changed between finite and non-finite; the tree has to be built"); return RT_ERR_STATE; }
  return RT_OK;
}

double rt_dbg_bvh_tree_cost(const void* nodes, size_t node_bytes) {
  if (!nodes || node_bytes % sizeof(rtb::Node) != 0u) return 0.0;
  return rtb::tree_cost(static_cast<const rtb::Node*>(nodes), node_bytes / sizeof(rtb::Node));
}

int rt_dbg_query_tree_read(rt_tracer* t, void* nodes, size_t node_capacity_bytes, void* records, size_t record_capacity_bytes,
                           uint64_t info[8]) {
  if (!t || !info) return RT_ERR_INVALID;
  return query_entry(t, [&](rt_tracer* b) { return rt_dbg_query_tree_read(b, nodes, node_capacity_bytes, records, record_capacity_bytes, info); }, [&] {
    if (!t->queries.bvh_valid(t->scene_generation)) { t->set_error("rt_dbg_query_tree_read: no valid tree (the next RT_QUERY_BVH query makes one)"); return RT_ERR_STATE; }
    return guarded(t, [&] {
      const size_t nb = t->queries.bvh_info[0] * sizeof(rtb::Node), rb = (size_t(t->queries.bvh_leaf_records) + t->queries.bvh_info[3]) * sizeof(rtb::Record);
      info[0] = rtb::kBvhMaxDepth; info[1] = 1u;
      for (int i = 0; i < 6; ++i) info[2 + i] = t->queries.bvh_info[i];
      if (node_capacity_bytes == 0u && record_capacity_bytes == 0u) return;  // sizes only
      if (!nodes || !records || node_capacity_bytes < nb || record_capacity_bytes < rb)
        throw HipFail{fmt("rt_dbg_query_tree_read: the tree needs %zu + %zu bytes", nb, rb)};
      const hipStream_t st = host_query_stream(t);
      t->wait_queries();
      if (nb) HIP_CHECK(hipMemcpyAsync(nodes, t->queries.d_bvh_nodes.get(), nb, hipMemcpyDeviceToHost, st));
      if (rb) HIP_CHECK(hipMemcpyAsync(records, t->queries.d_bvh_records.get(), rb, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    });
  });
}

// rays -> hits, under the tracer's hit rule
static int intersect_query(rt_tracer* t, QueryWhere w, const float* rays, size_t n, rt_hit* hits) {
  return run_query(t, w, n, {{rays, n * 24u, 4u}}, {{hits, n * 16u, 16u}},
                   "rt_tracer_intersect_device: hits must be 16-byte aligned, rays 4-byte aligned", no_check, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_query(h, n, static_cast<const float*>(in[0]), nullptr, nullptr, static_cast<float4*>(out[0]), st);
                   });
}
int rt_tracer_intersect(rt_tracer* t, const float* rays, size_t n, rt_hit* hits) { return intersect_query(t, on_host(), rays, n, hits); }
int rt_tracer_intersect_device(rt_tracer* t, const float* rays, size_t n, rt_hit* hits, void* stream) {
  return intersect_query(t, on_device(stream), rays, n, hits);
}

// segments -> one byte per ray.  The hit rule plays no part (an OR over the primitives), so the flags stay 0.
static int occluded_query(rt_tracer* t, QueryWhere w, const float* segs, size_t n, uint8_t* occluded) {
  return run_query(t, w, n, {{segs, n * 32u, 16u}}, {{occluded, n, 1u}}, "rt_tracer_occluded_device: segs must be 16-byte aligned",
                   no_check, nullptr, [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_occluded(p, b, h->fma, query_k(h, n), static_cast<uint32_t>(n), static_cast<const float*>(in[0]),
                                                   static_cast<uint8_t*>(out[0]), st);
                     });
                   });
}
int rt_tracer_occluded(rt_tracer* t, const float* segs, size_t n, uint8_t* occluded) { return occluded_query(t, on_host(), segs, n, occluded); }
int rt_tracer_occluded_device(rt_tracer* t, const float* segs, size_t n, uint8_t* occluded, void* stream) {
  return occluded_query(t, on_device(stream), segs, n, occluded);
}

// points and a direction table -> one 64-bit mask per point (rt_exposure.hpp).  An OR per ray, as Occluded: the flags stay 0.
static int exposure_query(rt_tracer* t, QueryWhere w, const char* who, const float* points, size_t n, const float* dirs, uint32_t n_dirs,
                    uint32_t flags, uint64_t* masks) {
  return run_query(t, w, n, {{points, n * 32u, 16u}, {dirs, size_t(n_dirs) * 16u, 16u}}, {{masks, n * 8u, 8u}},
                   "rt_tracer_exposure_device: points and dirs must be 16-byte aligned, masks 8-byte aligned",
                   [&](rt_tracer* h) { return exposure_args_ok(h, who, n_dirs, flags); }, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_exposure(p, b, h->fma, static_cast<uint32_t>(n), static_cast<const float*>(in[0]),
                                                   static_cast<const float*>(in[1]), n_dirs, flags, static_cast<uint64_t*>(out[0]), st);
                     });
                   });
}
int rt_tracer_exposure(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags, uint64_t* masks) {
  return exposure_query(t, on_host(), "rt_tracer_exposure", points, n, dirs, n_dirs, flags, masks);
}
int rt_tracer_exposure_device(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags,
                              uint64_t* masks, void* stream) {
  return exposure_query(t, on_device(stream), "rt_tracer_exposure_device", points, n, dirs, n_dirs, flags, masks);
}

int rt_dbg_exposure_rays(rt_tracer* t, const float* points, size_t n, const float* dirs, uint32_t n_dirs, uint32_t flags, float* segs_out) {
  if (!exposure_args_ok(t, "rt_dbg_exposure_rays", n_dirs, flags)) return RT_ERR_INVALID;
  if (!t) {                                                              // the host evaluates the kernels' function
    if (n != 0u && (!points || !dirs || !segs_out)) { set_global_error("rt_dbg_exposure_rays: null array"); return RT_ERR_INVALID; }
    return guarded(nullptr, [&] { rtk::exposure_rays_host(n, points, dirs, n_dirs, flags, segs_out); });
  }
  if (!query_args_ok(t, n, points && dirs && segs_out)) return RT_ERR_INVALID;
  if (n * static_cast<uint64_t>(n_dirs) >= 0x80000000ull) { t->set_error("rt_dbg_exposure_rays: n * n_dirs must be below 2^31"); return RT_ERR_INVALID; }
  return query_call(t, [&](rt_tracer* b) { return rt_dbg_exposure_rays(b, points, n, dirs, n_dirs, flags, segs_out); }, [&] {
    if (n == 0u) return;
    const hipStream_t st = host_query_stream(t);
    DevArray<float> d_out(n * n_dirs * 8u);
    const float* d_points = staged_in<float>(t->queries.in[0], points, n * 8u, st);
    const float* d_dirs = staged_in<float>(t->queries.in[1], dirs, n_dirs * 4u, st);
    enqueue_launch(t, st, 0u, false, [&](const rtk::TraceParams&, const rtk::BvhParams*) {
      return rtk::launch_exposure_rays(static_cast<uint32_t>(n), d_points, d_dirs, n_dirs, flags, d_out.get(), st);
    });
    HIP_CHECK(hipMemcpyAsync(segs_out, d_out.get(), n * n_dirs * 8u * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// segments -> rows of max_hits records and one count per ray.  The order rule names no hit rule, so the flags stay 0.
static int intersect_all_query(rt_tracer* t, QueryWhere w, const char* who, const float* segs, size_t n, uint32_t max_hits, rt_hit* hits,
                               uint32_t* counts) {
  return run_query(t, w, n, {{segs, n * 32u, 16u}}, {{hits, n * max_hits * 16u, 16u}, {counts, n * 4u, 4u}},
                   "rt_tracer_intersect_all_device: segs and hits must be 16-byte aligned, counts 4-byte aligned",
                   [&](rt_tracer* h) { return query_row_ok(h, who, "max_hits", max_hits); }, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_allhits(p, b, h->fma, static_cast<uint32_t>(n), static_cast<const float*>(in[0]), max_hits,
                                                  static_cast<float4*>(out[0]), static_cast<uint32_t*>(out[1]), st);
                     });
                   });
}
int rt_tracer_intersect_all(rt_tracer* t, const float* segs, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts) {
  return intersect_all_query(t, on_host(), "rt_tracer_intersect_all", segs, n, max_hits, hits, counts);
}
int rt_tracer_intersect_all_device(rt_tracer* t, const float* segs, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts,
                                   void* stream) {
  return intersect_all_query(t, on_device(stream), "rt_tracer_intersect_all_device", segs, n, max_hits, hits, counts);
}

static int closest_point_query(rt_tracer* t, QueryWhere w, const float* pts, size_t n, rt_hit* out) {
  return run_query(t, w, n, {{pts, n * 16u, 16u}}, {{out, n * 16u, 16u}}, "rt_tracer_closest_point_device: pts and out must be 16-byte aligned",
                   no_check, nullptr, [&](rt_tracer* h, DevIn in, DevOut d_out, hipStream_t st) {
                     enqueue_closest(h, n, static_cast<const float*>(in[0]), static_cast<float4*>(d_out[0]), st);
                   });
}
int rt_tracer_closest_point(rt_tracer* t, const float* pts, size_t n, rt_hit* out) { return closest_point_query(t, on_host(), pts, n, out); }
int rt_tracer_closest_point_device(rt_tracer* t, const float* pts, size_t n, rt_hit* out, void* stream) {
  return closest_point_query(t, on_device(stream), pts, n, out);
}

// points (and their cursors, or nullptr) -> rows of max_hits records and one count per point, with enqueue_closest's tree and rho_c
static int closest_all_query(rt_tracer* t, QueryWhere w, const char* who, const float* pts, const rt_hit* after, size_t n, uint32_t max_hits,
                             rt_hit* hits, uint32_t* counts) {
  return run_query(t, w, n, {{pts, n * 16u, 16u}, {after, n * 16u, 16u, true}}, {{hits, n * max_hits * 16u, 16u}, {counts, n * 4u, 4u}},
                   "rt_tracer_closest_all_device: pts, after and hits must be 16-byte aligned, counts 4-byte aligned",
                   [&](rt_tracer* h) { return query_row_ok(h, who, "max_hits", max_hits); }, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_nearest(p, b, closest_rho(h), static_cast<uint32_t>(n), static_cast<const float*>(in[0]),
                                                  static_cast<const float4*>(in[1]), max_hits, static_cast<float4*>(out[0]),
                                                  static_cast<uint32_t*>(out[1]), st);
                     });
                   });
}
int rt_tracer_closest_all(rt_tracer* t, const float* pts, const rt_hit* after, size_t n, uint32_t max_hits, rt_hit* hits,
                          uint32_t* counts) {
  return closest_all_query(t, on_host(), "rt_tracer_closest_all", pts, after, n, max_hits, hits, counts);
}
int rt_tracer_closest_all_device(rt_tracer* t, const float* pts, const rt_hit* after, size_t n, uint32_t max_hits, rt_hit* hits,
                                 uint32_t* counts, void* stream) {
  return closest_all_query(t, on_device(stream), "rt_tracer_closest_all_device", pts, after, n, max_hits, hits, counts);
}

static int signed_distance_query(rt_tracer* t, QueryWhere w, const float* pts, size_t n, rt_hit* hits, rt_side* sides) {
  return run_query(t, w, n, {{pts, n * 16u, 16u}}, {{hits, n * 16u, 16u}, {sides, n * 8u, 8u}},
                   "rt_tracer_signed_distance_device: pts and hits must be 16-byte aligned, sides 8-byte aligned", no_check, ensure_feature_table,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {   // the closest kernel's output is the sides kernel's input
                     enqueue_closest(h, n, static_cast<const float*>(in[0]), static_cast<float4*>(out[0]), st);
                     enqueue_sides(h, n, 1u, static_cast<const float*>(in[0]), static_cast<const float4*>(out[0]), out[1], st);
                   });
}
int rt_tracer_signed_distance(rt_tracer* t, const float* pts, size_t n, rt_hit* hits, rt_side* sides) {
  return signed_distance_query(t, on_host(), pts, n, hits, sides);
}
int rt_tracer_signed_distance_device(rt_tracer* t, const float* pts, size_t n, rt_hit* hits, rt_side* sides, void* stream) {
  return signed_distance_query(t, on_device(stream), pts, n, hits, sides);
}

static int closest_sides_query(rt_tracer* t, QueryWhere w, const char* who, const float* pts, const rt_hit* hits, size_t n, uint32_t per_point,
                               rt_side* sides) {
  return run_query(t, w, n, {{pts, n * 16u, 16u}, {hits, n * per_point * 16u, 16u}}, {{sides, n * per_point * 8u, 8u}},
                   "rt_tracer_closest_sides_device: pts and hits must be 16-byte aligned, sides 8-byte aligned",
                   [&](rt_tracer* h) { return query_row_ok(h, who, "per_point", per_point); }, ensure_feature_table,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_sides(h, n, per_point, static_cast<const float*>(in[0]), static_cast<const float4*>(in[1]), out[0], st);
                   });
}
int rt_tracer_closest_sides(rt_tracer* t, const float* pts, const rt_hit* hits, size_t n, uint32_t per_point, rt_side* sides) {
  return closest_sides_query(t, on_host(), "rt_tracer_closest_sides", pts, hits, n, per_point, sides);
}
int rt_tracer_closest_sides_device(rt_tracer* t, const float* pts, const rt_hit* hits, size_t n, uint32_t per_point, rt_side* sides,
                                   void* stream) {
  return closest_sides_query(t, on_device(stream), "rt_tracer_closest_sides_device", pts, hits, n, per_point, sides);
}

// queries (and their cursors, or nullptr) -> rows of max_hits prims and one total per query (rt_overlap.hpp, rt_trioverlap.hpp,
// rt_hexoverlap.hpp).  One arithmetic for both math modes: the flags stay 0.  The tree is the ray queries' (ensure_query_tree, so
// RT_ACCEL_REFIT applies); no rho is passed.  max_hits is checked whatever n is; with 0 only the counts are made and prims may be null.
static int region_query(rt_tracer* t, QueryWhere w, const RegionShape& s, const char* who, const float* queries, const int32_t* after,
                        size_t n, uint32_t max_hits, int32_t* prims, uint32_t* counts) {
  const std::string misaligned = w.device ? fmt("%s: %s must be 16-byte aligned, after, prims and counts 4-byte aligned", who, s.array) : std::string();
  return run_query(t, w, n, {{queries, n * s.floats * 4u, 16u}, {after, n * 4u, 4u, true}},
                   {{prims, n * max_hits * 4u, 4u, max_hits == 0u}, {counts, n * 4u, 4u}}, misaligned.c_str(),
                   [&](rt_tracer* h) {
                     if (max_hits > RT_MAX_HITS) h->set_error(fmt("%s: max_hits = %u (0 to %u)", who, max_hits, RT_MAX_HITS));
                     return max_hits <= RT_MAX_HITS;
                   }, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return s.launch(p, b, static_cast<uint32_t>(n), static_cast<const float*>(in[0]), static_cast<const int32_t*>(in[1]), max_hits,
                                       static_cast<int32_t*>(out[0]), static_cast<uint32_t*>(out[1]), st);
                     });
                   });
}

static const RegionShape kBoxes{8u, "boxes", rtk::launch_overlap};
static const RegionShape kTriangles{12u, "tris", rtk::launch_overlap_triangles};
static const RegionShape kHexahedra{32u, "hexa", rtk::launch_overlap_hexahedra};   // 128 bytes per query

int rt_tracer_overlap(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                      uint32_t* counts) {
  return region_query(t, on_host(), kBoxes, "rt_tracer_overlap", boxes, after, n, max_hits, prims, counts);
}
int rt_tracer_overlap_device(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                             uint32_t* counts, void* stream) {
  return region_query(t, on_device(stream), kBoxes, "rt_tracer_overlap_device", boxes, after, n, max_hits, prims, counts);
}
int rt_tracer_overlap_triangles(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                uint32_t* counts) {
  return region_query(t, on_host(), kTriangles, "rt_tracer_overlap_triangles", tris, after, n, max_hits, prims, counts);
}
int rt_tracer_overlap_triangles_device(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                       uint32_t* counts, void* stream) {
  return region_query(t, on_device(stream), kTriangles, "rt_tracer_overlap_triangles_device", tris, after, n, max_hits, prims, counts);
}
int rt_tracer_overlap_hexahedra(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                uint32_t* counts) {
  return region_query(t, on_host(), kHexahedra, "rt_tracer_overlap_hexahedra", hexa, after, n, max_hits, prims, counts);
}
int rt_tracer_overlap_hexahedra_device(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                                       uint32_t* counts, void* stream) {
  return region_query(t, on_device(stream), kHexahedra, "rt_tracer_overlap_hexahedra_device", hexa, after, n, max_hits, prims, counts);
}

// slabs: the region query of rt_section.hpp, a RegionShape as the three above (the tree form is a kernel of its own)
static const RegionShape kPlanes{8u, "planes", rtk::launch_section};
int rt_tracer_section(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                      uint32_t* counts) {
  return region_query(t, on_host(), kPlanes, "rt_tracer_section", planes, after, n, max_hits, prims, counts);
}
int rt_tracer_section_device(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,
                             uint32_t* counts, void* stream) {
  return region_query(t, on_device(stream), kPlanes, "rt_tracer_section_device", planes, after, n, max_hits, prims, counts);
}

// slabs and n * per_plane prims of them -> as many rt_cut (rt_section.hpp); no tree and nothing to prepare
static int section_segments_query(rt_tracer* t, QueryWhere w, const char* who, const float* planes, const int32_t* prims, size_t n,
                                  uint32_t per_plane, uint32_t side, rt_cut* cuts) {
  return run_query(t, w, n, {{planes, n * 32u, 16u}, {prims, n * per_plane * 4u, 4u}}, {{cuts, n * per_plane * 32u, 16u}},
                   "rt_tracer_section_segments_device: planes and cuts must be 16-byte aligned, prims 4-byte aligned",
                   [&](rt_tracer* h) {
                     if (side > 1u) { h->set_error(fmt("%s: side = %u (0 or 1)", who, side)); return false; }
                     return query_row_ok(h, who, "per_plane", per_plane);
                   }, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, false, [&](const rtk::TraceParams& p, const rtk::BvhParams*) {
                       return rtk::launch_section_segments(p, static_cast<uint32_t>(n), per_plane, side, static_cast<const float*>(in[0]),
                                                           static_cast<const int32_t*>(in[1]), out[0], st);
                     });
                   });
}
int rt_tracer_section_segments(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane, uint32_t side,
                               rt_cut* cuts) {
  return section_segments_query(t, on_host(), "rt_tracer_section_segments", planes, prims, n, per_plane, side, cuts);
}
int rt_tracer_section_segments_device(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane, uint32_t side,
                                      rt_cut* cuts, void* stream) {
  return section_segments_query(t, on_device(stream), "rt_tracer_section_segments_device", planes, prims, n, per_plane, side, cuts);
}

// sweeps -> one record per sweep (rt_spherecast.hpp).  One arithmetic for both math modes and no hit rule: the flags stay 0.  The
// tree is the ray queries' (ensure_query_tree, so RT_ACCEL_REFIT applies); the walk's allowance beyond r takes the tracer's slack.
static int sphere_cast_query(rt_tracer* t, QueryWhere w, const float* sweeps, size_t n, rt_hit* hits) {
  return run_query(t, w, n, {{sweeps, n * 32u, 16u}}, {{hits, n * 16u, 16u}}, "rt_tracer_sphere_cast_device: sweeps and hits must be 16-byte aligned",
                   no_check, nullptr, [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_sphere_cast(p, b, static_cast<float>(h->queries.slack_milli) / 1000.0f, static_cast<uint32_t>(n),
                                                      static_cast<const float*>(in[0]), static_cast<float4*>(out[0]), st);
                     });
                   });
}
int rt_tracer_sphere_cast(rt_tracer* t, const float* sweeps, size_t n, rt_hit* hits) { return sphere_cast_query(t, on_host(), sweeps, n, hits); }
int rt_tracer_sphere_cast_device(rt_tracer* t, const float* sweeps, size_t n, rt_hit* hits, void* stream) {
  return sphere_cast_query(t, on_device(stream), sweeps, n, hits);
}

// query triangles -> one record and one witness per triangle (rt_tridistance.hpp), with enqueue_closest's tree, flags and rho_c
static int triangle_distance_query(rt_tracer* t, QueryWhere w, const float* tris, size_t n, rt_hit* hits, rt_witness* witness) {
  return run_query(t, w, n, {{tris, n * 48u, 16u}}, {{hits, n * 16u, 16u}, {witness, n * 16u, 16u}},
                   "rt_tracer_triangle_distance_device: tris, hits and witness must be 16-byte aligned", no_check, nullptr,
                   [&](rt_tracer* h, DevIn in, DevOut out, hipStream_t st) {
                     enqueue_launch(h, st, 0u, true, [&](const rtk::TraceParams& p, const rtk::BvhParams* b) {
                       return rtk::launch_triangle_distance(p, b, closest_rho(h), static_cast<uint32_t>(n), static_cast<const float*>(in[0]),
                                                            static_cast<float4*>(out[0]), static_cast<float4*>(out[1]), st);
                     });
                   });
}
int rt_tracer_triangle_distance(rt_tracer* t, const float* tris, size_t n, rt_hit* hits, rt_witness* witness) {
  return triangle_distance_query(t, on_host(), tris, n, hits, witness);
}
int rt_tracer_triangle_distance_device(rt_tracer* t, const float* tris, size_t n, rt_hit* hits, rt_witness* witness, void* stream) {
  return triangle_distance_query(t, on_device(stream), tris, n, hits, witness);
}

int rt_dbg_feature_normals(const rt_float4* rows, size_t count, int edges_layout, void* out, size_t capacity_bytes, uint64_t info[8]) {
  if (!rows || !info || count < 3u || count % 3u != 0u || count / 3u > rtb::kBvhMaxTris) return RT_ERR_INVALID;
  return guarded(nullptr, [&] {
    const size_t n = count / 3u;
    const rtf::Table tab = rtf::build(&rows[0].x, n, edges_layout != 0);
    info[0] = n; info[1] = tab.vertices; info[2] = tab.edges; info[3] = tab.contributing; info[4] = tab.build_us; info[5] = tab.bytes();
    info[6] = info[7] = 0u;
    if (capacity_bytes == 0u) return;                                    // sizes only
    if (!out || capacity_bytes < tab.bytes()) throw HipFail{fmt("rt_dbg_feature_normals: the table needs %zu bytes", tab.bytes())};
    memcpy(out, tab.normals.data(), tab.bytes());
  });
}

int rt_tracer_pick(rt_tracer* t, const uint32_t* pixels, size_t n, rt_hit* hits, float* rays) {
  const QueryIns in = {{pixels, n * 8u, 4u}};
  const QueryOuts out = {{hits, n * 16u, 16u}, {rays, n * 24u, 4u, true}};
  if (!t || !query_arrays_ok(t, on_host(), n, in, out, nullptr)) return RT_ERR_INVALID;
  const auto forward = [&](rt_tracer* b) {
    multi_push_camera(t);                                                // the camera of the whole frame
    return rt_tracer_pick(b, pixels, n, hits, rays);
  };
  return query_entry(t, forward, [&] {
    for (size_t i = 0; i < n; ++i) {                                     // full-image coordinates (a band may pick any row)
      if (pixels[2u * i] >= t->W || pixels[2u * i + 1u] >= t->H) {
        t->set_error(fmt("Pick: pixel (%u, %u) is outside the %u x %u image", pixels[2u * i], pixels[2u * i + 1u], t->W, t->H));
        return RT_ERR_INVALID;
      }
    }
    return query_body(t, on_host(), n, in, out, nullptr, [&](rt_tracer* h, DevIn d_in, DevOut d_out, hipStream_t st) {
      enqueue_query(h, n, nullptr, static_cast<const uint32_t*>(d_in[0]), static_cast<float*>(d_out[1]), static_cast<float4*>(d_out[0]), st);
    });
  });
}

int rt_tracer_focus_at(rt_tracer* t, uint32_t x, uint32_t y, float* focal_length) {
  if (!t) return RT_ERR_INVALID;
  const uint32_t px[2] = {x, y};
  rt_hit h;
  const int rc = rt_tracer_pick(t, px, 1, &h, nullptr);
  if (rc != RT_OK) return rc;
  if (h.prim < 0) {
    t->set_error(fmt("FocusAt: pixel (%u, %u) sees the background", x, y));
    return RT_ERR_INVALID;
  }
  if (!(h.t > 0.0f && h.t < INFINITY)) {
    t->set_error(fmt("FocusAt: the hit of pixel (%u, %u) is not in front of the camera (t = %g)", x, y, static_cast<double>(h.t)));
    return RT_ERR_INVALID;
  }
  {
    std::lock_guard<std::mutex> lk(t->state_mu);                         // the focal length only: fov and aperture keep their bits
    t->cam.focal = h.t;
  }
  if (focal_length) *focal_length = h.t;
  return RT_OK;
}

}  // extern "C"
