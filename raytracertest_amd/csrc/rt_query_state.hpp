// rt_query_state.hpp -- rtr::QueryState, what the ray, point and region queries of a tracer own (rt_tracer::queries).
// rt_query_api.hpp is its user; the uploads and quiesce() of rt_tracer.hip call wait() and write scene_rows.
#pragma once
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_hip_host.hpp"

namespace rtr {

struct QueryState {
  Stream stream_q;                    // created by the first query (stream()), highest priority; declared first: destroyed last
  // An event behind every query enqueued (on stream_q or a caller's stream) that covers all earlier ones -- what uploads and
  // destroy wait for before they free the scene's records.
  Event done;
  hipStream_t stream() {
    int lo = 0, hi = 0;
    if (!stream_q) stream_q = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo ? Stream(hipStreamNonBlocking, hi) : Stream(hipStreamNonBlocking);
    return stream_q;
  }
  void wait() { if (done) HIP_CHECK(hipEventSynchronize(done)); }
  // Grow-only staging of the host-array entry points, as bytes: query_body (rt_query_api.hpp) stages the i-th input array of a
  // call's description through in[i] and its i-th output through out[i] (staged_in, room, staged_out).  No query has more than two
  // inputs and two outputs (rt_tracer_closest_all) and each waits for its stream before it returns.
  DevArray<unsigned char> in[2], out[2];
  // RT_QUERY_BVH (rt_bvh_host.hpp, rt_bvh.hpp): the tree of the scene of generation bvh_scene, built by the first query in
  // that mode after an upload (rt_query_api.hpp, under api_mu).  The buffers are grow-only; a rebuild waits for the queries.
  uint32_t accel = RT_QUERY_SCAN;
  uint32_t slack_milli = 1000u;                       // rt_dbg_query_accel_slack: multiplies the box test's rho
  uint32_t stack_cap = UINT32_MAX;                    // rt_dbg_query_stack_cap: an upper limit on the walks' stack entries per lane
  DevArray<float4> d_bvh_nodes, d_bvh_records;
  bool bvh_built = false;
  uint32_t bvh_scene = 0;                             // scene_generation the tree was built for
  uint64_t bvh_info[6] = {0, 0, 0, 0, 0, 0};          // nodes, leaves, depth, always-tested, build us, device bytes
  uint32_t bvh_leaf_records = 0;
  bool bvh_valid(uint32_t scene_generation) const { return bvh_built && bvh_scene == scene_generation; }
  // The signed queries (rt_features_host.hpp, rt_sides.hpp): the host copy of the rows of the last upload, which
  // the feature table is welded from, and the table of the scene of generation features_scene, built by the first signed query
  // after an upload (rt_query_api.hpp, under api_mu).  The buffer is grow-only; a rebuild waits for the queries.
  std::vector<float> scene_rows;                      // 12 floats per triangle, as uploaded
  bool scene_rows_edges = false;
  DevArray<float4> d_features;                        // 7 float4 per triangle
  bool features_built = false;
  uint32_t features_scene = 0;
  uint64_t features_info[6] = {0, 0, 0, 0, 0, 0};     // triangles, welded vertices, edges, contributing triangles, build us, bytes
  bool features_valid(uint32_t scene_generation) const { return features_built && features_scene == scene_generation; }
  // RT_ACCEL_REFIT (rt_refit.hpp): what the next query in RT_QUERY_BVH mode does with a tree of an earlier
  // upload.  bvh_built stays set across uploads -- the device tree keeps its topology, and its record count decides whether
  // a refit may replace the build; rt_tracer_query_accel_rebuild clears it.
  uint32_t accel_update = RT_ACCEL_REBUILD;
  DevArray<uint32_t> d_bvh_levels;                    // the node indices grouped by level, root first (rtb::Tree::level_nodes)
  std::vector<uint32_t> bvh_level_begin;              // depth + 1 offsets into it
  DevArray<uint64_t> d_refit_out;                     // {class-change flag, the cost as a double}
  PinnedArray<uint64_t> h_refit_out;
  Event refit_begin, refit_end;
  uint64_t refits = 0, refit_fallbacks = 0, refit_us = 0;   // since the last build; over the tracer's life; the last refit's
  double bvh_cost = 0.0, bvh_cost_built = 0.0;
};

}  // namespace rtr
