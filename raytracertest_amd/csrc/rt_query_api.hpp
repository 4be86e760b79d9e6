// rt_query_api.hpp -- the ray-query entry points of include/rt_mi355x.h (rt_tracer_intersect*, rt_tracer_pick,
// rt_tracer_focus_at).  Included by rt_tracer.hip.
//
// A query is not an exclusive() entry point: it never cancels or joins a running Trace.  It is serialised with the other API
// calls by api_mu, reads only the scene and a snapshot of the camera (params(), under state_mu), and runs on a stream of its
// own (stream_q, created by the first query) or on the caller's.  query_done, recorded behind every query, is what the scene
// uploads and destroy wait for before they touch the records a query may still read.
#pragma once
#include <cmath>

namespace rtr {

constexpr size_t kQueryMaxRays = 0xFFFFFFFFu;

// K rays per lane: 4 once a batch fills the GPU's resident blocks at K = 4 (256 CUs x 4 blocks of 256 lanes), 2 once it
// does so at K = 2, else 1 -- a pick of one pixel is one block with K = 1.  rt_options.samples_in_flight forces it.
inline int query_k(const rt_tracer* t, size_t n) {
  if (t->k_req == 1 || t->k_req == 2 || t->k_req == 4) return static_cast<int>(t->k_req);
  constexpr size_t kResidentLanes = 256u * 4u * 256u;
  return n >= 4u * kResidentLanes ? 4 : n >= 2u * kResidentLanes ? 2 : 1;
}

inline hipStream_t query_stream(rt_tracer* t) {
  if (!t->stream_q) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo) t->stream_q = Stream(hipStreamNonBlocking, hi);
    else t->stream_q = Stream(hipStreamNonBlocking);
  }
  return t->stream_q;
}

// rays (or pixels) -> hits on `st`, behind every earlier query: query_done then covers this one and all before it
inline void enqueue_query(rt_tracer* t, size_t n, const float* rays, const uint32_t* pixels, float* rays_out, float4* hits,
                          hipStream_t st) {
  rtk::TraceParams p = t->params(1);                                     // the launches' camera snapshot and scene
  p.flags = t->nearest_hit ? rtk::TRACE_NEAREST_HIT : 0u;
  if (!t->query_done) t->query_done = Event(hipEventDisableTiming);
  else HIP_CHECK(hipStreamWaitEvent(st, t->query_done, 0));
  HIP_CHECK(rtk::launch_query(p, t->fma, query_k(t, n), static_cast<uint32_t>(n), rays, pixels, rays_out, hits, st));
  HIP_CHECK(hipEventRecord(t->query_done, st));
}

inline bool query_args_ok(rt_tracer* t, size_t n, const void* a, const void* b) {
  if (n == 0u) return true;
  if (!a || !b) { t->set_error("query: null array"); return false; }
  if (n > kQueryMaxRays) { t->set_error(fmt("query: %zu rays (at most %zu)", n, kQueryMaxRays)); return false; }
  return true;
}

}  // namespace rtr

extern "C" {

int rt_tracer_intersect(rt_tracer* t, const float* rays, size_t n, rt_hit* hits) {
  if (!t) return RT_ERR_INVALID;
  if (!query_args_ok(t, n, rays, hits)) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {
    const int rc = rt_tracer_intersect(t->mg->bands[0], rays, n, hits);
    if (rc != RT_OK) t->set_error(t->mg->bands[0]->last_error);
    return rc;
  }
  return guarded(t, [&] {
    if (n == 0u) return;
    t->use_device();
    const hipStream_t st = query_stream(t);
    t->d_q_rays.ensure(n * 6u);
    t->d_q_hits.ensure(n);
    HIP_CHECK(hipMemcpyAsync(t->d_q_rays.get(), rays, n * 6u * sizeof(float), hipMemcpyHostToDevice, st));
    enqueue_query(t, n, t->d_q_rays.get(), nullptr, nullptr, t->d_q_hits.get(), st);
    HIP_CHECK(hipMemcpyAsync(hits, t->d_q_hits.get(), n * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int rt_tracer_intersect_device(rt_tracer* t, const float* rays, size_t n, rt_hit* hits, void* stream) {
  if (!t) return RT_ERR_INVALID;
  if (!query_args_ok(t, n, rays, hits)) return RT_ERR_INVALID;
  if (n != 0u && (reinterpret_cast<uintptr_t>(hits) % 16u != 0u || reinterpret_cast<uintptr_t>(rays) % 4u != 0u)) {
    t->set_error("rt_tracer_intersect_device: hits must be 16-byte aligned, rays 4-byte aligned");
    return RT_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {
    const int rc = rt_tracer_intersect_device(t->mg->bands[0], rays, n, hits, stream);
    if (rc != RT_OK) t->set_error(t->mg->bands[0]->last_error);
    return rc;
  }
  return guarded(t, [&] {
    if (n == 0u) return;
    t->use_device();
    enqueue_query(t, n, rays, nullptr, nullptr, reinterpret_cast<float4*>(hits), static_cast<hipStream_t>(stream));
  });
}

int rt_tracer_pick(rt_tracer* t, const uint32_t* pixels, size_t n, rt_hit* hits, float* rays) {
  if (!t) return RT_ERR_INVALID;
  if (!query_args_ok(t, n, pixels, hits)) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {
    multi_push_camera(t);                                                // the camera of the whole frame
    const int rc = rt_tracer_pick(t->mg->bands[0], pixels, n, hits, rays);
    if (rc != RT_OK) t->set_error(t->mg->bands[0]->last_error);
    return rc;
  }
  for (size_t i = 0; i < n; ++i) {                                       // full-image coordinates (a band may pick any row)
    if (pixels[2u * i] >= t->W || pixels[2u * i + 1u] >= t->H) {
      t->set_error(fmt("Pick: pixel (%u, %u) is outside the %u x %u image", pixels[2u * i], pixels[2u * i + 1u], t->W, t->H));
      return RT_ERR_INVALID;
    }
  }
  return guarded(t, [&] {
    if (n == 0u) return;
    t->use_device();
    const hipStream_t st = query_stream(t);
    t->d_q_pixels.ensure(n * 2u);
    t->d_q_hits.ensure(n);
    if (rays) t->d_q_rays.ensure(n * 6u);
    HIP_CHECK(hipMemcpyAsync(t->d_q_pixels.get(), pixels, n * 2u * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    enqueue_query(t, n, nullptr, t->d_q_pixels.get(), rays ? t->d_q_rays.get() : nullptr, t->d_q_hits.get(), st);
    HIP_CHECK(hipMemcpyAsync(hits, t->d_q_hits.get(), n * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
    if (rays) HIP_CHECK(hipMemcpyAsync(rays, t->d_q_rays.get(), n * 6u * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
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
