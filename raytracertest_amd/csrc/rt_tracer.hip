// rt_tracer.hip -- the C ABI of include/rt_mi355x.h over struct rt_tracer (rt_tracer.hpp).
#include "rt_tracer.hpp"

#include <map>

namespace rtr {

std::mutex g_err_mu;
std::string g_last_error;

void set_global_error(const std::string& s) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_last_error = s;
  static const bool log = getenv("RT_MI355X_LOG") != nullptr;
  if (log) fprintf(stderr, "[rt_mi355x] %s\n", s.c_str());
}

// jump table: built once per process, uploaded once per device
std::mutex g_jump_mu;
std::vector<uint32_t> g_jump_host;
std::map<int, uint32_t*> g_jump_dev;    // per device: the jump table followed by the window tables

const std::vector<uint32_t>& jump_host() {
  std::lock_guard<std::mutex> lk(g_jump_mu);
  if (g_jump_host.empty()) g_jump_host = rth::build_jump_table();
  return g_jump_host;
}

uint32_t* jump_device(int device) {
  const std::vector<uint32_t>& h = jump_host();
  std::lock_guard<std::mutex> lk(g_jump_mu);
  auto it = g_jump_dev.find(device);
  if (it != g_jump_dev.end()) return it->second;
  static const std::vector<uint32_t> win = rth::build_window_tables(h);
  uint32_t* d = nullptr;
  HIP_CHECK(hipMalloc(&d, (h.size() + win.size()) * sizeof(uint32_t)));
  HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d + h.size(), win.data(), win.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  g_jump_dev[device] = d;
  return d;
}

size_t buffer_bytes(rt_tracer* t, int which) {
  const size_t n = t->npix();          // (a multi-device tracer: W x H of the whole frame)
  switch (which) {
    case RT_BUF_RENDER: return n * sizeof(float4);
    case RT_BUF_COUNTS: return n * sizeof(uint32_t);
    case RT_BUF_IMAGE: return n * sizeof(uint32_t);
    case RT_BUF_RNG: return n * 6 * sizeof(uint32_t);
    case RT_BUF_FRAME: {               // the gathered frame: on the root of a group only
      const Group* g = t->mg ? &t->mg->group : t->grp;
      return (g && g->has_root) ? g->frame_bytes() : 0;
    }
    default: return 0;
  }
}

void* buffer_ptr(rt_tracer* t, int which) {
  if (which == RT_BUF_FRAME || (t->mg && which == RT_BUF_IMAGE)) {
    Group* g = t->mg ? &t->mg->group : t->grp;
    return (g && g->has_root) ? g->d_frame[g->last_b < 0 ? 0 : g->last_b] : nullptr;
  }
  if (t->mg) return nullptr;           // per-band buffers of a multi-device tracer: rt_tracer_read_buffer assembles them
  switch (which) {
    case RT_BUF_RENDER: return t->d_render.get();
    case RT_BUF_COUNTS: return t->d_counts.get();
    case RT_BUF_IMAGE: return t->d_image.get();
    case RT_BUF_RNG: return t->d_rng.get();
    default: return nullptr;
  }
}

// rt_tracer_kernel_time / rt_tracer_launch_time: the first band's sums for a multi-device tracer; a reset applies to every band
static int read_clock(rt_tracer* t, bool span, double* total_ms, uint64_t* launches, int reset_after) {
  if (!t) return RT_ERR_INVALID;
  if (t->mg) {
    const int rc = read_clock(t->mg->bands[0], span, total_ms, launches, reset_after);
    if (reset_after) for (size_t k = 1; k < t->mg->bands.size(); ++k) (void)read_clock(t->mg->bands[k], span, nullptr, nullptr, 1);
    return rc;
  }
  t->clock.read(span, total_ms, launches, reset_after != 0);
  return RT_OK;
}

int require_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_global_error(fmt("no HIP device available (%s); librt_mi355x has no CPU fallback",
                         e == hipSuccess ? "device count 0" : hipGetErrorString(e)));
    return RT_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    set_global_error(fmt("device %d out of range (%d devices)", device, n));
    return RT_ERR_INVALID;
  }
  return RT_OK;
}

}  // namespace rtr

#include "rt_multi_api.hpp"

using namespace rtr;

extern "C" {

#ifndef RT_KERNEL_SOURCE_HASH
#define RT_KERNEL_SOURCE_HASH "unknown"
#endif
const char* rt_version(void) { return "rt_mi355x 0.2 (gfx950, kernels=" RT_KERNEL_SOURCE_HASH ")"; }

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* rt_last_error(void) {
  static thread_local std::string copy;
  std::lock_guard<std::mutex> lk(g_err_mu);
  copy = g_last_error;
  return copy.c_str();
}

const char* rt_tracer_last_error(rt_tracer* t) {
  static thread_local std::string copy;
  if (!t) return rt_last_error();
  std::lock_guard<std::mutex> lk(t->err_mu);
  copy = t->last_error;
  return copy.c_str();
}

int rt_tracer_create_ex(const uint32_t imageSize[2], const float cameraPosition[3],
                        const float cameraAngles[2], float fov, float focalLength, float aperture,
                        const rt_options* options, rt_tracer** out) {
  if (!out) return RT_ERR_INVALID;
  *out = nullptr;
  if (!imageSize || !cameraAngles || imageSize[0] == 0 || imageSize[1] == 0) {
    set_global_error("rt_tracer_create: invalid image size or camera angles");
    return RT_ERR_INVALID;
  }
  rt_options opt;
  memset(&opt, 0, sizeof opt);
  opt.use_time_seed = 1;                                                 // Random.cu:45 by default
  if (options) {
    const size_t n = options->struct_size < sizeof(opt) ? options->struct_size : sizeof(opt);
    if (n < 8) { set_global_error("rt_options.struct_size not set"); return RT_ERR_INVALID; }
    opt.use_time_seed = 0;
    memcpy(&opt, options, n);
  }
  // the geometry is judged before a device is asked for anything
  const std::string refused = band_refusal(imageSize[0], opt.full_height ? opt.full_height : imageSize[1], imageSize[1]);
  if (!refused.empty()) { set_global_error("rt_tracer_create: " + refused); return RT_ERR_INVALID; }
  int rc = require_device(opt.device);
  if (rc != RT_OK) return rc;

  rt_tracer* t = new rt_tracer();
  t->device = opt.device;
  t->W = imageSize[0];
  if (opt.full_height) {
    t->band_mode = true;
    t->H = opt.full_height; t->row0 = opt.row_begin; t->rows = imageSize[1];
    if (static_cast<uint64_t>(t->row0) + t->rows > t->H) {
      delete t;
      set_global_error("row band exceeds full_height");
      return RT_ERR_INVALID;
    }
  } else {
    t->H = imageSize[1]; t->row0 = 0; t->rows = imageSize[1];
  }
  t->seed = opt.use_time_seed ? static_cast<uint64_t>(static_cast<uint32_t>(time(nullptr))) : opt.seed;
  t->fma = opt.math_mode != RT_MATH_STRICT;
  t->filter = (opt.flags & RT_FLAG_NO_FILTER) == 0;
  t->bin = (opt.flags & RT_FLAG_NO_BINNING) == 0;
  t->nearest_hit = (opt.flags & RT_FLAG_NEAREST_HIT) != 0;
  t->smooth_normals = (opt.flags & RT_FLAG_SMOOTH_NORMALS) != 0;
  t->env = Env();                                                        // (tests flip switches between tracers of one process: a snapshot per tracer)
  t->pretest = !t->env.no_pretest;
  t->sure_hit = (opt.flags & RT_FLAG_NO_SURE_HIT) == 0;
  t->split_launches = !t->env.no_split;
  t->macro = (opt.flags & RT_FLAG_NO_MACRO_BINS) == 0;
  t->super_level = (opt.flags & RT_FLAG_NO_SUPER_BINS) == 0;
  t->k_req = opt.samples_in_flight;
  t->chunk_req = opt.lds_chunk;
  t->bin_list_req = opt.bin_list;
  Camera& c = t->cam;
  for (int i = 0; i < 3; ++i) c.position[i] = cameraPosition ? cameraPosition[i] : 0.0f;
  c.angles[0] = cameraAngles[0]; c.angles[1] = cameraAngles[1];
  c.fov = Camera::radians(fov);                                          // ThinLensCamera.cuh:23
  c.focal = focalLength; c.aperture = aperture;
  c.transform();                                                         // :27
  rc = guarded(t, [&] {
    t->use_device();
    t->stream = Stream(hipStreamNonBlocking);
    // The runtime maps streams onto a few hardware queues.  The two streams of the first tracer of a process get queues
    // of their own; a tracer created while another one is alive on the device was measured 20 % slower (its two
    // half-frame kernels serialise on one queue; tools/placement_probe.py); GPU_MAX_HW_QUEUES=8 in the environment cures it.
    t->stream_b = Stream(hipStreamNonBlocking);
    int lo = 0, hi = 0;                                                  // (numerically lower = higher priority)
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo) t->stream_l = Stream(hipStreamNonBlocking, hi);
    else t->stream_l = Stream(hipStreamNonBlocking);
    t->stagger_event = Event(hipEventDisableTiming);
    t->d_half_cost.ensure(2);
    HIP_CHECK(hipMemset(t->d_half_cost.get(), 0, 2 * sizeof(uint32_t)));
    HIP_CHECK(hipDeviceSynchronize());                                    // (a null-stream memset is not ordered with the list stream)
    t->h_half_cost.ensure(1);
    *t->h_half_cost.get() = 0ull;
    t->lists.create(t->stream, t->stream_b, t->stream_l, &t->calls);
    t->handoff_event = Event(hipEventDisableTiming);
    t->join_event = Event(hipEventDisableTiming);
    t->fork_event = Event(hipEventDisableTiming);
    t->create_buffers();
  });
  if (rc != RT_OK) {
    // the reference's ctor logs and carries on with null buffers (RayTracerImpl.cu:42-45);
    // a C ABI can do better: report, release, hand back nothing.
    std::string why = t->last_error;
    rt_tracer_destroy(t);
    set_global_error("rt_tracer_create: " + why);
    return rc;
  }
  *out = t;
  return RT_OK;
}

int rt_tracer_create(const uint32_t imageSize[2], const float cameraPosition[3],
                     const float cameraAngles[2], float fov, float focalLength, float aperture,
                     rt_tracer** out) {
  return rt_tracer_create_ex(imageSize, cameraPosition, cameraAngles, fov, focalLength, aperture,
                             nullptr, out);
}

void rt_tracer_destroy(rt_tracer* t) {                                   // RayTracerImpl.cu:48-67
  if (!t) return;
  t->stopped = true;
  t->render.shutdown();
  if (t->mg) {                                                           // multi-device: the bands own the device state
    multi_destroy(t);
    delete t;
    return;
  }
  member_leave(t);
  t->quiesce();
  delete t;                                                              // the owning members release the rest
}

int rt_tracer_trace(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration,
                    uint32_t updateInterval) {
  if (!t) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  return guarded(t, [&] {
    t->cancel_and_join();                                                // :72-77
    t->completed = false;
    if (t->mg) t->render.run([=] { multi_trace_funct(t, iterationCount, samplesPerIteration, updateInterval); });
    else t->render.run([=] { t->trace_funct(iterationCount, samplesPerIteration, updateInterval); });   // :80-85
  });
}

void rt_tracer_stop(rt_tracer* t) {                                      // :89-92
  if (t) t->stopped = true;
}

int rt_tracer_wait(rt_tracer* t) {
  if (!t) return 0;
  std::lock_guard<std::mutex> lk(t->api_mu);
  t->render.wait_idle();
  t->stopped = false;
  return t->completed ? 1 : 0;
}

int rt_tracer_resize(rt_tracer* t, const uint32_t size[2]) {             // :94-103
  if (!t || !size || size[0] == 0 || size[1] == 0) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    if (t->mg) { multi_resize(t, size[0], size[1]); return; }
    if (t->grp) throw HipFail{"Resize: the tracer is a member of a multi-process group (leave and re-join with the new bands)"};
    const std::string refused = band_refusal(size[0], t->band_mode ? t->H : size[1], size[1]);   // before the buffers go
    if (!refused.empty()) throw BadArgument{refused};
    t->use_device();
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    t->release_buffers();
    t->W = size[0];
    if (t->band_mode) {
      if (static_cast<uint64_t>(t->row0) + size[1] > t->H) throw HipFail{"row band exceeds full_height"};
      t->rows = size[1];
    } else {
      t->H = size[1]; t->rows = size[1];
    }
    t->create_buffers();
  });
}

void rt_tracer_set_camera_parameters(rt_tracer* t, float fov, float focalLength, float aperture) {
  if (!t) return;                                                        // :105-112
  std::lock_guard<std::mutex> lk(t->state_mu);
  t->cam.fov = Camera::radians(fov);
  t->cam.focal = focalLength;
  t->cam.aperture = aperture;
}

void rt_tracer_rotate_camera(rt_tracer* t, const float angles[2]) {      // :114-117
  if (!t || !angles) return;
  std::lock_guard<std::mutex> lk(t->state_mu);
  t->cam.angles[0] += angles[0];                                         // ThinLensCamera.cuh:104-108
  t->cam.angles[1] += angles[1];
  t->cam.transform();
}

static int upload_scene_impl(rt_tracer* t, const rt_float4* hostData, size_t count, bool edges) {
  if (!t) return RT_ERR_INVALID;
  if (!hostData || count < 3 || count % 3 != 0) {                        // :121-125
    t->set_error(fmt("UploadScene got invalid triangle list. Size = %zu", count));
    return RT_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {                                                           // the scene is replicated on every device
    int rc = guarded(t, [&] { t->cancel_and_join(); multi_sync_all(t); });
    for (rt_tracer* b : t->mg->bands) {
      if (rc != RT_OK) break;
      rc = upload_scene_impl(b, hostData, count, edges);
      if (rc != RT_OK) t->set_error(b->last_error);
    }
    if (rc == RT_OK) { t->n_tris = static_cast<uint32_t>(count / 3); t->scene_generation++; }
    return rc;
  }
  return guarded(t, [&] {
    t->cancel_and_join();
    t->use_device();
    t->settle();                                                         // owed RNG draws, while the lists of the old scene say whose
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    t->sync_list_stream();                                               // (a list build may still be reading the old records)
    t->wait_queries();                                                   // (and so may a query)
    t->d_tri.reset(); t->d_tri_b.reset(); t->d_tri_color.reset(); t->d_tri_n.reset();   // :128-137
    t->n_tris = 0;
    t->queries.scene_rows.clear();
    const uint32_t n = static_cast<uint32_t>(count / 3);                 // :139
    DevArray<float4> verts(count);
    t->d_tri.ensure(static_cast<size_t>(n) * 2); t->d_tri_b.ensure(n); t->d_tri_color.ensure(n);
    if (edges) t->d_tri_n.ensure(static_cast<size_t>(n) * 3);
    HIP_CHECK(hipMemcpyAsync(verts.get(), hostData, count * sizeof(float4), hipMemcpyHostToDevice, t->main_stream()));
    HIP_CHECK(rtk::launch_prep_triangles(t->fma, edges, verts.get(), n, t->d_tri.get(), t->d_tri_b.get(),
                                         t->d_tri_color.get(), t->d_tri_n.get(), t->main_stream()));
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    t->queries.scene_rows.assign(&hostData[0].x, &hostData[0].x + count * 4u);    // what the signed queries weld their table from
    t->queries.scene_rows_edges = edges;
    t->n_tris = n;
    t->scene_generation++;
  });
}

int rt_tracer_upload_scene(rt_tracer* t, const rt_float4* hostData, size_t count) {
  return upload_scene_impl(t, hostData, count, false);
}

int rt_tracer_upload_scene_edges(rt_tracer* t, const rt_float4* hostData, size_t count) {
  return upload_scene_impl(t, hostData, count, true);
}

// Corrected form of the reference's experimental normal packing (UnitTests/NormalPackingTest.cpp:10-23,
// Documentation/gpu.meshes.txt:20-33): three 8-bit components in the 24-bit fraction of one float.
float rt_pack_normal(const float n[3]) {
  return floorf(n[0] * 127.0f + 127.5f) / 256.0f + floorf(n[1] * 127.0f + 127.5f) / 65536.0f +
         floorf(n[2] * 127.0f + 127.5f) / 16777216.0f;
}

void rt_unpack_normal(float packed, float n[3]) {
  // byte k sits at bits 2^-8(k+1): shift by 1, 256, 65536 (the reference's test multiplies
  // by 1, 65536, 16777216, which does not invert pack)
  const float m[3] = {1.0f, 256.0f, 65536.0f};
  for (int i = 0; i < 3; ++i) {
    const float s = packed * m[i];
    const float frac = s - floorf(s);
    n[i] = floorf(frac * 256.0f) / 127.0f - 1.0f;
  }
}

int rt_tracer_upload_spheres(rt_tracer* t, const rt_float4* spheres, size_t count) {
  if (!t || (count && !spheres)) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {
    int rc = guarded(t, [&] { t->cancel_and_join(); multi_sync_all(t); });
    for (rt_tracer* b : t->mg->bands) {
      if (rc != RT_OK) break;
      rc = rt_tracer_upload_spheres(b, spheres, count);
      if (rc != RT_OK) t->set_error(b->last_error);
    }
    if (rc == RT_OK) t->n_spheres = static_cast<uint32_t>(count);
    return rc;
  }
  return guarded(t, [&] {
    t->cancel_and_join();
    t->use_device();
    t->settle();
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    t->wait_queries();
    t->d_spheres.reset();
    t->n_spheres = 0;
    if (count == 0) return;
    t->d_spheres.ensure(count);
    HIP_CHECK(hipMemcpy(t->d_spheres.get(), spheres, count * sizeof(float4), hipMemcpyHostToDevice));
    t->n_spheres = static_cast<uint32_t>(count);
  });
}

void rt_tracer_set_update_callback(rt_tracer* t, rt_callback_fn fn, void* user) {     // :179-182
  if (!t) return;
  std::lock_guard<std::mutex> lk(t->state_mu);
  t->update_cb = fn; t->update_user = user;
}

void rt_tracer_set_finished_callback(rt_tracer* t, rt_callback_fn fn, void* user) {   // :184-187
  if (!t) return;
  std::lock_guard<std::mutex> lk(t->state_mu);
  t->finished_cb = fn; t->finished_user = user;
}

int rt_tracer_set_seed(rt_tracer* t, uint64_t seed) {
  if (!t) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    t->seed = seed;
    if (t->mg) {
      t->mg->opt.seed = seed;
      for (rt_tracer* b : t->mg->bands)
        if (rt_tracer_set_seed(b, seed) != RT_OK) throw HipFail{b->last_error};
      return;
    }
    t->use_device();
    t->create_states();
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
  });
}

// one device-resident Trace pass on any kind of handle (api_mu held, render thread idle)
static void trace_enqueue_once(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration) {
  if (t->mg) { multi_trace_enqueue(t, iterationCount, samplesPerIteration); return; }
  if (t->grp) {                                                          // member of a multi-process group: trace, then the gather
    const size_t k = member_band_index(t);
    const int b = t->grp->begin_frame();
    t->trace_enqueue_body(iterationCount, samplesPerIteration, t->grp->tile_target(k, b));
    t->grp->tile_written(k);
    t->grp->gather(b);
    return;
  }
  t->trace_enqueue_body(iterationCount, samplesPerIteration, t->image_mirror);
}

int rt_tracer_trace_enqueue(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration) {
  return rt_tracer_trace_enqueue_n(t, iterationCount, samplesPerIteration, 1u);
}

int rt_tracer_trace_enqueue_n(rt_tracer* t, uint32_t iterationCount, uint32_t samplesPerIteration, uint32_t n_steps) {
  if (!t) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    for (uint32_t s = 0; s < n_steps; ++s) trace_enqueue_once(t, iterationCount, samplesPerIteration);
  });
}

int rt_tracer_set_list_reuse(rt_tracer* t, int across_traces) {
  if (!t) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  t->cancel_and_join();
  if (t->mg) for (rt_tracer* b : t->mg->bands) (void)rt_tracer_set_list_reuse(b, across_traces);
  t->reuse_across_traces = across_traces != 0;
  if (!t->mg) (void)guarded(t, [&] { t->use_device(); t->settle(); });   // (the lists stay in their slots; the next launch rebuilds them)
  t->lists.key.reset();
  return RT_OK;
}

int rt_tracer_set_image_mirror(rt_tracer* t, void* device_visible_image) {
  if (!t) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg || t->grp) { t->set_error("rt_tracer_set_image_mirror: the gather owns the second image target of a sharded frame"); return RT_ERR_STATE; }
  t->image_mirror = static_cast<uint32_t*>(device_visible_image);
  return RT_OK;
}

int rt_tracer_fused_iterations(rt_tracer* t, uint32_t samples) {
  if (t && t->mg) return static_cast<int>(t->mg->bands[0]->fused_iterations(samples));
  return t ? static_cast<int>(t->fused_iterations(samples)) : 0;
}

// one launch of rt_tracer_launch / rt_tracer_launch_iterations on any kind of handle
static void launch_impl(rt_tracer* t, uint32_t samples, uint32_t iterations, bool clear_first, bool emit) {
  if (t->mg) { multi_launch(t, samples, iterations, clear_first, emit); return; }
  t->use_device();
  const uint32_t flags = (clear_first ? rtk::TRACE_ZERO_ACC : 0u) | (emit ? rtk::TRACE_EMIT_IMAGE : 0u);
  if (t->grp && emit) {                                                  // member of a multi-process group: the tile travels
    const size_t k = member_band_index(t);
    const int b = t->grp->begin_frame();
    t->enqueue_trace_launch(samples, flags, 0, iterations, t->grp->tile_target(k, b));
    t->grp->tile_written(k);
    t->grp->gather(b);
    return;
  }
  t->enqueue_trace_launch(samples, flags, 0, iterations, emit ? t->image_mirror : nullptr);
}

int rt_tracer_launch_iterations(rt_tracer* t, uint32_t samples, uint32_t iterations, int clear_first, int emit_image) {
  if (!t || iterations == 0u) return RT_ERR_INVALID;
  if (iterations > static_cast<uint32_t>(rt_tracer_fused_iterations(t, samples))) {
    t->set_error(fmt("rt_tracer_launch_iterations: %u iterations of %u samples exceed rt_tracer_fused_iterations", iterations, samples));
    return RT_ERR_INVALID;
  }
  return exclusive(t, [&] { launch_impl(t, samples, iterations, clear_first != 0, emit_image != 0); });
}

int rt_tracer_launch(rt_tracer* t, uint32_t samples, int clear_first, int emit_image) {
  return rt_tracer_launch_iterations(t, samples, 1u, clear_first, emit_image);
}

int rt_tracer_trace_stats(rt_tracer* t, uint32_t samples, uint64_t out[16]) {
  if (!t || !out) return RT_ERR_INVALID;
  std::lock_guard<std::mutex> lk(t->api_mu);
  if (t->mg) {                                                           // sums over the bands
    memset(out, 0, 16 * sizeof(uint64_t));
    t->cancel_and_join();
    multi_push_camera(t);
    for (rt_tracer* b : t->mg->bands) {
      uint64_t part[16];
      const int rc = rt_tracer_trace_stats(b, samples, part);
      if (rc != RT_OK) { t->set_error(b->last_error); return rc; }
      for (int i = 0; i < 16; ++i) out[i] += part[i];
    }
    return RT_OK;
  }
  return guarded(t, [&] {
    t->cancel_and_join();
    t->use_device();
    DevArray<unsigned long long> counters(16);
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, 16 * sizeof(unsigned long long), t->main_stream()));
    t->clear_accumulators();
    rtk::TraceParams p = t->params(samples);
    p.stats = counters.get();
    p.flags = t->mode_flags(p);
    t->launch_instrumented(p, samples);
    HIP_CHECK(hipMemcpy(out, counters.get(), 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  });
}

int rt_tracer_sync(rt_tracer* t) {
  if (!t) return RT_ERR_INVALID;
  if (t->mg) return guarded(t, [&] { multi_sync_all(t); });
  return guarded(t, [&] {
    t->use_device();
    t->sync_all();
    if (t->grp) t->grp->sync();
  });
}

int rt_tracer_kernel_time(rt_tracer* t, double* total_ms, uint64_t* launches, int reset_after) {
  return read_clock(t, false, total_ms, launches, reset_after);
}
int rt_tracer_launch_time(rt_tracer* t, double* total_ms, uint64_t* launches, int reset_after) {
  return read_clock(t, true, total_ms, launches, reset_after);
}

size_t rt_tracer_buffer_bytes(rt_tracer* t, int which) { return t ? buffer_bytes(t, which) : 0; }
void* rt_tracer_device_pointer(rt_tracer* t, int which) {
  if (!t) return nullptr;
  // plane 0 of the RNG states / the counts as of this call, filled on the primary stream (rt_tracer::materialise)
  if (!t->mg && (which == RT_BUF_RNG || which == RT_BUF_COUNTS) &&
      guarded(t, [&] { t->use_device(); t->materialise(which); }) != RT_OK) return nullptr;
  return buffer_ptr(t, which);
}

int rt_tracer_read_buffer(rt_tracer* t, int which, void* dst, size_t bytes) {
  if (!t || !dst) return RT_ERR_INVALID;
  if (t->mg) {
    if (bytes > buffer_bytes(t, which) || buffer_bytes(t, which) == 0) return RT_ERR_INVALID;
    return guarded(t, [&] { multi_read_buffer(t, which, dst, bytes); });
  }
  if (buffer_ptr(t, which) == nullptr || bytes > buffer_bytes(t, which)) return RT_ERR_INVALID;
  return guarded(t, [&] {
    t->use_device();
    t->materialise(which);
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    if (t->grp) t->grp->sync();
    HIP_CHECK(hipMemcpy(dst, buffer_ptr(t, which), bytes, hipMemcpyDeviceToHost));
  });
}

int rt_tracer_copy_buffer_to_device(rt_tracer* t, int which, void* dst_device, size_t bytes) {
  if (!t || !dst_device || buffer_ptr(t, which) == nullptr || bytes > buffer_bytes(t, which)) return RT_ERR_INVALID;
  if (t->mg) return guarded(t, [&] {                                      // the gathered frame, from the root device
    multi_sync_all(t);
    HIP_CHECK(hipSetDevice(t->mg->group.local[0].device));
    HIP_CHECK(hipMemcpy(dst_device, buffer_ptr(t, which), bytes, hipMemcpyDeviceToDevice));
  });
  return guarded(t, [&] {
    t->use_device();
    if (t->grp && which == RT_BUF_FRAME) t->grp->sync();
    t->materialise(which);
    HIP_CHECK(hipMemcpyAsync(dst_device, buffer_ptr(t, which), bytes, hipMemcpyDeviceToDevice, t->main_stream()));
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
  });
}

int rt_tracer_copy_buffer_to_device_async(rt_tracer* t, int which, void* dst_device, size_t bytes) {
  if (!t || !dst_device || buffer_ptr(t, which) == nullptr || bytes > buffer_bytes(t, which)) return RT_ERR_INVALID;
  if (t->mg || which == RT_BUF_FRAME) { t->set_error("rt_tracer_copy_buffer_to_device_async: per-stream copies are for plain tracers' own buffers"); return RT_ERR_STATE; }
  return guarded(t, [&] {
    t->use_device();
    t->materialise(which);
    HIP_CHECK(hipMemcpyAsync(dst_device, buffer_ptr(t, which), bytes, hipMemcpyDeviceToDevice, t->main_stream()));
  });
}

void* rt_tracer_stream(rt_tracer* t) { return (t && !t->mg) ? static_cast<void*>(t->stream) : nullptr; }
void* rt_tracer_stream_b(rt_tracer* t) { return (t && !t->mg) ? static_cast<void*>(t->stream_b) : nullptr; }

int rt_tracer_info(rt_tracer* t, uint32_t out[8]) {
  if (!t || !out) return RT_ERR_INVALID;
  if (t->mg) {                                                           // launch geometry of the first band, sizes of the frame
    (void)rt_tracer_info(t->mg->bands[0], out);
    out[3] = (t->W + 31) / 32; out[4] = (t->H + 7) / 8;
    out[7] = static_cast<uint32_t>(t->device);
    return RT_OK;
  }
  out[0] = t->last_k; out[1] = t->last_chunk; out[2] = t->last_lds;
  out[3] = (t->W + 31) / 32; out[4] = (t->rows + 7) / 8;
  out[5] = t->n_tris; out[6] = t->n_spheres; out[7] = static_cast<uint32_t>(t->device);
  return RT_OK;
}

// ---- a frame sharded over several GPUs ------------------------------------------------------

int rt_tracer_create_multi(const uint32_t imageSize[2], const float cameraPosition[3], const float cameraAngles[2],
                           float fov, float focalLength, float aperture, const rt_options* options,
                           const int32_t* devices, uint32_t n_bands, rt_tracer** out) {
  return multi_create(imageSize, cameraPosition, cameraAngles, fov, focalLength, aperture, options, devices, n_bands, out);
}

int rt_group_unique_id(uint8_t id[RT_GROUP_ID_BYTES]) {
  if (!id) return RT_ERR_INVALID;
  return guarded(nullptr, [&] {
    ncclUniqueId uid;
    RCCL_CHECK(need_rccl().GetUniqueId(&uid));
    memcpy(id, uid.internal, RT_GROUP_ID_BYTES);
  });
}

static int join_impl(rt_tracer* t, uint32_t n_ranks, uint32_t rank, const uint8_t id[RT_GROUP_ID_BYTES], const uint32_t* row_begin) {
  if (!t || t->mg || n_ranks == 0u || rank >= n_ranks || (!id && n_ranks > 1u)) return RT_ERR_INVALID;
  static const uint8_t zero_id[RT_GROUP_ID_BYTES] = {0};
  return exclusive(t, [&] {
    member_join(t, n_ranks, rank, id ? id : zero_id, row_begin);
  });
}

int rt_tracer_join_group(rt_tracer* t, uint32_t n_ranks, uint32_t rank, const uint8_t id[RT_GROUP_ID_BYTES]) {
  return join_impl(t, n_ranks, rank, id, nullptr);                      // equal bands
}

int rt_tracer_join_group_bands(rt_tracer* t, uint32_t n_ranks, uint32_t rank, const uint8_t id[RT_GROUP_ID_BYTES],
                               const uint32_t* row_begin) {
  return row_begin ? join_impl(t, n_ranks, rank, id, row_begin) : RT_ERR_INVALID;
}

int rt_balance_rows(uint32_t n_bands, const uint32_t* row_begin, const double* cost, uint32_t granule, uint32_t* new_row_begin) {
  if (n_bands == 0u || !row_begin || !cost || !new_row_begin) return RT_ERR_INVALID;
  for (uint32_t k = 0; k < n_bands; ++k) if (row_begin[k + 1] <= row_begin[k]) return RT_ERR_INVALID;
  balance_rows(n_bands, row_begin, cost, granule, new_row_begin);
  return RT_OK;
}

int rt_tracer_set_band(rt_tracer* t, uint32_t row_begin, uint32_t rows) {
  if (!t || t->mg || rows == 0u) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    if (t->grp) throw HipFail{"rt_tracer_set_band: leave the group first"};
    if (!t->band_mode) throw HipFail{"rt_tracer_set_band: the tracer owns a whole image, not a band (rt_options.full_height)"};
    if (static_cast<uint64_t>(row_begin) + rows > t->H) throw HipFail{"row band exceeds full_height"};
    t->use_device();
    t->reshape(t->W, t->H, row_begin, rows);
  });
}

int rt_tracer_rebalance(rt_tracer* t) {
  if (!t || !t->mg) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    multi_sync_all(t);
    MultiState& m = *t->mg;
    const uint32_t n = static_cast<uint32_t>(m.bands.size());
    std::vector<uint32_t> begins(n + 1u), fresh(n + 1u);
    std::vector<double> cost(n);
    for (uint32_t k = 0; k < n; ++k) {
      begins[k] = m.group.bands[k].row0;
      cost[k] = m.bands[k]->clock.span_per_launch();
    }
    begins[n] = t->H;
    for (uint32_t k = 0; k < n; ++k) if (!(cost[k] > 0.0)) throw HipFail{"rt_tracer_rebalance: no timed launch on every band yet"};
    balance_rows(n, begins.data(), cost.data(), 8u, fresh.data());
    if (fresh == begins) return;
    multi_resize(t, t->W, t->H, fresh.data());
  });
}

int rt_tracer_leave_group(rt_tracer* t) {
  if (!t || t->mg) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    member_leave(t);
  });
}

int rt_tracer_gather_time(rt_tracer* t, double* total_ms, uint64_t* gathers, int reset_after) {
  if (!t) return RT_ERR_INVALID;
  Group* g = t->mg ? &t->mg->group : t->grp;
  if (total_ms) *total_ms = 0.0;
  if (gathers) *gathers = 0u;
  if (g) g->read_time(total_ms, gathers, reset_after != 0);
  return RT_OK;
}

int rt_tracer_gather_only(rt_tracer* t) {
  if (!t || (!t->mg && !t->grp)) return RT_ERR_INVALID;
  return exclusive(t, [&] {
    group_gather_only(t);
  });
}

int rt_tracer_group_info(rt_tracer* t, char* json, size_t capacity) {
  if (!t || !json || capacity == 0) return RT_ERR_INVALID;
  const std::string s = group_info_json(t);
  if (s.size() + 1 > capacity) return RT_ERR_INVALID;
  memcpy(json, s.c_str(), s.size() + 1);
  return RT_OK;
}

int rt_tracer_band_count(rt_tracer* t) {
  if (!t) return 0;
  return t->mg ? static_cast<int>(t->mg->bands.size()) : 1;
}

int rt_tracer_band_info(rt_tracer* t, uint32_t band, uint32_t out[4]) {
  if (!t || !out) return RT_ERR_INVALID;
  if (t->mg) {
    if (band >= t->mg->bands.size()) return RT_ERR_INVALID;
    const GroupBand& b = t->mg->group.bands[band];
    out[0] = static_cast<uint32_t>(t->mg->band_device[band]); out[1] = b.row0; out[2] = b.rows; out[3] = static_cast<uint32_t>(b.rank);
    return RT_OK;
  }
  if (band != 0u) return RT_ERR_INVALID;
  out[0] = static_cast<uint32_t>(t->device); out[1] = t->row0; out[2] = t->rows;
  out[3] = t->grp ? static_cast<uint32_t>(t->grp->local[0].rank) : 0u;
  return RT_OK;
}

}  // extern "C"

#include "rt_query_api.hpp"
