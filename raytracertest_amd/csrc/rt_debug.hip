// rt_debug.hip -- the rt_dbg_* entry points of include/rt_mi355x.h: single-function device harnesses and read-outs of a
// tracer's internal state (measurement aids and tests).
#include "rt_tracer.hpp"

using namespace rtr;

// a harness on a bare device: selected first; failures go to the process's error text
template <class F>
static int on_device(int device, F&& f) {
  const int rc = require_device(device);
  if (rc != RT_OK) return rc;
  return guarded(nullptr, [&] { HIP_CHECK(hipSetDevice(device)); f(); });
}

// a read-out of a plain tracer: exclusive, on its device
template <class F>
static int on_tracer(rt_tracer* t, F&& f) { return exclusive(t, [&] { t->use_device(); f(); }); }

extern "C" {

int rt_dbg_hit_triangle(int device, uint32_t math_mode, uint32_t n, const float* rays, const float* tris,
                        int eps_mode, int32_t* hit, float* tuv, float* normal, float* point) {
  return on_device(device, [&] {
    DevArray<float> dr(n * 6), dt(n * 9), duv(n * 3), dn(n * 3), dp(n * 3);
    DevArray<int> dh(n);
    HIP_CHECK(hipMemcpy(dr.get(), rays, n * 6 * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dt.get(), tris, n * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(rtk::launch_dbg_hit_triangle(math_mode != RT_MATH_STRICT, n, dr.get(), dt.get(), eps_mode, dh.get(), duv.get(),
                                           dn.get(), dp.get(), nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(hit, dh.get(), n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(tuv, duv.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(normal, dn.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(point, dp.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_check_midrange(int device, uint64_t out[4]) {
  if (!out) return RT_ERR_INVALID;
  return on_device(device, [&] {
    DevArray<unsigned long long> d(4);
    HIP_CHECK(hipMemset(d.get(), 0, 4 * sizeof(unsigned long long)));
    HIP_CHECK(rtk::launch_dbg_check_midrange(d.get(), nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d.get(), 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_valu_peak(int device, double* lane_fma_per_s, double* clock_ghz) {
  return on_device(device, [&] {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    const uint32_t blocks = static_cast<uint32_t>(prop.multiProcessorCount) * 8u;   // 8 waves per SIMD
    const int iters = 20000;
    DevArray<float> out(static_cast<size_t>(blocks) * 256);
    DevArray<unsigned long long> clk(2);
    const Event e0 = Event::timing(), e1 = Event::timing();
    HIP_CHECK(rtk::launch_dbg_valu_peak(blocks, iters, out.get(), clk.get(), nullptr));
    HIP_CHECK(hipEventRecord(e0, nullptr));
    HIP_CHECK(rtk::launch_dbg_valu_peak(blocks, iters, out.get(), clk.get(), nullptr));
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long c[2];
    HIP_CHECK(hipMemcpy(c, clk.get(), sizeof c, hipMemcpyDeviceToHost));
    if (lane_fma_per_s) *lane_fma_per_s = static_cast<double>(blocks) * 256.0 * iters * 8.0 / (ms * 1e-3);
    if (clock_ghz) *clock_ghz = c[1] ? static_cast<double>(c[0]) / static_cast<double>(c[1]) * 0.1 : 0.0;
  });
}

#ifdef RT_TIMELINE
// experiment builds only (make EXTRA=-DRT_TIMELINE): one launch with per-wave timestamps
int rt_dbg_trace_timeline(rt_tracer* t, uint32_t samples, unsigned long long* out, size_t capacity_words) {
  if (!t || !out) return RT_ERR_INVALID;
  return on_tracer(t, [&] {
    const size_t words = static_cast<size_t>((t->W + 31u) / 32u) * ((t->rows + 7u) / 8u) * 4u * 16u;
    if (words > capacity_words) throw HipFail{fmt("timeline needs %zu words", words)};
    DevArray<unsigned long long> buf(words);
    HIP_CHECK(hipMemsetAsync(buf.get(), 0, words * sizeof(unsigned long long), t->main_stream()));
    rtk::TraceParams p = t->params(samples);
    p.flags = rtk::TRACE_ZERO_ACC | rtk::TRACE_EMIT_IMAGE | t->mode_flags(p);
    p.image = t->d_image.get();
    p.timeline = buf.get();
    t->launch_instrumented(p, samples);
    HIP_CHECK(hipMemcpy(out, buf.get(), words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  });
}
#endif

// the stored tile candidate lists of a small-scene tracer, as the last storing launch wrote them: per wave tile
// (grid order, 4 per 32x8 block) 1 + bin_list words; word 0 = count | winner << 10 | certain << 31.  Measurement aid.
int rt_dbg_read_tile_lists(rt_tracer* t, uint32_t* dst, size_t capacity_words, uint32_t* words_per_tile) {
  if (!t || t->mg || !dst) return RT_ERR_INVALID;
  return on_tracer(t, [&] {
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    t->sync_list_stream();
    if (!t->lists.now() || !t->lists.key) throw HipFail{"no tile lists (small scenes build them ahead of their first trace launch)"};
    const size_t n = t->lists.words() < capacity_words ? t->lists.words() : capacity_words;
    HIP_CHECK(hipMemcpy(dst, t->lists.now(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (words_per_tile) *words_per_tile = 1u + t->lists.key->bin_list;
  });
}

// dense scenes: the header words (candidate count, 0xFFFFFFFF = overflow) of the tiles' lists in HBM as the last launch left
// them -- half 0 = the unsplit launch or the upper half of a split one, half 1 = the lower half.  Measurement aid / tests.
int rt_dbg_wave_list_counts(rt_tracer* t, int half, uint32_t* dst, size_t capacity_tiles, uint32_t* n_tiles, uint32_t* capacity_per_tile) {
  if (!t || t->mg || !dst || half < 0 || half > 1) return RT_ERR_INVALID;
  return on_tracer(t, [&] {
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    const HalfLists& h = t->half_lists[half];
    if (!h.wave.get() || !h.wave_valid) throw HipFail{"no wave lists (dense scenes build them ahead of their first trace launch)"};
    const size_t n = h.wave_tiles < capacity_tiles ? h.wave_tiles : capacity_tiles;   // (what the lists were built with)
    HIP_CHECK(hipMemcpy2D(dst, sizeof(uint32_t), h.wave.get(), static_cast<size_t>(1u + h.wave_cap) * 64u, sizeof(uint32_t), n, hipMemcpyDeviceToHost));
    if (n_tiles) *n_tiles = static_cast<uint32_t>(h.wave_tiles);
    if (capacity_per_tile) *capacity_per_tile = h.wave_cap;
  });
}

int rt_dbg_trace_occupancy(int device, int samples_in_flight, uint32_t lds_bytes) {
  if (require_device(device) != RT_OK) return -1;
  if (hipSetDevice(device) != hipSuccess) return -1;
  return rtk::trace_occupancy(samples_in_flight, lds_bytes);
}

int rt_dbg_sincos(int device, uint32_t n, const float* x, float* s, float* c) {
  return on_device(device, [&] {
    DevArray<float> dx(n), ds(n), dc(n);
    HIP_CHECK(hipMemcpy(dx.get(), x, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(rtk::launch_dbg_sincos(n, dx.get(), ds.get(), dc.get(), nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(s, ds.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(c, dc.get(), n * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_uniform(int device, uint32_t n, uint32_t m, uint32_t* states, float* out) {
  return on_device(device, [&] {
    DevArray<uint32_t> ds(n * 6);
    DevArray<float> dout(static_cast<size_t>(n) * m);
    HIP_CHECK(hipMemcpy(ds.get(), states, n * 6 * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_CHECK(rtk::launch_dbg_uniform(n, m, ds.get(), dout.get(), nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(states, ds.get(), n * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out, dout.get(), static_cast<size_t>(n) * m * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_get_ray(rt_tracer* t, uint32_t n, const uint32_t* pixels, uint32_t* states, float* rays) {
  if (!t) return RT_ERR_INVALID;
  if (t->mg) { multi_push_camera(t); return rt_dbg_get_ray(t->mg->bands[0], n, pixels, states, rays); }   // the camera of the whole frame
  return guarded(t, [&] {
    t->use_device();
    rtk::TraceParams p = t->params(1);
    DevArray<uint32_t> dpix(n * 2), ds(n * 6);
    DevArray<float> dr(n * 6);
    HIP_CHECK(hipMemcpy(dpix.get(), pixels, n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ds.get(), states, n * 6 * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_CHECK(rtk::launch_dbg_get_ray(t->fma, p, n, dpix.get(), ds.get(), dr.get(), t->main_stream()));
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    HIP_CHECK(hipMemcpy(states, ds.get(), n * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(rays, dr.get(), n * 6 * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_focal_boxes(rt_tracer* t, float curv_scale, float* boxes, size_t boxes_capacity, float* focal, size_t focal_capacity) {
  if (!t || t->mg || !boxes || !focal) return RT_ERR_INVALID;
  return on_tracer(t, [&] {
    rtk::TraceParams p = t->params(1);
    if (p.tile_curv > 0.0f) p.tile_curv = std::max(p.tile_curv * curv_scale, 1e-30f);   // this launch only; the corner path stays on (the test's teeth: 0 must fail)
    const size_t tiles = static_cast<size_t>((t->W + 31u) / 32u) * ((t->rows + 7u) / 8u) * 4u;
    const size_t nb = tiles * 8u, nf = static_cast<size_t>(t->npix()) * 3u;
    if (nb > boxes_capacity || nf > focal_capacity) throw HipFail{fmt("focal boxes need %zu + %zu floats", nb, nf)};
    DevArray<float> db(nb), df(nf);
    HIP_CHECK(hipMemsetAsync(db.get(), 0, nb * sizeof(float), t->main_stream()));
    HIP_CHECK(rtk::launch_dbg_focal_boxes(t->fma, p, db.get(), df.get(), t->main_stream()));
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    HIP_CHECK(hipMemcpy(boxes, db.get(), nb * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(focal, df.get(), nf * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rt_dbg_classify(rt_tracer* t, uint32_t level, uint32_t forms, uint32_t slack_milli, const uint32_t* regions, uint32_t n_regions,
                    float* out, size_t capacity_floats) {
  if (!t || t->mg || !regions || !out || level > 4u) return RT_ERR_INVALID;
  return on_tracer(t, [&] {
    rtk::TraceParams p = t->params(1);
    p.macro_w = rt_tracer::kMacroW; p.macro_h = rt_tracer::kMacroH;      // level 2: the macro tile of attach_macro_lists
    p.super_f = rt_tracer::kSuperF;                                       // level 4: the super tile above it
    const uint32_t rw = level == 0u ? 8u : level == 2u ? p.macro_w : level == 4u ? p.macro_w * p.super_f : 32u;
    const uint32_t rh = level == 2u ? p.macro_h : level == 4u ? p.macro_h * p.super_f : level == 3u ? 16u : 8u;
    for (uint32_t i = 0; i < n_regions; ++i)                             // the kernel's pixel <-> lane mapping assumes the trace grid
      if (regions[2u * i] % rw != 0u || regions[2u * i + 1u] % rh != 0u || regions[2u * i] >= t->W || regions[2u * i + 1u] >= t->rows)
        throw HipFail{fmt("region %u (%u, %u) is not a level-%u region of the %ux%u band", i, regions[2u * i], regions[2u * i + 1u], level, t->W, t->rows)};
    const size_t per = 16u + static_cast<size_t>(t->n_tris) * (forms ? 32u : 12u);
    if (per * n_regions > capacity_floats) throw HipFail{fmt("rt_dbg_classify needs %zu floats", per * n_regions)};
    DevArray<uint32_t> dr(static_cast<size_t>(n_regions) * 2u);
    DevArray<float> dout(per * n_regions);
    HIP_CHECK(hipMemcpyAsync(dr.get(), regions, static_cast<size_t>(n_regions) * 2u * sizeof(uint32_t), hipMemcpyHostToDevice, t->main_stream()));
    HIP_CHECK(rtk::launch_dbg_classify(t->fma, forms != 0u, slack_milli, p, level, n_regions, dr.get(), dout.get(), t->main_stream()));
    HIP_CHECK(hipStreamSynchronize(t->main_stream()));
    HIP_CHECK(hipMemcpy(out, dout.get(), per * n_regions * sizeof(float), hipMemcpyDeviceToHost));
  });
}

void rt_dbg_rng_init_host(uint64_t seed, uint64_t subsequence, uint32_t state[6]) {
  rth::init_state(jump_host(), seed, subsequence & 0xffffffffull, state);
}


// count states of v0..v4 advanced by n draws on the host: through the 4-bit window table of T^n (what rng_settle_kernel
// does with it; built once per call) or by n single steps (all states in lockstep: the loop vectorises).  No device needed.
void rt_dbg_rng_advance_host_n(uint32_t* states, uint32_t count, uint32_t n, int use_table) {
  if (use_table) {
    const std::vector<uint32_t> table = rth::build_window_table(rth::step_power(n));
    for (uint32_t i = 0; i < count; ++i) rth::window_product(table, states + 5u * i, states + 5u * i);
    return;
  }
  constexpr uint32_t kLanes = 64;
  for (uint32_t base = 0; base < count; base += kLanes) {
    const uint32_t m = count - base < kLanes ? count - base : kLanes;
    uint32_t v[5][kLanes] = {};
    for (uint32_t i = 0; i < m; ++i) for (int w = 0; w < 5; ++w) v[w][i] = states[5u * (base + i) + w];
    auto f = [](uint32_t x, uint32_t y) -> uint32_t { const uint32_t t = x ^ (x >> 2); return (y ^ (y << 4)) ^ (t ^ (t << 1)); };
    uint32_t k = 0;
    for (; k + 5u <= n; k += 5u)                                        // five draws rotate the words once: in place (rtd::rng_discard)
      for (uint32_t i = 0; i < kLanes; ++i) {
        v[0][i] = f(v[0][i], v[4][i]); v[1][i] = f(v[1][i], v[0][i]); v[2][i] = f(v[2][i], v[1][i]);
        v[3][i] = f(v[3][i], v[2][i]); v[4][i] = f(v[4][i], v[3][i]);
      }
    for (uint32_t i = 0; i < m; ++i) {
      uint32_t one[5] = {v[0][i], v[1][i], v[2][i], v[3][i], v[4][i]};
      for (uint32_t r = k; r < n; ++r) rth::xorshift_step(one);
      memcpy(states + 5u * (base + i), one, sizeof one);
    }
  }
}
void rt_dbg_rng_advance_host(uint32_t state[5], uint32_t n, int use_table) { rt_dbg_rng_advance_host_n(state, 1u, n, use_table); }

// out = {owed draws, owing launches since the last settle, settle kernels enqueued so far, device tables held}
int rt_dbg_owed_state(rt_tracer* t, uint64_t out[4]) {
  if (!t || t->mg || !out) return RT_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lk(t->order_mu);
  out[0] = t->debt.owed_draws; out[1] = t->debt.owing_launches; out[2] = t->debt.settles_enqueued; out[3] = t->debt.settle_tables.size();
  return RT_OK;
}

// out = {launches (steps) enqueued, kernel launches, event records, stream waits, list_ready records, list_free records,
// events carried by a kernel as its stop event, 0} of the enqueue path since the last call; reading clears them
int rt_dbg_enqueue_calls(rt_tracer* t, uint64_t out[8]) {
  if (!t || t->mg || !out) return RT_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lk(t->order_mu);
  const rtr::EnqueueCalls& c = t->calls;
  out[0] = c.steps; out[1] = c.launches; out[2] = c.records; out[3] = c.waits; out[4] = c.ready_records; out[5] = c.free_records;
  out[6] = c.stop_events; out[7] = 0;
  t->calls = rtr::EnqueueCalls{};
  return RT_OK;
}

// out[kind] = list builds of a small scene by the builder launched (rtk::launch_tile_lists: 0 region pairs, 1 regions, 2 tiles of
// up to 32 triangles, 3 tiles) since the tracer was created; reading changes nothing
int rt_dbg_list_builds(rt_tracer* t, uint64_t out[4]) {
  if (!t || t->mg || !out) return RT_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lk(t->order_mu);
  for (int k = 0; k < 4; ++k) out[k] = t->list_builds[k];
  return RT_OK;
}

}  // extern "C"
