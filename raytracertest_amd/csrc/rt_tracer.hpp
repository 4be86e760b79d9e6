// rt_tracer.hpp -- struct rt_tracer, the host runtime behind the C ABI of include/rt_mi355x.h, and the types it is made of.
//
// Mirrors rt::RayTracerImpl (RayTracer/RayTracerImpl.cuh:17-75, RayTracerImpl.cu): owns the
// device buffers, the RNG states, the scene, the camera, the render std::thread, launches
// the kernels and fires the callbacks.  HIP streams/events, pinned host image for the
// callbacks (the PBO interop is cut), no CPU fallback: without a HIP device creation fails.
// Included by rt_tracer.hip (the C ABI) and rt_debug.hip (the rt_dbg_* harnesses).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_device_math.hpp"
#include "rt_hip_host.hpp"
#include "rt_kernels.hpp"
#include "rt_query_state.hpp"
#include "rt_rng_host.hpp"

namespace rtr {

// The environment switches of the library, read ONCE per process: every one of them is exercised by
// a test (tests/test_gpu_*.py) -- A/B knobs of past rounds are gone, their measurements are in HISTORY.md.
struct Env {
  bool log;             // RT_MI355X_LOG=1: recorded failures and launch-shape changes go to stderr
  bool no_split;        // RT_MI355X_NO_SPLIT=1: launches as one kernel on one stream
  bool no_pretest;      // RT_MI355X_NO_PRETEST=1: no per-sample forms in the dense-scene kernels
  bool no_sure_table;   // RT_MI355X_NO_SURE_TABLE=1: certain-winner tiles add their samples' colours per pixel
  int row_interleave;   // RT_MI355X_ROW_INTERLEAVE=0|1: pins the halves of a split small-scene launch (-1: by the builder's counts)
  long macro_cap;       // RT_MI355X_MACRO_CAP=n: capacity of the macro lists (tests: forces the overflow fallback); 0 = default
  bool no_owe;          // RT_MI355X_NO_OWE=1: certain-winner tiles advance their RNG states in every launch (no owed draws)
  long owe_period;      // RT_MI355X_OWE_PERIOD=n: owing launches between two periodic settles (tests); 0 = RT_OWE_PERIOD
  static bool on(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
  Env() {
    log = getenv("RT_MI355X_LOG") != nullptr;
    no_split = on("RT_MI355X_NO_SPLIT");
    no_pretest = on("RT_MI355X_NO_PRETEST");
    no_sure_table = on("RT_MI355X_NO_SURE_TABLE");
    const char* ri = getenv("RT_MI355X_ROW_INTERLEAVE");
    row_interleave = (ri && (ri[0] == '0' || ri[0] == '1') && ri[1] == 0) ? ri[0] - '0' : -1;
    const char* mc = getenv("RT_MI355X_MACRO_CAP");
    macro_cap = mc ? strtol(mc, nullptr, 10) : 0;
    no_owe = on("RT_MI355X_NO_OWE");
    const char* op = getenv("RT_MI355X_OWE_PERIOD");
    owe_period = op ? strtol(op, nullptr, 10) : 0;
  }
};

void set_global_error(const std::string& s);

// jump table: built once per process, uploaded once per device (rt_tracer.hip)
const std::vector<uint32_t>& jump_host();
uint32_t* jump_device(int device);        // the jump table followed by the window tables
constexpr size_t kJumpWords = 32u * 160u * 8u;

// ThinLensCamera host side, ThinLensCamera.cuh:16-28,79-108,132-141 (host code: no fusing)
struct Camera {
  float position[3];   // mPosition: stored, never used (reference quirk Q1)
  float angles[2];     // mRotationAngles, radians
  float fov;           // mFov, radians
  float focal, aperture;
  float M[16];         // column-major mCameraTransformation

  static float radians(float deg) { return deg * 0.01745329251994329576923690768489f; }

  void transform() {                                                     // :132-141
    float sx, cx, sy, cy;
    rtd::sincos_spec(angles[0] * 0.5f, sx, cx);                          // glm::angleAxis
    rtd::sincos_spec(angles[1] * 0.5f, sy, cy);
    const float Xw = cx, Xx = 1.0f * sx, Xy = 0.0f * sx, Xz = 0.0f * sx;  // qX
    const float Yw = cy, Yx = 0.0f * sy, Yy = 1.0f * sy, Yz = 0.0f * sy;  // qY
    const float w = Yw * Xw - Yx * Xx - Yy * Xy - Yz * Xz;                // qY * qX
    const float x = Yw * Xx + Yx * Xw + Yy * Xz - Yz * Xy;
    const float y = Yw * Xy + Yy * Xw + Yz * Xx - Yx * Xz;
    const float z = Yw * Xz + Yz * Xw + Yx * Xy - Yy * Xx;
    const float qxx = x * x, qyy = y * y, qzz = z * z, qxz = x * z, qxy = x * y, qyz = y * z;
    const float qwx = w * x, qwy = w * y, qwz = w * z;
    memset(M, 0, sizeof M);                                              // glm::mat4_cast
    M[0] = 1.0f - 2.0f * (qyy + qzz); M[1] = 2.0f * (qxy + qwz);        M[2] = 2.0f * (qxz - qwy);
    M[4] = 2.0f * (qxy - qwz);        M[5] = 1.0f - 2.0f * (qxx + qzz); M[6] = 2.0f * (qyz + qwx);
    M[8] = 2.0f * (qxz + qwy);        M[9] = 2.0f * (qyz - qwx);        M[10] = 1.0f - 2.0f * (qxx + qyy);
    M[15] = 1.0f;
  }
  float tan_half_fov() const {                                           // :114, hoisted per launch
    float s, c;
    rtd::sincos_spec(fov / 2.0f, s, c);
    return s / c;
  }
};

#ifndef RT_EVENT_STRIDE
#define RT_EVENT_STRIDE 16        // every 16th launch carries timing events (an event record costs its stream 1.4 us: stride 4 -> 16 bought 1.8 % of a C3 step)
#endif
#ifndef RT_PRETEST_LIST
#define RT_PRETEST_LIST 84u      // per-wave list capacity of the dense-scene kernels with forms: 4 x 84 x 116 bytes = 38 KiB of LDS per block (C4's fullest tile: 48)
#endif
// Timing of sampled launches and the flow control that waits on it.  Event pairs bracket every kEventStride-th launch (and
// every launch the caller waits for): an event record is a packet of its own that the next kernel has to wait behind --
// measured 5.6 us per C3 step (157.9 -> 152.3 us) and 2.3x on the 38x21 interactive loop (13.9 -> 6.0 us per iteration)
// with both events on every launch.  The mean of the sampled launches is what rt_tracer_kernel_time reports; the first
// launch after a reset is always sampled.
struct EventPair { Event a, b, c; bool split = false; uint64_t seq = 0; };   // c: end of the lower half on stream_b
class LaunchClock {
 public:
  static constexpr uint32_t kEventStride = RT_EVENT_STRIDE;
  // whether the next launch is sampled (`waited`: its caller waits for it); if so, `e` holds a recycled or a new pair
  bool start(bool waited, bool split, EventPair& e) {
    if (!waited && (counter_++ % kEventStride) != 0u) return false;
    std::lock_guard<std::mutex> lk(mu_);
    if (!free_.empty()) { e = std::move(free_.back()); free_.pop_back(); }
    else { e.a = Event::timing(); e.b = Event::timing(); e.c = Event::timing(); }   // (c timed as well: span_ms)
    e.split = split;
    return true;
  }
  // A sampled launch is enqueued.  sync_after: 0 = no waiting (what has finished meanwhile is recycled, so that a long
  // enqueue loop without rt_tracer_sync does not grow `pending_`), 1 = wait for this launch, N > 1 = flow control in units
  // of sampled launches: the launch waited for is max(kEventStride, N) launches back, i.e. fewer than N + kEventStride
  // launches are in flight.
  void enqueued(EventPair e, int sync_after) {
    hipEvent_t wait_b = nullptr, wait_c = nullptr;
    size_t back = 2;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (sync_after == 0) reap_locked();
      e.seq = next_seq_++;
      pending_.push_back(std::move(e));
      back = (static_cast<size_t>(sync_after > 1 ? sync_after : 2) + kEventStride - 1u) / kEventStride;
      if (back < 2u) back = 2u;
      const EventPair* w = sync_after == 1 ? &pending_.back()
                           : (sync_after > 1 && pending_.size() >= back) ? &pending_[pending_.size() - back] : nullptr;
      if (w) { wait_b = w->b; wait_c = w->split ? w->c : nullptr; }
    }
    if (wait_b == nullptr) return;
    HIP_CHECK(hipEventSynchronize(wait_b));                                 // RayTracerImpl.cu:228
    if (wait_c) HIP_CHECK(hipEventSynchronize(wait_c));
    if (sync_after > 1) drain(back - 1u);                                   // everything older has finished: recycle
  }
  // the event pairs of finished launches, keeping the newest `keep_last` (the caller knows they finished)
  void drain(size_t keep_last = 0) {
    std::lock_guard<std::mutex> lk(mu_);
    if (pending_.size() > keep_last) recycle_locked(pending_.size() - keep_last);
  }
  // only the pairs pushed before `seq_end` (a caller that synchronised the streams at that point: pairs the
  // render thread has pushed since may still be in flight)
  void drain_before(uint64_t seq_end) {
    std::lock_guard<std::mutex> lk(mu_);
    size_t n = 0;
    while (n < pending_.size() && pending_[n].seq < seq_end) ++n;
    recycle_locked(n);
  }
  uint64_t seq_now() { std::lock_guard<std::mutex> lk(mu_); return next_seq_; }
  // the summed kernel times (span: each launch counted to the end of the later of its halves) and the sampled launches
  void read(bool span, double* total_ms, uint64_t* launches, bool reset) {
    std::lock_guard<std::mutex> lk(mu_);
    if (total_ms) *total_ms = span ? span_ms_ : kernel_ms_;
    if (launches) *launches = launches_;
    if (reset) { kernel_ms_ = 0.0; span_ms_ = 0.0; launches_ = 0; counter_ = 0; }   // next launch is sampled
  }
  double span_per_launch() { std::lock_guard<std::mutex> lk(mu_); return launches_ ? span_ms_ / static_cast<double>(launches_) : 0.0; }
  float last_half_ms() const { return last_half_ms_.load(); }

 private:
  // account and recycle the oldest n_done pairs (their launches have finished); mu_ held
  void recycle_locked(size_t n_done) {
    for (size_t i = 0; i < n_done; ++i) {
      EventPair& e = pending_[i];
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
        kernel_ms_ += ms; launches_ += 1;
        if (e.split) last_half_ms_ = ms;
        // what the launch COST: for a split launch from the start of the upper half to the end of the later half (the
        // lower half runs on stream_b; a band whose expensive rows sit there must not look cheap to the load balancer)
        float lower = 0.0f;
        if (e.split && hipEventElapsedTime(&lower, e.a, e.c) == hipSuccess && lower > ms) ms = lower;
        span_ms_ += ms;
      }
      free_.push_back(std::move(e));
    }
    pending_.erase(pending_.begin(), pending_.begin() + static_cast<std::ptrdiff_t>(n_done));
  }
  void reap_locked() {                // oldest first, no waiting
    size_t n = 0;
    while (n < pending_.size() && hipEventQuery(pending_[n].b) == hipSuccess &&
           (!pending_[n].split || hipEventQuery(pending_[n].c) == hipSuccess)) ++n;
    (void)hipGetLastError();          // hipErrorNotReady is an answer, not a failure of the next launch
    recycle_locked(n);
  }
  std::mutex mu_;
  std::vector<EventPair> pending_, free_;
  uint64_t next_seq_ = 0;
  std::atomic<uint32_t> counter_{0};
  double kernel_ms_ = 0.0, span_ms_ = 0.0;   // span: the same sampled launches, each to the end of the later of its halves
  uint64_t launches_ = 0;
  std::atomic<float> last_half_ms_{0.0f};    // duration of the last sampled upper half-frame kernel of a split launch
};

// The render thread of a tracer.  The reference starts a std::thread per Trace and joins the previous one first
// (RayTracerImpl.cu:69-87); its only caller re-traces on every mouse-move event (OpenGLView/MainFrame.cpp:394-444), so the
// thread's start-up is part of every frame's latency.  Here ONE thread per tracer, created by the first Trace, runs the
// Traces one after the other: between two of them it polls for the next job for a short while (a drag loop's next Trace
// arrives within microseconds of the finished callback) and then parks on a condition variable.  What a caller can observe
// is unchanged: run() returns at once, the job and its callbacks run on a thread that is not the caller's, wait_idle() is
// the join.
class RenderThread {
 public:
  ~RenderThread() { shutdown(); }
  bool busy() const { return busy_.load(std::memory_order_acquire); }
  // hands `job` to the render thread; the previous job has finished (callers cancel + wait_idle() first)
  void run(std::function<void()> job) {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !busy_.load(); });
    if (!th_.joinable()) th_ = std::thread([this] { loop(); });
    job_ = std::move(job);
    busy_.store(true, std::memory_order_release);
    posted_.store(true, std::memory_order_release);
    lk.unlock();
    cv_.notify_one();
  }
  void wait_idle() {
    if (!busy()) return;
    for (int i = 0; i < 2000 && busy(); ++i) spin_pause();              // a short Trace ends within microseconds
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !busy_.load(); });
  }
  void shutdown() {
    {
      std::unique_lock<std::mutex> lk(mu_);
      done_cv_.wait(lk, [&] { return !busy_.load(); });
      quit_ = true;
    }
    cv_.notify_one();
    if (th_.joinable()) th_.join();
  }

 private:
  static void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
  }
  void loop() {
    for (;;) {
      // poll ~50 us for the next job before parking (no lock taken while polling)
      const auto t0 = std::chrono::steady_clock::now();
      while (!posted_.load(std::memory_order_acquire) &&
             std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(50)) spin_pause();
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return posted_.load() || quit_; });
        if (!posted_.load()) return;                                   // quit
        posted_.store(false);
        job = std::move(job_);
        job_ = nullptr;
      }
      job();
      {
        std::lock_guard<std::mutex> lk(mu_);
        busy_.store(false, std::memory_order_release);
      }
      done_cv_.notify_all();
    }
  }
  std::thread th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::function<void()> job_;
  std::atomic<bool> busy_{false}, posted_{false};
  bool quit_ = false;
};

// Runtime calls the enqueue path of the trace launches has issued since the last read (rt_dbg_enqueue_calls; guarded by
// rt_tracer::order_mu): kernel launches, event records, stream waits -- of the records, those of a list_ready / a list_free
// event as a call of their own -- the events kernels carried as stop events instead, and the launches (steps) enqueued.
struct EnqueueCalls {
  uint64_t steps = 0, launches = 0, records = 0, waits = 0, ready_records = 0, free_records = 0, stop_events = 0;
};

// What the stored candidate lists were built for: camera snapshot, lens, frame, list length (or macro geometry), scene and
// arithmetic mode -- they do not depend on the samples.  rt_tracer::make_key zeroes the padding: keys compare bytewise.
struct ListKey {
  float cam[12], half_height, aspect, focal, aperture;
  uint32_t W, H, row0, rows, bin_list, n_tris, scene_generation;
  bool fma;
};
inline bool same_key(const std::optional<ListKey>& held, const ListKey& k) { return held && memcmp(&*held, &k, sizeof k) == 0; }

// What has to stay the same from one small-scene launch to the next for the certain-winner tiles to be the same tiles:
// the lists' key, what the kernel's certain-winner condition reads, the trace path and the arithmetic mode (rt_tracer::
// owe_key_of zeroes the padding: compared bytewise).
struct OweKey {
  ListKey lists;
  uint32_t mode_flags, n_spheres, smooth, path;
};
#ifndef RT_OWE_PERIOD
#define RT_OWE_PERIOD 16         // owing launches between two periodic settles (<= 20: the driver's timed region then holds one)
#endif
constexpr uint32_t kSettleStepMax = 96u;   // draws up to which rng_settle_kernel steps (7 VALU per draw) instead of one table product (~300 VALU + 80 LDS reads)

// Two words of the per-pixel state are the same for every pixel of the band, so the tracer keeps them and the launches
// get them as scalars (TraceParams::weyl, ::count) instead of loading and storing them per pixel:
//   weyl_now  -- the XORWOW Weyl word d: seeded[0] when the states are created (the subsequence jump acts on v0..v4
//                only), + 362437 per draw, 3 draws per sample on every path (get_ray, or rng_discard for certain winners);
//   count_now -- the samples accumulated since the accumulators were cleared.
// Plane 0 of d_rng and d_counts hold them only after rt_tracer::materialise(), which every reader of the two buffers calls
// first; *_plane is the word the plane was last filled with.  All guarded by rt_tracer::order_mu.
struct UniformWords {
  uint32_t weyl_now = 0, count_now = 0;
  uint32_t weyl_plane = 0, count_plane = 0;
  bool weyl_plane_ok = false, count_plane_ok = false;
  // Once per launch of `p.samples` x `p.iters` samples (not per half of a split one), with order_mu held until the
  // launch is enqueued: hands the launch the two words and advances them by what it will do to every pixel.
  void take(rtk::TraceParams& p) {
    if (p.flags & rtk::TRACE_ZERO_ACC) count_now = 0u;
    p.weyl = weyl_now; p.count = count_now;
    const uint32_t done = p.samples * (p.iters > 1u ? p.iters : 1u);
    weyl_now += 362437u * 3u * done;
    count_now += done;
  }
  bool weyl_plane_stale() const { return !(weyl_plane_ok && weyl_plane == weyl_now); }
  bool count_plane_stale() const { return !(count_plane_ok && count_plane == count_now); }
  void weyl_plane_filled() { weyl_plane = weyl_now; weyl_plane_ok = true; }
  void count_plane_filled() { count_plane = count_now; count_plane_ok = true; }
};

// A third word of the same kind: owed_draws -- the xorshift steps the pixels of the certain-winner tiles are behind.  A
// small-scene launch whose owe key equals that of the launch enqueued before it runs with TRACE_OWE_RNG: its
// certain-winner waves neither load, advance nor store v0..v4, and the launch adds its 3 x samples x iterations here instead.
// rt_tracer::settle() pays: one rng_settle_kernel over the tiles whose list header has the certain bit -- the same tiles in
// every owing launch, their key being the same.  Who calls it: the first launch that may not owe or has another key (before it
// replaces the lists), materialise(RT_BUF_RNG) -- every reader of the buffer --, the uploads, the instrumented launches,
// and every period-th owing launch (on the streams of its halves, so that the debt stays one table product).
// Where the states are created anew the debt is dropped.  All guarded by rt_tracer::order_mu.
struct RngDebt {
  uint32_t owed_draws = 0;
  uint32_t owing_launches = 0;                 // since the last settle
  uint64_t settles_enqueued = 0;               // settle kernels so far (rt_dbg_owed_state)
  std::optional<OweKey> key;                   // of the launch enqueued last; none: the next launch does not owe
  rtk::TraceParams owe_p;                      // the band-wide launch the debt is settled as: planes, lists, frame
  std::map<uint32_t, DevArray<uint32_t>> settle_tables;   // window tables of T^n by n; steady state holds one, n = period x 3 x samples
  uint32_t period;                             // owing launches between two periodic settles
  explicit RngDebt(const Env& env) : period(env.owe_period > 0 ? static_cast<uint32_t>(env.owe_period) : static_cast<uint32_t>(RT_OWE_PERIOD)) {}
  // whether a launch with owe key `k` (none: it may not owe) owes: its key is that of the launch before it
  bool owes(const std::optional<OweKey>& k) const { return k && key && memcmp(&*k, &*key, sizeof(OweKey)) == 0; }
  void add(const rtk::TraceParams& p) { owed_draws += 3u * p.samples * (p.iters > 1u ? p.iters : 1u); ++owing_launches; }   // once per launch, not per half
  bool settle_due() const { return owing_launches >= period; }
  // the device table of T^n, or null: n draws are stepped.  A new table is in device memory when this returns.
  const uint32_t* table(uint32_t n, hipStream_t a, hipStream_t b) {
    if (n <= kSettleStepMax) return nullptr;
    auto it = settle_tables.find(n);
    if (it != settle_tables.end()) return it->second.get();
    if (settle_tables.size() >= 32u) {                                   // (earlier settles on the trace streams may still read theirs)
      HIP_CHECK(hipStreamSynchronize(b));
      HIP_CHECK(hipStreamSynchronize(a));
      settle_tables.clear();
    }
    const std::vector<uint32_t> host = rth::build_window_table(rth::step_power(n));
    DevArray<uint32_t> dev(host.size());
    HIP_CHECK(hipMemcpy(dev.get(), host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return settle_tables.emplace(n, std::move(dev)).first->second.get();
  }
  void paid() { owed_draws = 0u; owing_launches = 0u; }
  void dropped() { paid(); key.reset(); }      // the states are created anew
};

// The small scenes' tile lists live in a small ring of buffers and are built on a stream of their own (stream_l, high priority): a build is
// enqueued when the launch that needs it is enqueued, so it runs UNDER the trace kernels of the previous launch instead of
// in front of its own (measured in-stream: each half-frame build took 35-45 us competing for wave slots with the other
// half's trace kernel and stalled its own stream meanwhile, profiles/r03_lists_inline_timeline.txt).  Ordering: the trace
// streams wait for list_ready[slot] (recorded on stream_l behind the build); a build into a slot waits until the slot's last
// readers are done.  An event record is a packet the next kernel of its stream queues behind (two of them per step cost
// 4 us of a 66 us C3 step), so the trace streams mark a "free" event only every kFreeStride-th build -- it covers every
// kernel enqueued before it -- and the ring is long enough that a build always finds such an event that is at least
// kFreeStride builds old and still covers the readers of the slot it overwrites (build m: the oldest marked at a build
// e >= m - kListRing + 1; then m - kListRing < e <= m - kFreeStride).
// Neither event is a packet of its own where a kernel can carry it: list_ready is the stop event of the builder's launch,
// and the free pair of build m (m a multiple of kFreeStride) is the stop event of the LAST kernel each trace stream got
// before build m -- in the steady state the two half-frame trace kernels of launch m - 1.  The invariant: when build m is
// enqueued, pair (m / kFreeStride) % kFreeEvents completes no earlier than every list-reading kernel enqueued on its stream
// so far.  A kernel's stop event gives that exactly when no kernel follows it on the stream before build m; carry() hands
// the event to a trace launch only under conditions that make it the last one (the launch built its own lists, so the next
// launch that reads lists builds too or rebinds the event; no settle kernel follows), drop_carry() withdraws it when
// something else is enqueued on a trace stream, and build_ahead() records the event where no kernel carries it for this
// build (an unsplit launch leaves stream_b without a kernel: recorded).  The free_build_ check below stays.
class TileListRing {
 public:
  static constexpr int kListRing = 8, kFreeEvents = 10;
  std::optional<ListKey> key;         // what the current lists were built for

  // a = the primary trace stream, b = stream_b, l = stream_l; calls: where the runtime calls are counted
  void create(hipStream_t a, hipStream_t b, hipStream_t l, EnqueueCalls* calls) {
    a_ = a; b_ = b; l_ = l; calls_ = calls;
    for (Event& e : list_ready_) e = Event(hipEventDisableTiming);
    for (int r = 0; r < kFreeEvents; ++r) { list_free_a_[r] = Event(hipEventDisableTiming); list_free_b_[r] = Event(hipEventDisableTiming); }
  }
  // Sizes the slots for `words` each and decides whether the launch with key `k` builds (reuse = lists built for the same
  // key serve it).  Replacing the slots waits for their readers: `quiesce` the trace streams, then stream_l.
  template <class Quiesce>
  bool prepare(size_t words, const ListKey& k, bool reuse, Quiesce&& quiesce) {
    if (words > words_) {
      quiesce();
      HIP_CHECK(hipStreamSynchronize(l_));
      release();
      const bool big = words * sizeof(uint32_t) > (size_t(128) << 20);   // long lists on large frames: a shorter ring (<= 1 GiB of lists)
      ring_n_ = big ? 4 : 8; free_stride_ = big ? 2 : 4;   // (4 : 2 when one slot exceeds 128 MiB; measured alternatives: HISTORY.md "List ring")
      for (int r = 0; r < ring_n_; ++r) {
        slots_[r].ensure(words);
        // count 0 everywhere until a launch builds; on the stream the builds run on (a hipMemset on the null stream is not
        // ordered with the non-blocking streams and may land AFTER the first build)
        HIP_CHECK(hipMemsetAsync(slots_[r].get(), 0, words * sizeof(uint32_t), l_));
      }
      words_ = words;
    }
    if (reuse && same_key(key, k)) return false;
    key = k;
    return true;
  }
  // The next build (index m) goes into slot m % ring_n on stream_l (see the type's comment); returns m.  The caller
  // enqueues the build kernel into now(), then built().
  uint64_t build_ahead() {
    const uint64_t m = builds_;
    if (m > 0 && m % free_stride_ == 0) {                              // everything the trace streams hold now: the readers of every earlier build
      const int i = static_cast<int>((m / free_stride_) % kFreeEvents);
      if (carried_[0] != m) { HIP_CHECK(hipEventRecord(list_free_a_[i], a_)); ++calls_->records; ++calls_->free_records; }
      if (carried_[1] != m) { HIP_CHECK(hipEventRecord(list_free_b_[i], b_)); ++calls_->records; ++calls_->free_records; }
      free_build_[i] = m;
    }
    const int r = static_cast<int>(m % ring_n_);
    if (m >= alloc_build_ + ring_n_) {                                 // the slot has readers: builds since the buffers exist wrap around
      const uint64_t e = ((m - ring_n_ + 1 + free_stride_ - 1) / free_stride_) * free_stride_;   // oldest record that covers build m - ring_n
      const int i = static_cast<int>((e / free_stride_) % kFreeEvents);
      if (free_build_[i] != e) throw HipFail{"list ring: the free event of the slot's readers is missing"};
      if (e != free_waited_) {                                         // (kFreeStride builds in a row need the same pair: stream_l has it behind it already)
        HIP_CHECK(hipStreamWaitEvent(l_, list_free_a_[i], 0));
        HIP_CHECK(hipStreamWaitEvent(l_, list_free_b_[i], 0));
        calls_->waits += 2u;
        free_waited_ = e;
      }
    }
    cur_ = r;
    return m;
  }
  // the event the build kernel's launch takes as its stop event (launch_tile_lists): no record behind the kernel
  hipEvent_t ready_event() const { return list_ready_[cur_]; }
  void built() { ++builds_; }
  // trace stream `which` (0: a, 1: b) is about to run a trace kernel that reads the current lists
  void wait(hipStream_t st, int which) {
    if (waited_[which] == builds_) return;
    HIP_CHECK(hipStreamWaitEvent(st, list_ready_[cur_], 0));
    ++calls_->waits;
    waited_[which] = builds_;
  }
  // The stop event of the trace kernel about to be launched on stream `which`, or null.  last_before_next_build: the caller
  // knows that no other kernel follows this one on the stream before the next build (see the type's comment).  Every
  // launch passes here, so a launch that does not carry also withdraws what an earlier one on the stream carried.
  hipEvent_t carry(int which, bool last_before_next_build) {
    carried_[which] = 0;
    if (!last_before_next_build || builds_ == 0 || builds_ % free_stride_ != 0) return nullptr;
    carried_[which] = builds_;                                         // the next build's index
    ++calls_->stop_events;
    return (which == 0 ? list_free_a_ : list_free_b_)[(builds_ / free_stride_) % kFreeEvents];
  }
  void drop_carry() { carried_[0] = carried_[1] = 0; }                 // something else goes onto a trace stream
  // Points one (half-)launch at its slots of the current lists (null: `have` = false): a lower half starts behind the
  // upper half's block rows (the split row is a multiple of 8).
  void attach(rtk::TraceParams& p, uint32_t band_row0, bool have) const {
    const size_t slot_base = static_cast<size_t>((p.W + 31u) / 32u) * ((p.row0 - band_row0) / 8u) * 4u;
    p.tile_lists = have ? now() + slot_base * (1u + p.bin_list) : nullptr;
  }
  void release() {                    // callers have synchronised every stream
    for (DevArray<uint32_t>& s : slots_) s.reset();
    words_ = 0; key.reset(); cur_ = 0; alloc_build_ = builds_;
    drop_carry();
  }
  uint32_t* now() const { return slots_[cur_].get(); }
  size_t words() const { return words_; }

 private:
  hipStream_t a_ = nullptr, b_ = nullptr, l_ = nullptr;
  EnqueueCalls* calls_ = nullptr;
  int ring_n_ = 8, free_stride_ = 4;
  DevArray<uint32_t> slots_[kListRing];
  size_t words_ = 0;                  // of each slot
  Event list_ready_[kListRing];
  Event list_free_a_[kFreeEvents], list_free_b_[kFreeEvents];
  uint64_t free_build_[kFreeEvents] = {};   // the build index each pair was marked for (0 = never)
  uint64_t carried_[2] = {0, 0};            // per trace stream: the build index its last kernel carries the free event of (0 = none)
  uint64_t alloc_build_ = 0;          // builds before this one wrote buffers that no longer exist
  uint64_t free_waited_ = 0;          // the build index of the free-event pair stream_l waited for last
  int cur_ = 0;                       // slot of the current lists
  uint64_t builds_ = 0;               // builds so far; the trace streams remember which one they have waited for
  uint64_t waited_[2] = {0, 0};
};

// The dense-scene lists of one half of a split launch (half 0: the unsplit launch or the upper half)
struct HalfLists {
  DevArray<uint32_t> macro, super, wave;
  std::optional<ListKey> macro_key;   // what the macro (and super) lists were built for
  bool wave_valid = false;            // the wave lists follow the macro lists' key
  uint32_t wave_cap = 0;              // capacity per tile and tiles the wave lists were built with
  size_t wave_tiles = 0;
};

// What a tracer of `rows` rows of a w x h frame cannot be, as the text of the refusal; empty = acceptable.  Asked before
// anything is allocated (rt_tracer_create_ex, rt_tracer_resize, rt_tracer::reshape): a pixel's subsequence x + y * W and
// the band's pixel count are 32-bit words everywhere, and rng_init_kernel indexes a band only up to kRngInitMaxPixels.
inline std::string band_refusal(uint32_t w, uint32_t h, uint32_t rows) {
  if (static_cast<uint64_t>(w) * h > 0xFFFFFFFFull)
    return "frames above 2^32 - 1 pixels are not supported (32-bit pixel index, Kernels.cuh:128)";
  if (static_cast<uint64_t>(w) * rows > rtk::kRngInitMaxPixels)
    return fmt("a tracer holds at most 2^32 - 2^19 = %llu pixels (%u x %u asked for): shard a larger frame into row bands "
               "(rt_options.full_height / row_begin)", static_cast<unsigned long long>(rtk::kRngInitMaxPixels), w, rows);
  return std::string();
}

struct Group;        // rt_multi.hpp: the tile gather of a frame sharded over several GPUs
struct MultiState;   // rt_multi.hpp: the bands of a multi-device tracer

}  // namespace rtr

struct rt_tracer {
  // A handle is one of: a plain tracer (one device, the whole frame or one row band), a band tracer that joined a multi-process
  // group (grp != null), or a multi-device tracer (mg != null: the fields below then describe the whole frame and hold camera,
  // callbacks, render thread and error text; the device buffers live in the band tracers mg owns).
  // Fields first, by subject, the functions behind them.  Members are destroyed in reverse order of declaration: the streams are
  // declared before everything that is freed or recorded on them, the render thread behind everything its jobs use
  // (rt_tracer_destroy calls quiesce() before any of it goes).
  rtr::Group* grp = nullptr;
  rtr::MultiState* mg = nullptr;
  // ---- configuration and options
  rtr::Env env;                     // the environment switches as they were at rt_tracer_create
  int device = 0;
  uint32_t W = 0, H = 0;            // full image
  uint32_t row0 = 0, rows = 0;      // owned band
  bool band_mode = false;
  uint64_t seed = 1;
  bool fma = true, filter = true, bin = true, nearest_hit = false;
  bool smooth_normals = false;        // RT_FLAG_SMOOTH_NORMALS; takes effect for edge-format scenes
  uint32_t k_req = 0, chunk_req = 0, bin_list_req = 0;
  bool split_launches = true;         // RT_MI355X_NO_SPLIT=1 turns it off
  bool macro = true;                  // RT_FLAG_NO_MACRO_BINS turns it off
  bool pretest = true;                // RT_MI355X_NO_PRETEST=1 turns the per-sample forms off
  bool sure_hit = true;               // RT_FLAG_NO_SURE_HIT: tiles of one certainly-hit triangle run the tests anyway
  // Stored tile candidate lists (small scenes) survive from one Trace to the next while camera, lens, scene,
  // frame and arithmetic mode are unchanged -- like any acceleration structure that is rebuilt only when its
  // inputs change.  rt_tracer_set_list_reuse(t, 0) restricts the reuse to the launches of one Trace.
  bool reuse_across_traces = true;
  // the forms pay for themselves on dense scenes only (break-even ~3000 triangles at 1080p; C4: -13 %)
  static constexpr uint32_t kPretestMinTris = 4096;
  static constexpr uint32_t kMacroW = 128, kMacroH = 64, kMacroCapMax = 65536;
  // Dense scenes: a level above the macro tiles (super tiles of kSuperF x kSuperF of them, super_bin_kernel) so that a macro
  // tile tests its super tile's lists instead of the scene (rt_lists.hpp): C4 10.2 M -> ~1.5 M triangle tests per rebuild.
#ifndef RT_SUPER_F
#define RT_SUPER_F 4
#endif
  static constexpr uint32_t kSuperF = RT_SUPER_F, kSuperMinTris = 2048;
  bool super_level = true;            // RT_FLAG_NO_SUPER_BINS turns it off
  // ---- streams and ordering
  rtr::Stream stream;                 // primary stream: everything that is not the lower half of a split launch
  // Trace launches of tall frames are split into two half-frame kernels on two streams: consecutive
  // launches then overlap one half's drain (falling occupancy at the end of a kernel) with the other half's
  // bulk -- 146 -> 131 us per back-to-back C3 step (tools/two_stream.py); a pixel's launches stay ordered
  // because its half always uses the same stream.  main_stream() is the ordering point for everything else.
  rtr::Stream stream_b;
  rtr::Stream stream_l;               // the small scenes' list builds (highest priority; TileListRing)
  rtr::Event join_event, fork_event;
  bool b_dirty = false;               // work on stream_b the primary stream has not waited for yet
  bool a_dirty = false;               // non-launch work on the primary stream that stream_b has not waited for yet
  // The ordering state is shared by the render thread and by entry points that do not join it
  // (rt_tracer_sync, rt_tracer_read_buffer, the device copies): order_mu serialises the dirty flags and the
  // re-recording of the two shared events -- and the uniform state words and the owed draws below with the launches that
  // advance them (recursive: a launch is enqueued under it and asks for main_stream() / fork_b() on the way).
  std::recursive_mutex order_mu;
  rtr::EnqueueCalls calls;            // guarded by order_mu
  uint64_t list_builds[4] = {};       // small-scene list builds by builder kind (rtk::launch_tile_lists) since creation (rt_dbg_list_builds; guarded by order_mu)
  // ---- render buffers and scene
  rtk::KernelTable kernels;           // launch descriptors of this tracer's device
  rtr::DevArray<float4> d_render;
  rtr::DevArray<uint32_t> d_counts, d_image, d_rng;
  rtr::UniformWords words;            // the Weyl word and the sample count of every pixel (guarded by order_mu)
  rtr::RngDebt debt{env};             // the draws the certain-winner tiles are behind (guarded by order_mu)
  rtr::PinnedArray<uint32_t> h_image;       // handed to callbacks
  rtr::PinnedArray<uint32_t> h_image_alt;   // second image: update i+1 is produced while the callback reads update i
  uint32_t* image_mirror = nullptr; // rt_tracer_set_image_mirror: second target of emitting rt_tracer_launch* / trace_enqueue launches
  rtr::Event handoff_event;
  int handoff_next = 0;             // which of the two host images the next emitting launch of a Trace writes
  rtr::DevArray<float4> d_tri;      // (e2.xyz,e1.x),(e1.yz,v0.xy) records
  rtr::DevArray<float> d_tri_b;     // v0.z
  rtr::DevArray<float4> d_tri_color;
  rtr::DevArray<float4> d_tri_n;    // 3 unpacked vertex normals per triangle, edge-format scenes only
  uint32_t n_tris = 0;
  rtr::DevArray<float4> d_spheres;
  uint32_t n_spheres = 0, scene_generation = 0;
  // ---- lists
  // Candidate lists + certain-winner verdicts of the small scenes' tiles (TracePath::SmallLists): built by tile_lists_kernel
  // on stream_l into the next slot of a ring, ahead of the launch that needs them, and kept while camera snapshot, lens,
  // scene, frame, list length and arithmetic mode are unchanged (lists.key; they do not depend on the samples).  The first
  // launch of a Trace rebuilds them when lists are not kept across Traces (reuse_across_traces: bench.py's headline).
  rtr::TileListRing lists;            // small scenes: the tile lists, built ahead on stream_l
  rtr::Event stagger_event;
  std::atomic<bool> stagger_next{true};   // the next split launch starts from an idle tracer: stagger its halves (enqueue_trace_launch)
  // Which halves a split small-scene launch uses: the band's upper and lower rows (best when the two cost the same: C3 61.0
  // against 62.2 us per step) or its even and odd block rows (the same cost whatever the picture: a tilted camera with 57 % /
  // 22 % ray-generating tiles above / below the split 62.6 against 70.5 us).  The two-level list builder counts the
  // ray-generating tiles per half and publishes the pair to pinned host memory behind every build; the enqueueing thread
  // reads the latest pair (a few launches old: the picture does not jump) and switches with hysteresis -- a switch moves
  // pixels from one stream to the other, so both streams are joined first (want_interleave()).
  rtr::DevArray<uint32_t> d_half_cost;                // two device counters
  rtr::PinnedArray<unsigned long long> h_half_cost;   // upper | lower << 32 of the latest finished build
  bool rows_interleaved = false;
  rtr::DevArray<float4> d_sure_table;                 // small scenes: what a certain-winner pixel accumulates (attach_sure_table())
  uint32_t sure_table_samples = 0;
  uint64_t sure_table_scene = ~0ull;
  rtr::HalfLists half_lists[2];       // dense scenes: one per half of a split launch (attach_macro_lists())
  // ---- queries (rt_query_api.hpp)
  rtr::QueryState queries;
  // ---- camera, callbacks and threads (camera + callbacks: guarded by state_mu; snapshotted per launch like the by-value kernel argument)
  std::mutex state_mu;
  rtr::Camera cam;
  rt_callback_fn update_cb = nullptr; void* update_user = nullptr;
  rt_callback_fn finished_cb = nullptr; void* finished_user = nullptr;
  std::mutex api_mu;
  rtr::RenderThread render;
  std::atomic<bool> stopped{false}, completed{false};
  rtr::LaunchClock clock;
  std::mutex err_mu;
  std::string last_error;
  uint32_t last_k = 0, last_chunk = 0, last_lds = 0;

  hipStream_t main_stream() {         // primary stream, made to wait for everything enqueued on stream_b
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    if (b_dirty) {
      HIP_CHECK(hipEventRecord(join_event, stream_b));
      HIP_CHECK(hipStreamWaitEvent(stream, join_event, 0));
      ++calls.records; ++calls.waits;
      b_dirty = false;
    }
    a_dirty = true;
    lists.drop_carry();                                                // (whatever the caller enqueues may read the lists)
    return stream;
  }
  void fork_b() {                     // stream_b waits for the non-launch work enqueued on the primary stream
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    if (!a_dirty) return;
    HIP_CHECK(hipEventRecord(fork_event, stream));
    HIP_CHECK(hipStreamWaitEvent(stream_b, fork_event, 0));
    ++calls.records; ++calls.waits;
    a_dirty = false;
  }
  void wait_queries() { queries.wait(); }
  // the owe key of the launch `p` on `path`, or none: such a launch may not owe
  std::optional<rtr::OweKey> owe_key_of(const rtk::TraceParams& p, rtk::TracePath path) const {
    const bool sure_ok = (p.flags & (rtk::TRACE_NEAREST_HIT | rtk::TRACE_NO_SURE_HIT)) == 0u && p.n_spheres == 0u && p.tri_n == nullptr;
    if (env.no_owe || path != rtk::TracePath::SmallLists || p.n_tris == 0u || p.stats != nullptr || !sure_ok) return std::nullopt;
    rtr::OweKey k;
    memset(&k, 0, sizeof k);
    k.lists = make_key(p, p.bin_list);
    k.mode_flags = mode_flags(p); k.n_spheres = p.n_spheres; k.smooth = p.tri_n != nullptr ? 1u : 0u;
    k.path = static_cast<uint32_t>(path);
    return k;
  }
  const uint32_t* settle_table(uint32_t n) { return debt.table(n, stream, stream_b); }
  // pays the debt on the stream that orders behind both trace streams; nothing owed: nothing enqueued
  void settle() {
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    if (debt.owed_draws == 0u) return;
    const uint32_t* const table = settle_table(debt.owed_draws);
    HIP_CHECK(rtk::launch_rng_settle(debt.owe_p, debt.owed_draws, table, main_stream()));
    ++calls.launches;
    debt.paid(); ++debt.settles_enqueued;
  }
  // RT_BUF_RNG / RT_BUF_COUNTS are about to be read: plane 0 / the counts get the current word, on the stream that
  // orders behind both trace streams (no launch touches either plane).  Skipped when the plane already holds it.
  void materialise(int which) {
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    if (which == RT_BUF_RNG && d_rng.get() != nullptr) settle();
    if (which == RT_BUF_RNG && words.weyl_plane_stale() && d_rng.get() != nullptr) {
      HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_rng.get()), static_cast<int>(words.weyl_now), npix(), main_stream()));
      words.weyl_plane_filled();
    }
    if (which == RT_BUF_COUNTS && words.count_plane_stale() && d_counts.get() != nullptr) {
      HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_counts.get()), static_cast<int>(words.count_now), npix(), main_stream()));
      words.count_plane_filled();
    }
  }
  bool want_interleave() {
    if (env.row_interleave >= 0) return env.row_interleave != 0;
    if (h_half_cost.get() == nullptr) return false;
    const unsigned long long w = *reinterpret_cast<volatile unsigned long long*>(h_half_cost.get());
    const double u = static_cast<double>(w & 0xFFFFFFFFull), l = static_cast<double>(w >> 32);
    if (u + l < 16.0) return rows_interleaved;    // nothing (yet) to go by
    const double ratio = (u > l ? u : l) / ((u > l ? l : u) + 1.0);
    return rows_interleaved ? ratio > 1.15 : ratio > 1.25;
  }
  uint32_t split_row(uint32_t band_rows) const {   // first row of the lower half of a split launch (a multiple of 8); 0 = not split
    return (split_launches && band_rows >= 128u) ? ((band_rows / 2u + 7u) / 8u) * 8u : 0u;   // (40 / 45 / 55 / 60 % measured: the halves have to cost the same)
  }
  void sync_list_stream() { if (stream_l) HIP_CHECK(hipStreamSynchronize(stream_l)); }
  // rt_tracer_sync: every stream idle, the next split launch staggered again, the sampled launches enqueued so far accounted
  void sync_all() {
    const uint64_t seen = clock.seq_now();           // launches enqueued so far; a running render thread may add more
    HIP_CHECK(hipStreamSynchronize(main_stream()));
    sync_list_stream();                              // (nothing the caller could read depends on it; a Sync leaves the device idle)
    stagger_next = true;
    clock.drain_before(seen);
  }

  void set_error(const std::string& s) {
    { std::lock_guard<std::mutex> lk(err_mu); last_error = s; }
    rtr::set_global_error(s);
  }
  uint32_t npix() const { return W * rows; }
  void use_device() { HIP_CHECK(hipSetDevice(device)); }

  void cancel_and_join() {                                               // RayTracerImpl.cu:72-77
    if (render.busy()) {
      stopped = true;
      render.wait_idle();
      stopped = false;
    }
  }

  void release_buffers() {                                               // :317-342
    d_render.reset(); d_counts.reset(); d_image.reset(); d_rng.reset(); h_image.reset(); h_image_alt.reset();
  }

  // every stream idle and every sampled launch accounted (destruction: the owning members release the rest)
  void quiesce() {
    (void)hipSetDevice(device);
    for (const rtr::Stream* s : {&stream_b, &stream, &stream_l, &queries.stream_q}) if (*s) (void)hipStreamSynchronize(*s);
    if (queries.done) (void)hipEventSynchronize(queries.done);
    clock.drain();
  }

  void create_states() {                                                 // random::CreateStates, Random.cu:32-52
    uint32_t seeded[6];
    rth::seed_state(seed, seeded);
    const uint32_t p0 = row0 * W;                                        // subsequence of the band's first pixel
    const std::string refused = rtr::band_refusal(W, H, rows);           // (the entry points asked before they allocated)
    if (!refused.empty()) throw rtr::BadArgument{refused};
    uint32_t* const tables = rtr::jump_device(device);
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    HIP_CHECK(rtk::launch_rng_init(d_rng.get(), npix(), p0, seeded, tables, tables + rtr::kJumpWords, main_stream()));
    words.weyl_now = seeded[0]; words.weyl_plane_ok = false;                         // (the kernel writes v0..v4)
    debt.dropped();
  }

  void create_buffers() {                                                // ctor :33-40, Resize :96-102
    const size_t n = npix();
    if (n == 0) throw rtr::HipFail{"image has no pixels"};
    d_rng.ensure(n * 6); d_render.ensure(n); d_counts.ensure(n); d_image.ensure(n); h_image.ensure(n); h_image_alt.ensure(n);
    memset(h_image.get(), 0, n * sizeof(uint32_t));
    memset(h_image_alt.get(), 0, n * sizeof(uint32_t));
    // the reference leaves new buffers uninitialised until the first Trace clears them; we
    // zero them so that reading before a Trace is defined (the counts: materialise())
    HIP_CHECK(hipMemsetAsync(d_render.get(), 0, n * sizeof(float4), main_stream()));
    HIP_CHECK(hipMemsetAsync(d_image.get(), 0, n * sizeof(uint32_t), main_stream()));
    { std::lock_guard<std::recursive_mutex> lk(order_mu); words.count_now = 0u; words.count_plane_ok = false; }
    create_states();
    HIP_CHECK(hipStreamSynchronize(main_stream()));
  }

  // multi-device Resize: new frame size AND new band of it (scene, camera and options stay)
  void reshape(uint32_t w, uint32_t h, uint32_t r0, uint32_t n) {
    const std::string refused = rtr::band_refusal(w, h, n);              // before the buffers go: a refused tracer stays as it is
    if (!refused.empty()) throw rtr::BadArgument{refused};
    HIP_CHECK(hipStreamSynchronize(main_stream()));
    sync_list_stream();
    release_buffers();
    W = w; H = h; row0 = r0; rows = n;
    lists.key.reset();
    create_buffers();
  }

  // the band's BGRA8 image to a gather buffer on the same device (paths that converted without a trace launch)
  void copy_image_to(uint32_t* target) {
    HIP_CHECK(hipMemcpyAsync(target, d_image.get(), static_cast<size_t>(npix()) * sizeof(uint32_t), hipMemcpyDeviceToDevice, main_stream()));
  }

  // Focal points of a full 8x8 tile from its four corner pixels.  F = pos + focal * d, d = M q / |M q|, q = (cx, cy, -1)
  // affine in the pixel (ThinLensCamera.cuh:116-128).  Along an axis direction h the second derivative of x -> M x / |M x|
  // at q is ((3 c^2 - 1) u - 2 c h') |h'|^2 / |M q|^2 (u = M q / |M q|, h' = M h / |M h|, c = u.h'), of norm
  // <= 4 smax^2 / (smin^2 |q|^2) <= 4 lmax / lmin with lmax, lmin bounds of the eigenvalues of M^T M (Gershgorin; 1 for the
  // rotation the camera builds) and |q| >= 1.  A bilinear interpolant over a rectangle of sides a x b is off by at most
  // (a^2 sup|f_xx| + b^2 sup|f_yy|) / 8 in every direction, and its extremes are at the corners; cx, cy are monotone in the
  // pixel index (rounded operations are monotone), so the corner pixels bound the rectangle.  Evaluated in double, rounded up.
  void tile_corner_bound(rtk::TraceParams& p) const {
    p.tile_curv = -1.0f; p.tile_round = 0.0f;
    double G[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        G[i][j] = 0.0;
        for (int r = 0; r < 3; ++r) G[i][j] += static_cast<double>(p.cam[i * 3 + r]) * static_cast<double>(p.cam[j * 3 + r]);
      }
    double lmax = 0.0, lmin = 1e300;
    for (int i = 0; i < 3; ++i) {
      const double off = std::fabs(G[i][(i + 1) % 3]) + std::fabs(G[i][(i + 2) % 3]);
      lmax = std::max(lmax, G[i][i] + off);
      lmin = std::min(lmin, G[i][i] - off);
    }
    if (!(lmin > 0.25) || !(lmax < 4.0)) return;                       // not a (near-)rotation: every lane bounds
    const double hh = std::fabs(static_cast<double>(p.half_height)), asp = std::fabs(static_cast<double>(p.aspect));
    const double a = 7.0 * 2.0 * hh * asp / static_cast<double>(W), b = 7.0 * 2.0 * hh / static_cast<double>(H);
    // worth it only where the curvature term is small against the tile itself (<= 10 % of its smaller side: 1080p at
    // 70 degrees is 0.9 %); coarse wide-angle frames keep the exact range of their lanes
    if (!(0.5 * (a * a + b * b) * (lmax / lmin) <= 0.1 * std::min(a, b))) return;
    const double foc = std::fabs(static_cast<double>(p.focal));
#ifndef RT_TILE_CURV_SCALE          // teeth test of the adversarial campaign only (profiles/r02_boundary_campaign.txt)
#define RT_TILE_CURV_SCALE 1.0
#endif
    const double curv = foc * 0.5 * (a * a + b * b) * (lmax / lmin) * 1.001 * RT_TILE_CURV_SCALE + 1e-30;
    const double pos = std::max(std::fabs(p.cam[9]), std::max(std::fabs(p.cam[10]), std::fabs(p.cam[11])));
    const double round = foc * (1.0 + hh * asp + hh) + pos;
    if (!(curv <= 1e30) || !(round <= 1e30)) return;                   // NaN / inf lens: every lane bounds
    p.tile_curv = std::nextafter(static_cast<float>(curv), 3.0e38f);
    p.tile_round = std::nextafter(static_cast<float>(round), 3.0e38f);
  }

  rtk::TraceParams params(uint32_t samples) {
    rtk::TraceParams p;
    memset(&p, 0, sizeof p);
    rtr::Camera c;
    { std::lock_guard<std::mutex> lk(state_mu); c = cam; }               // *mCamera by value, :221
    p.render = d_render.get(); p.rng = d_rng.get();             // (weyl, count: UniformWords::take)
    p.W = W; p.H = H; p.row0 = row0; p.rows = rows; p.npix = npix(); p.samples = samples;
    for (int col = 0; col < 4; ++col)
      for (int r = 0; r < 3; ++r) p.cam[col * 3 + r] = c.M[col * 4 + r];
    p.half_height = c.tan_half_fov();
    p.aspect = static_cast<float>(W) / static_cast<float>(H);            // ThinLensCamera.cuh:113
    p.focal = c.focal; p.aperture = c.aperture;
    tile_corner_bound(p);
    p.tri_a = d_tri.get(); p.tri_b = d_tri_b.get(); p.tri_color = d_tri_color.get(); p.n_tris = n_tris;
    p.tri_n = smooth_normals ? d_tri_n.get() : nullptr;
    p.stats = nullptr;
    p.spheres = d_spheres.get(); p.n_spheres = n_spheres;
    p.chunk = chunk_req ? chunk_req : 1024u;
    if (p.chunk > 4096u) p.chunk = 4096u;                                // 144 KiB of the CU's 160 KiB LDS
    // per-wave candidate list: whole (small) scene if it fits, else 256 records = 40 KiB per
    // block -> 4 blocks per CU; 64 records = 10 KiB per block lets 8 blocks (32 waves) share a CU
    // (a trace block holds its LDS until its slowest wave is done -- in a frame of mostly certain-winner tiles most resident
    // blocks are down to one or two live waves, and at 10 KiB per block the CU's LDS, not its wave slots, capped the waves in
    // flight: 32-record granularity, 5 KiB per block for scenes of up to 32 triangles)
    uint32_t want = bin_list_req ? bin_list_req : ((n_tris + 31u) / 32u) * 32u;
    want = ((want + 31u) / 32u) * 32u;
    p.bin_list = want < 32u ? 32u : want > (bin_list_req ? 960u : 256u) ? (bin_list_req ? 960u : 256u) : want;
    // scenes that do not fit the per-wave list: 192 records per wave + a 1024-entry block-level
    // pre-cull list keep the block at 34.9 KiB of LDS (4 blocks per CU)
    p.block_list = n_tris > p.bin_list ? 1024u : 0u;
    if (p.block_list != 0u && !bin_list_req) p.bin_list = 192u;
    // Per-sample conservative forms (TRACE_PRETEST) for the large-scene kernels: 76 instead of 40 bytes per
    // candidate in LDS, so 128 candidates per wave and a 448-entry block list keep the block at 40 KiB
    // (4 blocks per CU, as before).  Scenes dense enough to overflow 128-entry lists regularly lose more
    // by the extra classification rounds than the forms save (100 k triangles at 4K: 4.98 -> 5.43 ms),
    // hence the size limit; C4 (10 k): 5.93 -> 5.66 ms.
    if (pretest && filter && bin && n_tris >= kPretestMinTris && n_tris <= 50000u) {
      p.pretest_on = 1u;
      if (!bin_list_req) p.bin_list = RT_PRETEST_LIST;
      else p.bin_list = (p.bin_list + 1u) & ~1u;
      if (p.block_list != 0u) p.block_list = 448u;
    }
    return p;
  }

  // the launch-independent TRACE_* flags of this tracer
  uint32_t mode_flags(const rtk::TraceParams& p) const {
    return (nearest_hit ? rtk::TRACE_NEAREST_HIT : 0u) | (p.pretest_on ? rtk::TRACE_PRETEST : 0u) |
           (sure_hit ? 0u : rtk::TRACE_NO_SURE_HIT);
  }

  int pick_k(uint32_t samples) const {
    if (k_req == 1 || k_req == 2 || k_req == 4) return static_cast<int>(k_req);
    // K samples of a pixel in registers per pass.  4 amortises the LDS record reads on long
    // candidate lists (C4: 27 ms vs 35 ms at K = 1); scenes with a handful of triangles are
    // ray-generation bound and run ~5 % faster at 2 (fewer VGPRs, C3: 191 vs 197 us).
    const uint32_t want = (n_tris <= 128u) ? 2u : 4u;
    return samples >= want ? static_cast<int>(want) : samples >= 2 ? 2 : 1;
  }

  // RunTraceKernel, RayTracerImpl.cu:204-234, without the blocking wait.  `flags` are the TRACE_* fusions: the first launch after
  // the clear treats the accumulators as zero (no memset, no accumulator read), a launch whose result is handed out also writes
  // BGRA8.  sync_after: 0 = none, 1 = wait for this launch (the reference's behaviour, :228), N > 1 = keep at most N launches in
  // flight (wait for the launch N-1 back).  One body for the launch's 1 or 2 parts ("Where a trace launch's parts are formed").
  void enqueue_trace_launch(uint32_t samples, uint32_t flags, int sync_after, uint32_t iters = 1,
                            uint32_t* host_image = nullptr, bool allow_split = true) {
    const int K = pick_k(samples);
    rtk::TraceParams p = params(samples);
    p.iters = iters;
    p.image_host = host_image;
    p.flags = flags | mode_flags(p);
    p.image = d_image.get();
    const rtk::TracePath path = trace_path(p);
    std::unique_lock<std::recursive_mutex> uniform_lk(order_mu);          // the state words and the launch that advances them
    // Owed draws: the launch owes when its key is that of the launch before it; otherwise the debt is paid first -- before
    // the lists the owing launches read are replaced.
    const std::optional<rtr::OweKey> okey = owe_key_of(p, path);
    const bool owes = debt.owes(okey);
    if (!owes) settle();
    debt.key = okey;
    bool have_lists = false;
    const bool build_lists = prepare_tile_lists(p, path, (flags & rtk::TRACE_ZERO_ACC) != 0u, have_lists);
    attach_sure_table(p, have_lists);
    if (owes) p.flags |= rtk::TRACE_OWE_RNG;
    last_k = K; last_chunk = p.chunk;
    // (DenseLists: the LDS of the classifying kernel, what rt_tracer_info has always reported for dense scenes)
    last_lds = rtk::trace_lds_bytes(p, path == rtk::TracePath::DenseLists ? rtk::TracePath::ClassifyForms : path);
    // The launch's parts: the band on the primary stream or, for tall frames, its upper half there and its lower half on stream_b (see
    // the fields' comment).  The split row is a multiple of 8, each half is a row band of its own (own tile / macro lists).
    const uint32_t r0 = allow_split ? split_row(p.rows) : 0u;
    rtr::EventPair e;                                                    // sampled launches: timing events (LaunchClock)
    const bool timed = clock.start(sync_after == 1, r0 != 0u, e);
    words.take(p);
    if (owes) debt.add(p);
    const bool settle_now = owes && debt.settle_due();                    // the periodic settle, behind this launch's kernels
    const uint32_t* const settle_tab = settle_now ? settle_table(debt.owed_draws) : nullptr;
    ++calls.steps;
    // The list ring's free events ride on this launch's trace kernels when those are the last kernels their streams get
    // before the next build (TileListRing): the launch built its lists -- then the next launch that reads lists builds too,
    // or passes lists.carry() itself and withdraws the event -- and no settle kernel follows.
    const bool last_before_build = build_lists && !settle_now;
    const int n_parts = r0 == 0u ? 1 : 2;
    rtk::TraceParams part[2] = {p, p};
    const hipStream_t st[2] = {stream, stream_b};
    bool stagger = false;
    if (n_parts == 1) {
      (void)main_stream();                                               // a launch on one stream orders behind both
      if (build_lists) build_tile_lists_ahead(p);
    } else {
      if (a_dirty) fork_b();                                             // (order_mu is held: the steady state takes it once per launch)
      if (build_lists) build_tile_lists_ahead(p);
      // The two halves overlap best in ANTI-phase (one half's drain under the other's bulk); started together -- both
      // released by the same event, or from an idle device -- they can lock IN phase and stay there for a whole run
      // (measured at C3: 93 instead of 80 us per step, profiles/r03_phase_regimes.txt).  The first split launch after
      // the tracer was idle therefore lets its second kernel start about half a kernel behind its first (a delay wave, or
      // -- before any kernel has been sampled -- behind the first kernel's end).  Later launches free-run.
      stagger = stagger_next.exchange(false);
      // Small scenes: the halves are the band's upper and lower rows or its even and odd block rows (want_interleave()).
      // Dense scenes keep row halves (their macro lists are per half, in macro tiles of 8 block rows).
      const bool interleave = have_lists && want_interleave();
      if (have_lists && interleave != rows_interleaved) {                  // pixels change streams: everything before goes first
        (void)main_stream();
        fork_b();
        rows_interleaved = interleave;
        if (env.log) fprintf(stderr, "[rt_mi355x] split launches: halves by %s\n", interleave ? "even / odd block rows" : "rows");
      }
      if (interleave) { part[0].row_il = part[1].row_il = 1u; part[1].row_phase = 1u; }
      else { part[0] = sub_band(p, 0u, r0); part[1] = sub_band(p, r0, p.rows - r0); }
    }
    if (timed) { HIP_CHECK(hipEventRecord(e.a, stream)); ++calls.records; }   // (of a split launch the sampled duration is the upper half-frame kernel's)
    for (int h = 0; h < n_parts; ++h) {
      lists.attach(part[h], row0, have_lists);
      if (have_lists) lists.wait(st[h], h);
      if (h == 1 && stagger) {
        // half a kernel behind the upper half: by the clock when the tracer knows how long its half-frame kernels take
        // (0.45 of the last sampled one), else behind the upper half's end
        const uint32_t us = static_cast<uint32_t>(clock.last_half_ms() * 450.0f);
        if (us >= 5u) { HIP_CHECK(rtk::launch_delay(us, stream_b)); ++calls.launches; }
        else { HIP_CHECK(hipStreamWaitEvent(stream_b, stagger_event, 0)); ++calls.waits; }
      }
      const rtk::TracePath part_path = trace_path(part[h]);              // (a half's rows decide whether its wave lists fit)
      attach_macro_lists(part[h], part_path, h, st[h], (flags & rtk::TRACE_ZERO_ACC) != 0u);   // part of the launch: timed with it
      // (one part: no lists.carry(1, ..) -- main_stream() withdrew what stream_b's last kernel carried)
      HIP_CHECK(rtk::launch_trace(part[h], fma, filter, part_path, K, st[h], &kernels, lists.carry(h, last_before_build)));
      ++calls.launches;
      if (h == 0 && stagger) { HIP_CHECK(hipEventRecord(stagger_event, stream)); ++calls.records; }
    }
    for (int h = 0; timed && h < n_parts; ++h) { HIP_CHECK(hipEventRecord(h == 0 ? e.b : e.c, st[h])); ++calls.records; }
    if (owes) { debt.owe_p = p; lists.attach(debt.owe_p, row0, true); }  // (the band as one launch: settle() orders behind both streams)
    // the periodic settle: each part's tiles on that part's own stream, with the geometry of its trace kernel: no join
    for (int h = 0; settle_now && h < n_parts; ++h) { HIP_CHECK(rtk::launch_rng_settle(part[h], debt.owed_draws, settle_tab, st[h])); ++debt.settles_enqueued; ++calls.launches; }
    if (settle_now) debt.paid();
    if (n_parts == 2) b_dirty = true;
    uniform_lk.unlock();
    if (timed) clock.enqueued(std::move(e), sync_after);
  }

  // a row band [off, off + n) of a launch as a launch of its own
  static rtk::TraceParams sub_band(const rtk::TraceParams& p, uint32_t off, uint32_t n) {
    rtk::TraceParams q = p;
    const size_t px = static_cast<size_t>(off) * p.W;
    q.row0 = p.row0 + off; q.rows = n;
    q.render = p.render + px; q.rng = p.rng + px;                              // npix stays the RNG planes' stride
    q.image = p.image + px;
    if (p.image_host != nullptr) q.image_host = p.image_host + px;
    return q;
  }

  void clear_accumulators() {                                            // :242-243
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    HIP_CHECK(hipMemsetAsync(d_render.get(), 0, static_cast<size_t>(npix()) * sizeof(float4), main_stream()));
    words.count_now = 0u;                                                      // (the count buffer: materialise())
  }

  void convert() {                                                       // RunConverterKernel :189-202
    std::lock_guard<std::recursive_mutex> lk(order_mu);
    HIP_CHECK(rtk::launch_convert(d_render.get(), words.count_now, d_image.get(), npix(), main_stream()));
  }

  // Waits for a stream with the host polling: the end of a Trace is latency, not throughput (the reference's caller re-traces
  // on every mouse-move event), and the runtime's blocking wait adds its wake-up to every frame.  Long waits block.
  static void sync_polling(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(st);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) HIP_CHECK(e);
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    (void)hipGetLastError();                                             // hipErrorNotReady is an answer, not a failure
    HIP_CHECK(hipStreamSynchronize(st));
  }

  void fetch_image() {                                                   // device image -> pinned host copy
    HIP_CHECK(hipMemcpyAsync(h_image.get(), d_image.get(), static_cast<size_t>(npix()) * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, main_stream()));
    HIP_CHECK(hipStreamSynchronize(main_stream()));                             // :259,:287
  }

  // the key of lists built for launch `p`; bin_word: the list length (tile lists) or the macro geometry (macro lists)
  rtr::ListKey make_key(const rtk::TraceParams& p, uint32_t bin_word) const {
    rtr::ListKey k;
    memset(&k, 0, sizeof k);                       // padding too: the key is compared bytewise
    memcpy(k.cam, p.cam, sizeof k.cam);
    k.half_height = p.half_height; k.aspect = p.aspect; k.focal = p.focal; k.aperture = p.aperture;
    k.W = p.W; k.H = p.H; k.row0 = p.row0; k.rows = p.rows; k.bin_list = bin_word; k.n_tris = p.n_tris;
    k.scene_generation = scene_generation; k.fma = fma;
    return k;
  }

  // Small scenes (no more triangles than the per-wave list holds): the tiles' candidate lists + certain-winner verdicts are
  // built by tile_lists_kernel ahead of the trace launch that needs them.  Decides once per launch whether the lists have to
  // be (re)built first -- camera snapshot, scene, frame, list length or arithmetic mode changed; or this is the first launch
  // of a Trace and the lists are not kept across Traces (rt_tracer_set_list_reuse(t, 0): bench.py's headline, every step
  // builds its own) -- and makes sure the buffer holds the whole band's lists.  have = the scene uses lists at all.
  bool prepare_tile_lists(const rtk::TraceParams& p, rtk::TracePath path, bool first_launch_of_trace, bool& have) {
    have = path == rtk::TracePath::SmallLists && p.n_tris != 0u;
    if (!have) return false;
    const size_t tiles = static_cast<size_t>((W + 31u) / 32u) * ((rows + 7u) / 8u + 1u) * 4u;   // (+1: a split adds a partial block row)
    return lists.prepare(tiles * (1u + p.bin_list), make_key(p, p.bin_list), !(first_launch_of_trace && !reuse_across_traces),
                         [&] { HIP_CHECK(hipStreamSynchronize(main_stream())); });
  }

  // Small scenes: the per-triangle table of what a certain-winner pixel accumulates in a launch of `samples` samples
  // (rtk::sure_table_kernel), rebuilt when the sample count or the scene changed.  Built on the stream that orders behind
  // both trace streams: earlier launches may still read the previous table.
  void attach_sure_table(rtk::TraceParams& p, bool have) {
    p.sure_table = nullptr;
    if (!have || env.no_sure_table || p.n_tris == 0u) return;
    if (sure_table_samples != p.samples || sure_table_scene != scene_generation || d_sure_table.size() < p.n_tris) {
      hipStream_t st = main_stream();
      if (d_sure_table.size() < p.n_tris) {
        HIP_CHECK(hipStreamSynchronize(st));
        d_sure_table.ensure(p.n_tris);
      }
      HIP_CHECK(rtk::launch_sure_table(p.tri_color, p.n_tris, p.samples, d_sure_table.get(), st));
      ++calls.launches;
      sure_table_samples = p.samples; sure_table_scene = scene_generation;
    }
    p.sure_table = d_sure_table.get();
  }

  // The lists of the whole band, built on stream_l into the next slot of the ring (rtr::TileListRing).
  void build_tile_lists_ahead(const rtk::TraceParams& p_band) {
    const uint64_t m = lists.build_ahead();                            // this build's index
    rtk::TraceParams q = p_band;
    lists.attach(q, row0, true);
    const uint32_t sr = split_row(rows);
    // (counted by every 32nd build only: the atomics and the publishing kernel cost 3.5 us per step when every build has
    //  them -- and nothing to decide when the mode is pinned)
    if (sr != 0u && d_half_cost.get() != nullptr && env.row_interleave < 0 && (m % 32u) == 0u) { q.half_cost = d_half_cost.get(); q.cost_split_brow = sr / 8u; }
    int kind = -1;
    HIP_CHECK(rtk::launch_tile_lists(q, fma, stream_l, &kernels, lists.ready_event(), &kind));   // list_ready: the build kernel's stop event
    ++calls.launches;
    if (kind >= 0) ++list_builds[kind];
    lists.built();
    if (q.half_cost != nullptr) { HIP_CHECK(rtk::launch_publish_half_cost(d_half_cost.get(), h_half_cost.get(), stream_l)); ++calls.launches; }   // (behind list_ready: nobody waits for it)
  }

  // One synchronous launch of `p` on the primary stream, its lists built in-stream into the current slot (the
  // instrumented launches of rt_tracer_trace_stats and rt_dbg_trace_timeline).
  void launch_instrumented(rtk::TraceParams& p, uint32_t samples) {
    const rtk::TracePath path = trace_path(p);
    { std::lock_guard<std::recursive_mutex> lk(order_mu); settle(); debt.key.reset(); }   // (it rebuilds the lists in place and advances every state)
    bool have_lists = false;
    (void)prepare_tile_lists(p, path, true, have_lists);
    sync_list_stream();
    lists.attach(p, row0, have_lists);
    if (have_lists) {
      int kind = -1;
      HIP_CHECK(rtk::launch_tile_lists(p, fma, main_stream(), &kernels, nullptr, &kind));
      std::lock_guard<std::recursive_mutex> lk(order_mu);
      if (kind >= 0) ++list_builds[kind];
    }
    attach_macro_lists(p, path, 0, main_stream());
    {
      std::lock_guard<std::recursive_mutex> lk(order_mu);
      words.take(p);
      HIP_CHECK(rtk::launch_trace(p, fma, filter, path, pick_k(samples), main_stream(), &kernels));
    }
    HIP_CHECK(hipStreamSynchronize(main_stream()));
  }

  // Macro level of the classification (scenes that do not fit the per-wave list): sizes the
  // lists, points the launch at them and runs macro_bin_kernel on the stream ahead of the trace
  // launch.  Every launch re-bins (the camera may have changed; the pass costs N x macro tiles tests).
  // Like the small scenes' tile lists the macro lists depend on camera, scene and frame only: a launch re-bins when one of
  // them changed since the lists of this half were built (HalfLists::macro_key) -- or when it is the first launch of a Trace
  // and the lists are not kept across Traces (bench.py's headline: every step bins afresh) -- and reads the kept lists
  // otherwise (accumulating launches of a progressive Trace: macro_bin_kernel is 0.15 ms per half at C4, 7 % of a launch).
  // (Growing a buffer frees the old one first: hipFree waits for the device, safe while the other half runs.)
  void attach_macro_lists(rtk::TraceParams& p, rtk::TracePath path, int half, hipStream_t st, bool first_launch_of_trace = true) {
    p.macro_lists = nullptr;
    if (!macro || path == rtk::TracePath::FullScan || path == rtk::TracePath::SmallLists) return;
    rtr::HalfLists& h = half_lists[half];
    p.macro_w = kMacroW; p.macro_h = kMacroH;
    p.macro_nx = (p.W + p.macro_w - 1u) / p.macro_w;
    const uint32_t ny = (p.rows + p.macro_h - 1u) / p.macro_h;
    p.macro_cap = p.n_tris < kMacroCapMax ? p.n_tris : kMacroCapMax;
    if (env.macro_cap > 0 && static_cast<uint32_t>(env.macro_cap) < p.macro_cap) p.macro_cap = static_cast<uint32_t>(env.macro_cap);   // tests: force the overflow fallback
    if (h.macro.ensure(static_cast<size_t>(p.macro_nx) * ny * (p.macro_cap + 1u))) h.macro_key.reset();
    p.macro_lists = h.macro.get();
    p.super_lists = nullptr; p.macro_bounds = nullptr; p.super_f = 0u; p.super_chunks = 0u; p.super_nx = 0u;
    const uint32_t chunks = (p.n_tris + rtk::kSuperChunk - 1u) / rtk::kSuperChunk;
    if (super_level && p.n_tris >= kSuperMinTris && chunks <= rtk::kSuperMaxChunks && p.macro_nx * ny > kSuperF * kSuperF) {
      p.super_f = kSuperF; p.super_chunks = chunks;
      p.super_nx = (p.macro_nx + kSuperF - 1u) / kSuperF;
      const size_t sw = static_cast<size_t>(p.super_nx) * ((ny + kSuperF - 1u) / kSuperF) * chunks * (rtk::kSuperChunk + 1u) +
                        static_cast<size_t>(p.macro_nx) * ny * 8u;      // + the macro tiles' focal boxes behind the lists
      if (h.super.ensure(sw)) h.macro_key.reset();
      p.super_lists = h.super.get();
      p.macro_bounds = reinterpret_cast<float*>(h.super.get() + (sw - static_cast<size_t>(p.macro_nx) * ny * 8u));
    }
    const rtr::ListKey k = make_key(p, p.macro_cap * 65536u + p.macro_w * 256u + p.macro_h);
    const bool same = rtr::same_key(h.macro_key, k) && !(first_launch_of_trace && !reuse_across_traces);
    if (!same) {
      h.macro_key = k;
      if (p.super_lists != nullptr) HIP_CHECK(rtk::launch_super_bin(p, fma, st));
      HIP_CHECK(rtk::launch_macro_bin(p, fma, st));
    }
    attach_wave_lists(p, path, h, st, !same);
  }

  // Dense scenes with the per-sample forms: the tiles' candidate lists (forms + triangle index, 64 bytes per candidate) live in HBM,
  // built by wave_lists_kernel behind the macro lists -- same key, same reuse rule -- and read by dense_trace_kernel through the
  // scalar cache (rt_dense.hpp).  Sized for the list capacity, (1 + cap) x 64 bytes per tile: 0.7 GB for a 4K frame at cap 84
  // (what a launch touches is the survivors: ~75 MB at C4); frames whose lists would exceed kWaveListsMaxBytes per half
  // and instrumented launches keep the classification inside the trace kernel (trace_path).
  static constexpr size_t kWaveListsMaxBytes = size_t(6) << 30;
  static size_t wave_list_tiles(const rtk::TraceParams& p) { return static_cast<size_t>((p.W + 31u) / 32u) * ((p.rows + 7u) / 8u) * 4u; }
  static size_t wave_list_words(const rtk::TraceParams& p) { return wave_list_tiles(p) * (1u + p.bin_list) * 16u; }
  void attach_wave_lists(rtk::TraceParams& p, rtk::TracePath path, rtr::HalfLists& h, hipStream_t st, bool macro_rebuilt) {
    p.wave_lists = nullptr; p.wave_cap = 0u;
    if (macro_rebuilt) h.wave_valid = false;                            // (also when this launch does not use them: they follow the macro lists' key)
    if (path != rtk::TracePath::DenseLists) return;
    if (h.wave.ensure(wave_list_words(p))) h.wave_valid = false;
    p.wave_lists = h.wave.get(); p.wave_cap = p.bin_list;
    if (!h.wave_valid) {
      HIP_CHECK(rtk::launch_wave_lists(p, fma, st));
      h.wave_valid = true; h.wave_cap = p.bin_list; h.wave_tiles = wave_list_tiles(p);
    }
  }

  // Which kernel the (half-)launch `p` runs: the one place that decides it.  Evaluated per half: a half's rows decide whether
  // its wave lists fit.  (p.pretest_on, params(): the forms need the filter, binning, pretest and 4 096 ... 50 000 triangles.)
  rtk::TracePath trace_path(const rtk::TraceParams& p) const {
    if (!bin) return rtk::TracePath::FullScan;
    if (p.n_tris <= p.bin_list) return rtk::TracePath::SmallLists;
    if (!p.pretest_on || !filter) return rtk::TracePath::Classify;
    if (p.stats != nullptr || !macro || wave_list_words(p) * sizeof(uint32_t) > kWaveListsMaxBytes) return rtk::TracePath::ClassifyForms;
    return rtk::TracePath::DenseLists;
  }

  static constexpr int kWindow = 4;

  // Device-resident form of one Trace (rt_tracer_trace_enqueue): clear + iterationCount launches + conversion,
  // all enqueued, no callbacks, no host synchronisation.  `target`: second BGRA8 destination of the emitting
  // launch (the caller's mirror or a gather buffer), or null.
  void trace_enqueue_body(uint32_t iterationCount, uint32_t samplesPerIteration, uint32_t* target) {
    use_device();
    if (iterationCount == 0) {
      clear_accumulators();
      convert();
      if (target) copy_image_to(target);
      return;
    }
    const uint32_t group = fused_iterations(samplesPerIteration);
    for (uint32_t i = 0; i < iterationCount;) {
      const uint32_t n = iterationCount - i < group ? iterationCount - i : group;
      const bool last = i + n == iterationCount;
      enqueue_trace_launch(samplesPerIteration, (i == 0 ? rtk::TRACE_ZERO_ACC : 0u) | (last ? rtk::TRACE_EMIT_IMAGE : 0u),
                           0, n, last ? target : nullptr);
      i += n;
    }
  }

  // RayTracerImpl::TraceFunct, RayTracerImpl.cu:236-315 (runs on the render thread)
  // How many consecutive iterations one launch may run (1 = no fusing): bounded so that a launch
  // stays short (<= 64 samples per pixel) and a Stop() takes effect within a few launches.
  uint32_t fused_iterations(uint32_t samplesPerIteration) {
    if (samplesPerIteration == 0u || !rtk::trace_can_fuse(trace_path(params(samplesPerIteration)), filter)) return 1u;
    const uint32_t n = 64u / samplesPerIteration;
    return n < 1u ? 1u : n;
  }

  void trace_funct(uint32_t iterationCount, uint32_t samplesPerIteration, uint32_t updateInterval) {
    try {
      use_device();
      bool cleared = false;                                              // :242-243, fused into launch 0
      // Update hand-off, pipelined: the launch that ends at an update point writes the BGRA8 image
      // into one of two pinned host images itself; its callback runs after the NEXT launch has been
      // enqueued, i.e. while the GPU is already tracing again (the reference converts, copies and
      // calls back with the GPU idle, :259-272).  An update whose iteration ran is always delivered,
      // also when Stop() arrives meanwhile, as in the reference's loop order.
      struct { bool due = false; uint32_t* image = nullptr; rt_callback_fn cb = nullptr; void* user = nullptr; } pend;
      auto deliver = [&] {
        if (!pend.due) return;
        HIP_CHECK(hipEventSynchronize(handoff_event));                   // :259
        pend.cb(pend.image, static_cast<size_t>(npix()) * sizeof(uint32_t), pend.user);   // :272
        pend.due = false;
      };
      uint32_t* final_image = h_image.get();
      uint32_t i = 0;
      while (!stopped && i < iterationCount) {                           // :246
        rt_callback_fn cb; void* user;
        { std::lock_guard<std::mutex> lk(state_mu); cb = update_cb; user = update_user; }
        auto is_update = [&](uint32_t k) { return cb != nullptr && k > 0 && updateInterval > 0 && k % updateInterval == 0; };   // :256
        // Iterations nobody observes in between -- up to the next update point or the end of the
        // Trace -- run as ONE launch (fused_iterations(): bit-identical to separate launches).
        const uint32_t last_allowed = iterationCount - 1u - i < fused_iterations(samplesPerIteration) - 1u
                                          ? iterationCount - 1u : i + fused_iterations(samplesPerIteration) - 1u;
        uint32_t e = i;                                                  // last iteration of this launch
        while (e < last_allowed && !is_update(e)) ++e;
        const bool update = is_update(e);
        const bool emit = update || e + 1 == iterationCount;
        const uint32_t flags = (cleared ? 0u : rtk::TRACE_ZERO_ACC) | (emit ? rtk::TRACE_EMIT_IMAGE : 0u);
        uint32_t* const target = emit ? (handoff_next ? h_image_alt : h_image).get() : nullptr;
        if (emit && pend.due && pend.image == target) deliver();         // never overwrite an image still to be handed out
        // The reference blocks on every launch (:228), which makes a stop take effect after one
        // kernel.  Here up to `kWindow` sampled launches are in flight: the host never starves the
        // GPU on short launches, and a stop still takes effect within a few launches.
        // (not split over two streams: the update hand-off is an ordering point for both halves anyway,
        //  and fused launches have no drain between their iterations: measured 18.6 vs 20.3 us per iteration)
        enqueue_trace_launch(samplesPerIteration, flags, kWindow, e - i + 1u, target, false);   // :249
        cleared = true;
        deliver();                                                       // the previous update, while this launch runs
        if (emit) { final_image = target; handoff_next ^= 1; }
        if (update) {
          HIP_CHECK(hipEventRecord(handoff_event, main_stream()));
          pend.due = true; pend.image = target; pend.cb = cb; pend.user = user;
        }
        i = e + 1u;
      }
      deliver();
      clock.drain();
      if (!cleared) {                                                    // no launch ran: plain clear (+ convert below)
        clear_accumulators();
        if (!stopped) convert();
      }
      if (stopped) { HIP_CHECK(hipStreamSynchronize(main_stream())); return; }   // :280-284, no callback
      if (cleared && i == iterationCount) {
        sync_polling(main_stream());                                     // the last launch wrote final_image itself
      } else {
        fetch_image();                                                   // :287-295 (no launch ran)
        final_image = h_image.get();
      }
      completed = true;
      rt_callback_fn cb; void* user;
      { std::lock_guard<std::mutex> lk(state_mu); cb = finished_cb; user = finished_user; }
      if (cb != nullptr) cb(final_image, static_cast<size_t>(npix()) * sizeof(uint32_t), user);   // :302-305
    } catch (const rtr::HipFail& f) {                                    // :307-314 swallowed, but recorded
      set_error(f.what);
    } catch (...) {
      set_error("unknown failure in the render thread");
    }
  }
};

#include "rt_multi.hpp"

namespace rtr {

// runs an entry point's body: a failure becomes the tracer's (or the process's) error text and an RT_ERR_* code
template <class F>
int guarded(rt_tracer* t, F&& f) {
  auto fail = [t](const std::string& why, int rc) { if (t) t->set_error(why); else set_global_error(why); return rc; };
  try {
    f();
    return RT_OK;
  } catch (const BadArgument& e) {
    return fail(e.what, RT_ERR_INVALID);
  } catch (const HipFail& e) {
    return fail(e.what, RT_ERR_HIP);
  } catch (const std::exception& e) {
    return fail(e.what(), RT_ERR_STATE);
  } catch (...) {
    return fail("unknown failure", RT_ERR_STATE);
  }
}

// an entry point's body on a handle: its API calls serialised, the render thread idle (RayTracerImpl.cu:72-77)
template <class F>
int exclusive(rt_tracer* t, F&& f) {
  std::lock_guard<std::mutex> lk(t->api_mu);
  return guarded(t, [&] { t->cancel_and_join(); f(); });
}

int require_device(int device);               // RT_OK, or RT_ERR_* with the process's error text set
void multi_push_camera(rt_tracer* t);         // rt_multi_api.hpp

}  // namespace rtr
