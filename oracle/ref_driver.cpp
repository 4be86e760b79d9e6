// ref_driver.cpp -- a C ABI over the REFERENCE'S OWN kernel text, compiled for the CPU (oracle/_ref/libref.so).
//
// TEST INFRASTRUCTURE, NOT PRODUCT CODE, and not the oracle either: this file holds no restatement of what the
// reference computes per pixel.  `#include "Kernels.cuh"` below is the reference's RayTracer/Kernels.cuh, unmodified,
// found through links that oracle/Makefile's `ref` target makes at build time; with it come ThinLensCamera.cuh, Ray.cuh,
// Random.cuh, DeviceUtils.cuh, Common/Math.h, Common/Color.h and Common/Sptr.h.  They compile as host C++ against the
// stand-in headers of oracle/ref_shim/ (CUDA built-ins, cuRAND's XORWOW, the glm subset), and rt::TraceKernel and
// rt::ConverterKernel are then called as plain functions, once per thread of the grid.
//
// What this driver has to write itself, because RayTracer/Random.cu and RayTracer/RayTracerImpl.cu cannot be compiled
// (kernel launches in <<< >>>, cudaMalloc, texture objects, a render thread) -- three pieces, each a few lines:
//   1. the grid: 32 x 32 threads per block, ceil(W / 32) x ceil(H / 32) blocks
//      (Random.cu:40-43, RayTracerImpl.cu:191-194 and :207-210);
//   2. the RNG states: curand_init(seed, x + y * W, 0, &state) per pixel (Random.cu:14-29; the body of that kernel is
//      these lines).  The reference seeds with time(nullptr) (Random.cu:45); the seed is a parameter here, and a resize
//      creates the states again from the same seed (RayTracerImpl.cu:94-103 calls random::CreateStates again);
//   3. the order of a trace: clear the render and the sample-count buffer, run the trace kernel `iterations` times with
//      `samples` each, convert (RayTracerImpl.cu:242-243, :246-249, :295: TraceFunct without its callbacks and its stop flag),
//      with ChannelCount() = 4 (RayTracerImpl.cuh) and buffers of W * H * 4 floats, W * H counts, W * H colours.
// The camera is the reference's own rt::ThinLensCamera object: construction, Rotate and the three setters
// (RayTracerImpl.cu:28, :105-117) are its code.  UploadScene's size check (:121-125) is restated in ref_upload.
//
// Stand-ins whose arithmetic is NOT the reference's text: glm (oracle/ref_shim/glm/glm.hpp), cuRAND
// (oracle/ref_shim/curand_kernel.h, oracle/ref_xorwow.cpp) and sin / cos / tan (libm, or whatever ref_set_trig installs).
// DESIGN.md section 2 lists them.
//
// The order of the includes matters: the reference has a `namespace random`, which collides with libc's random() once
// <cstdlib> is in; so every system header comes first, then `random` is renamed for the reference's text alone.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "cuda_runtime.h"
#include "curand_kernel.h"
#include "glm/glm.hpp"

#define random ref_random
#include "Kernels.cuh"
#undef random

thread_local dim3 blockIdx, blockDim, threadIdx;
thread_local unsigned int ref_shim::tex_width = 0;

// ---------------------------------------------------------------------------------------------------- sin / cos / tan
namespace {
typedef void (*sincos_fn_t)(float, float*, float*);
sincos_fn_t g_sincos = nullptr;

float libm_sin(float x) { return std::sin(x); }
float libm_cos(float x) { return std::cos(x); }
float libm_tan(float x) { return std::tan(x); }
float installed_sin(float x) {
  float s, c;
  g_sincos(x, &s, &c);
  return s;
}
float installed_cos(float x) {
  float s, c;
  g_sincos(x, &s, &c);
  return c;
}
// tan as the quotient of the installed pair: DESIGN.md section 2 defines the build-owned tan(fov / 2) so
float installed_tan(float x) {
  float s, c;
  g_sincos(x, &s, &c);
  return s / c;
}
}  // namespace

float (*ref_shim::sin_fn)(float) = libm_sin;
float (*ref_shim::cos_fn)(float) = libm_cos;
float (*ref_shim::tan_fn)(float) = libm_tan;

// ---------------------------------------------------------------------------------------------------- the tracer
namespace {

struct Tracer {
  math::uvec2 size;
  uint64_t seed;
  rt::ThinLensCamera camera;
  std::vector<float> render;           // W * H * 4
  std::vector<uint32_t> counts;        // W * H
  std::vector<rt::Color> image;        // W * H
  std::vector<curandState_t> states;   // W * H
  std::vector<float4> scene;           // 3 rows per triangle
  uint32_t n_triangles = 0;

  Tracer(uint32_t W, uint32_t H, const float* pos, const float* angles, float fov, float focal, float aperture, uint64_t seed_)
      : size(W, H), seed(seed_),
        camera(math::vec3(pos[0], pos[1], pos[2]), math::vec2(angles[0], angles[1]), fov, focal, aperture) {
    create_buffers();
  }

  // piece 1: one call of `thread` per thread of the reference's grid, blockIdx / blockDim / threadIdx set as CUDA would
  template <class F>
  void for_each_thread(F thread) const {
    blockDim = dim3{32u, 32u, 1u};
    const unsigned int gx = static_cast<unsigned int>(std::ceil(size.x / static_cast<float>(blockDim.x)));
    const unsigned int gy = static_cast<unsigned int>(std::ceil(size.y / static_cast<float>(blockDim.y)));
    for (unsigned int by = 0; by < gy; ++by)
      for (unsigned int bx = 0; bx < gx; ++bx) {
        blockIdx = dim3{bx, by, 0u};
        for (unsigned int ty = 0; ty < blockDim.y; ++ty)
          for (unsigned int tx = 0; tx < blockDim.x; ++tx) {
            threadIdx = dim3{tx, ty, 0u};
            thread();
          }
      }
  }

  void create_buffers() {
    const size_t n = static_cast<size_t>(size.x) * size.y;
    render.assign(n * 4, 0.0f);
    counts.assign(n, 0u);
    image.assign(n, 0u);
    states.assign(n, curandState_t{});
    // piece 2
    for_each_thread([this] {
      const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
      if (x >= size.x || y >= size.y) return;
      const size_t offset = x + static_cast<size_t>(y) * size.x;
      curand_init(seed, offset, 0, &states[offset]);
    });
  }

  void convert() {
    for_each_thread([this] { rt::ConverterKernel(size, 4u, render.data(), counts.data(), image.data()); });
  }

  // piece 3
  void trace(uint32_t iterations, uint32_t samples) {
    std::fill(render.begin(), render.end(), 0.0f);
    std::fill(counts.begin(), counts.end(), 0u);
    ref_shim::tex_width = static_cast<unsigned int>(scene.size());
    for (uint32_t i = 0; i < iterations; ++i)
      for_each_thread([this, samples] {
        rt::TraceKernel(render.data(), counts.data(), size, 4u, camera, samples, states.data(), scene.data(), n_triangles);
      });
    convert();
  }
};

}  // namespace

extern "C" {

// sincos == nullptr: libm's sinf, cosf and tanf.  Otherwise glm::sin and glm::cos -- those inside glm::angleAxis too -- return
// the function's two results, and glm::tan their quotient.
void ref_set_trig(sincos_fn_t sincos) {
  g_sincos = sincos;
  ref_shim::sin_fn = sincos ? installed_sin : libm_sin;
  ref_shim::cos_fn = sincos ? installed_cos : libm_cos;
  ref_shim::tan_fn = sincos ? installed_tan : libm_tan;
}

void* ref_create(uint32_t W, uint32_t H, const float position[3], const float angles[2], float fov, float focal, float aperture,
                 uint64_t seed) {
  if (W == 0 || H == 0) return nullptr;
  return new Tracer(W, H, position, angles, fov, focal, aperture, seed);
}

void ref_destroy(void* h) { delete static_cast<Tracer*>(h); }

// rows: n_rows float4, three absolute vertices per triangle.  Returns 0 and keeps the previous scene where UploadScene
// logs and returns (RayTracerImpl.cu:121-125).
int ref_upload(void* h, const float* rows, uint32_t n_rows) {
  Tracer* t = static_cast<Tracer*>(h);
  if (n_rows < 3u || n_rows % 3u != 0u) return 0;
  t->scene.resize(n_rows);
  std::memcpy(t->scene.data(), rows, sizeof(float4) * n_rows);
  t->n_triangles = n_rows / 3u;
  return 1;
}

void ref_trace(void* h, uint32_t iterations, uint32_t samples) { static_cast<Tracer*>(h)->trace(iterations, samples); }

void ref_rotate(void* h, const float angles[2]) { static_cast<Tracer*>(h)->camera.Rotate(math::vec2(angles[0], angles[1])); }

void ref_set_camera_parameters(void* h, float fov, float focal, float aperture) {   // RayTracerImpl.cu:105-112
  Tracer* t = static_cast<Tracer*>(h);
  t->camera.Fov(fov);
  t->camera.FocalLength(focal);
  t->camera.Aperture(aperture);
}

void ref_resize(void* h, uint32_t W, uint32_t H) {                                  // RayTracerImpl.cu:94-103
  Tracer* t = static_cast<Tracer*>(h);
  t->size = math::uvec2(W, H);
  t->create_buffers();
}

void ref_size(void* h, uint32_t wh[2]) {
  const Tracer* t = static_cast<Tracer*>(h);
  wh[0] = t->size.x;
  wh[1] = t->size.y;
}

void ref_read_render(void* h, float* out) {
  const Tracer* t = static_cast<Tracer*>(h);
  std::memcpy(out, t->render.data(), t->render.size() * sizeof(float));
}
void ref_read_counts(void* h, uint32_t* out) {
  const Tracer* t = static_cast<Tracer*>(h);
  std::memcpy(out, t->counts.data(), t->counts.size() * sizeof(uint32_t));
}
void ref_read_image(void* h, uint32_t* out) {
  const Tracer* t = static_cast<Tracer*>(h);
  std::memcpy(out, t->image.data(), t->image.size() * sizeof(uint32_t));
}
void ref_read_states(void* h, uint32_t* out) {                                      // {d, v0..v4} per pixel
  const Tracer* t = static_cast<Tracer*>(h);
  std::memcpy(out, t->states.data(), t->states.size() * sizeof(curandState_t));
}

// probe: rt::HitTriangle (Kernels.cuh:29-65) of ray i = rt::Ray(origin, direction), which normalises the direction
// (Ray.cuh:12-17), against triangle i.  rays: n x 6, tris: n x 9 (v0, v1, v2).  t, u, v start at 0 as in rt::Radiance (:83).
void ref_hit_triangle(uint32_t n, const float* rays, const float* tris, int32_t* hit, float* t, float* u, float* v) {
  for (uint32_t i = 0; i < n; ++i) {
    const float* r = rays + 6 * static_cast<size_t>(i);
    const float* p = tris + 9 * static_cast<size_t>(i);
    const rt::Ray ray(math::vec3(r[0], r[1], r[2]), math::vec3(r[3], r[4], r[5]));
    t[i] = u[i] = v[i] = 0.0f;
    hit[i] = rt::HitTriangle(ray, math::vec3(p[0], p[1], p[2]), math::vec3(p[3], p[4], p[5]), math::vec3(p[6], p[7], p[8]),
                             t[i], u[i], v[i])
                 ? 1
                 : 0;
  }
}

// probe: rt::ThinLensCamera::GetRay (ThinLensCamera.cuh:30-52) of the tracer's camera and frame size for pixel i with
// state i ({d, v0..v4}), which the three draws of the lens sample advance in place.  rays: n x 6 (origin, direction).
void ref_get_ray(void* h, uint32_t n, const uint32_t* pixels, uint32_t* states, float* rays) {
  const Tracer* t = static_cast<Tracer*>(h);
  for (uint32_t i = 0; i < n; ++i) {
    curandState_t s;
    std::memcpy(&s, states + 6 * static_cast<size_t>(i), sizeof s);
    const rt::Ray ray(t->camera.GetRay(math::uvec2(pixels[2 * i], pixels[2 * i + 1]), t->size, s));
    std::memcpy(states + 6 * static_cast<size_t>(i), &s, sizeof s);
    float* out = rays + 6 * static_cast<size_t>(i);
    out[0] = ray.origin().x; out[1] = ray.origin().y; out[2] = ray.origin().z;
    out[3] = ray.direction().x; out[4] = ray.direction().y; out[5] = ray.direction().z;
  }
}

}  // extern "C"
