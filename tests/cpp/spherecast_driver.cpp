// Drives rt::RayTracer::SphereCast (include/RayTracer/RayTracer.h) from a scene file and a sweep file and prints every answer,
// for tests/test_cpp_spherecast.py to compare with the Python class's.
//   spherecast_driver scene.f4 sweeps.f4 [accel]      scene: rows of 4 floats (3 per triangle); sweeps: o xyz, d xyz, r, tmax
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "RayTracer/RayTracer.h"

static std::vector<float> load(const char* path) {
  std::vector<float> v;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  float buf[1024];
  size_t n;
  while ((n = std::fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: spherecast_driver scene.f4 sweeps.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), sweeps = load(argv[2]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 3 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<rt_hit> hits;
  if (!tracer.SphereCast(sweeps, hits)) { std::printf("SPHERECAST_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (const rt_hit& h : hits) std::printf("SWEEP %d %08x %08x %08x\n", h.prim, bits(h.t), bits(h.u), bits(h.v));
  const std::vector<rt_hit> again = tracer.SphereCast(sweeps);           // the returning form
  if (again.size() != hits.size() || std::memcmp(again.data(), hits.data(), hits.size() * sizeof(rt_hit)) != 0) {
    std::printf("RETURNING_FORM_DIFFERS\n");
    return 1;
  }
  std::vector<rt_hit> bad(1);
  std::vector<float> misfit(sweeps.begin(), sweeps.end() - 1);
  if (tracer.SphereCast(misfit, bad) || bad.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
