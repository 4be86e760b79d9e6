// Drives rt::RayTracer::Exposure (include/RayTracer/RayTracer.h) from a scene file, a point file and a direction file and
// prints every mask in hexadecimal, for tests/test_cpp_exposure.py to compare with the Python class's bits.
//   exposure_driver scene.f4 points.f4 dirs.f4 [accel]
//   scene: rows of 4 floats (3 per triangle); points: origin, normal, tmin, tmax; dirs: x, y, z, w
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

int main(int argc, char** argv) {
  if (argc < 4) { std::printf("usage: exposure_driver scene.f4 points.f4 dirs.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), pts = load(argv[2]), dirs = load(argv[3]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 4 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<uint64_t> masks;
  if (!tracer.Exposure(pts, dirs, masks)) { std::printf("EXPOSURE_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < masks.size(); ++i) std::printf("LOCAL %016llx\n", static_cast<unsigned long long>(masks[i]));
  if (tracer.Exposure(pts, dirs) != masks) { std::printf("RETURNING_FORM_DIFFERS\n"); return 1; }
  const std::vector<uint64_t> world = tracer.Exposure(pts, dirs, true);
  if (world.size() != masks.size()) { std::printf("WORLD_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < world.size(); ++i) std::printf("WORLD %016llx\n", static_cast<unsigned long long>(world[i]));
  // the class's own direction set, as the command line uses it
  const std::vector<uint64_t> own = tracer.Exposure(pts, rt::RayTracer::HemisphereDirections(48));
  if (own.size() != masks.size()) { std::printf("OWN_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < own.size(); ++i) std::printf("OWN %016llx\n", static_cast<unsigned long long>(own[i]));
  std::vector<uint64_t> bad(1, 9u);
  std::vector<float> misfit(pts.begin(), pts.end() - 1);
  if (tracer.Exposure(misfit, dirs, bad) || bad.size() != 1 || bad[0] != 9u) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
