// Drives rt::RayTracer::SignedDistance and ClosestSides (include/RayTracer/RayTracer.h) from a scene file and a point file
// and prints every answer in hexadecimal floats, for tests/test_cpp_signed.py to compare with the Python class's bits.
//   signed_driver scene.f4 points.f4 [accel]      scene: rows of 4 floats (3 per triangle); points: x, y, z, d2max
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
  if (argc < 3) { std::printf("usage: signed_driver scene.f4 points.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), pts = load(argv[2]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 3 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<rt_hit> hits;
  std::vector<rt_side> sides;
  if (!tracer.SignedDistance(pts, hits, sides)) { std::printf("SIGNED_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < hits.size(); ++i)
    std::printf("SIGNED %d %a %a %a %d %a\n", hits[i].prim, hits[i].t, hits[i].u, hits[i].v, sides[i].feature, sides[i].s);
  const std::vector<rt_side> again = tracer.SignedDistance(pts);
  if (again.size() != sides.size() || std::memcmp(again.data(), sides.data(), sides.size() * sizeof(rt_side)) != 0) {
    std::printf("RETURNING_FORM_DIFFERS\n");
    return 1;
  }

  std::vector<rt_hit> rows4;
  std::vector<uint32_t> counts;
  std::vector<rt_side> sides4;
  if (!tracer.ClosestAll(pts, 4, rows4, counts) || !tracer.ClosestSides(pts, rows4, sides4)) {
    std::printf("SIDES_FAILED %s\n", tracer.LastError().c_str());
    return 1;
  }
  for (size_t j = 0; j < sides4.size(); ++j) std::printf("SIDE %d %d %a\n", rows4[j].prim, sides4[j].feature, sides4[j].s);
  std::vector<rt_side> bad(1);
  rows4.pop_back();
  if (tracer.ClosestSides(pts, rows4, bad) || bad.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
