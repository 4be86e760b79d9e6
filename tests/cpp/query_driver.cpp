// Ray queries through the C++ class (include/RayTracer/RayTracer.h): Pick and FocusAt on a fixed scene, results printed
// as hex floats for tests/test_gpu_query.py to compare with the Python API.
//   query_driver [strict]   -> lines "PICK x y prim t u v", "RAY x y ox oy oz dx dy dz", "FOCUS x y ok f"
#include <cstdio>
#include <cstring>
#include <vector>

#include "RayTracer/RayTracer.h"

int main(int argc, char** argv) {
  rt_options opt;
  std::memset(&opt, 0, sizeof opt);
  opt.struct_size = sizeof opt;
  opt.seed = 3;
  opt.math_mode = (argc > 1 && std::strcmp(argv[1], "strict") == 0) ? RT_MATH_STRICT : RT_MATH_FMA;
  rt::RayTracer tracer(math::uvec2(64, 48), math::vec3(0, 0, 0), math::vec2(0.1f, -0.05f), 60.0f, 10.0f, 0.5f, &opt);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float4> scene = {                        // a quad at z = -6 and a triangle in front of it
      make_float4(-2, -2, -6, 0), make_float4(2, -2, -6, 0), make_float4(-2, 2, -6, 0),
      make_float4(2, -2, -6, 0), make_float4(2, 2, -6, 0), make_float4(-2, 2, -6, 0),
      make_float4(-0.5f, -0.5f, -3, 0), make_float4(0.5f, -0.5f, -3, 0), make_float4(0, 0.5f, -3, 0)};
  tracer.UploadScene(scene);
  const uint32_t px[][2] = {{0, 0}, {32, 24}, {31, 20}, {10, 40}, {63, 47}, {50, 5}};
  for (const auto& p : px) {
    rt_hit h;
    math::vec3 ray[2];
    if (!tracer.Pick(math::uvec2(p[0], p[1]), h, ray)) { std::printf("PICK_FAILED %s\n", tracer.LastError().c_str()); return 1; }
    std::printf("PICK %u %u %d %a %a %a\n", p[0], p[1], h.prim, h.t, h.u, h.v);
    std::printf("RAY %u %u %a %a %a %a %a %a\n", p[0], p[1], ray[0].x, ray[0].y, ray[0].z, ray[1].x, ray[1].y, ray[1].z);
  }
  rt_hit h;
  if (tracer.Pick(math::uvec2(64, 0), h)) { std::printf("PICK_OUTSIDE_ACCEPTED\n"); return 1; }
  for (const auto& p : {px[1], px[0]}) {
    float f = 0.0f;
    const bool ok = tracer.FocusAt(math::uvec2(p[0], p[1]), &f);
    std::printf("FOCUS %u %u %d %a\n", p[0], p[1], ok ? 1 : 0, f);
  }
  std::vector<math::vec3> rays = {math::vec3(0, 0, 0), math::vec3(0, 0, -1), math::vec3(1.5f, 1.5f, 0), math::vec3(0, 0, -1)};
  std::vector<rt_hit> hits;
  if (!tracer.Intersect(rays, hits) || hits.size() != 2) { std::printf("INTERSECT_FAILED\n"); return 1; }
  for (const rt_hit& x : hits) std::printf("HIT %d %a %a %a\n", x.prim, x.t, x.u, x.v);
  return 0;
}
