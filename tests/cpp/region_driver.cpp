// Drives rt::RayTracer::Overlap, OverlapTriangles or OverlapHexahedra (include/RayTracer/RayTracer.h) from a scene file and a
// file of queries and prints every answer, for tests/test_cpp_region.py to compare with the Python class's.
//   region_driver box|tri|hexa scene.f4 queries.f4 [accel]
// scene: rows of 4 floats (3 per triangle); queries: lo xyz, -, hi xyz, - per box; P0 xyz, -, P1 xyz, -, P2 xyz, - per triangle;
// eight rows C_k xyz, - per hexahedron
#include <cstdio>
#include <cstring>
#include <string>
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

// the two forms of one shape's method
using Query = bool (rt::RayTracer::*)(const std::vector<float>&, uint32_t, std::vector<int32_t>&, std::vector<uint32_t>&,
                                      const std::vector<int32_t>&);
using Counts = std::vector<uint32_t> (rt::RayTracer::*)(const std::vector<float>&, uint32_t);

int main(int argc, char** argv) {
  const std::string shape = argc > 1 ? argv[1] : "";
  Query query = nullptr;
  Counts returning = nullptr;
  if (shape == "box") { query = &rt::RayTracer::Overlap; returning = &rt::RayTracer::Overlap; }
  if (shape == "tri") { query = &rt::RayTracer::OverlapTriangles; returning = &rt::RayTracer::OverlapTriangles; }
  if (shape == "hexa") { query = &rt::RayTracer::OverlapHexahedra; returning = &rt::RayTracer::OverlapHexahedra; }
  if (argc < 4 || !query) { std::printf("usage: region_driver box|tri|hexa scene.f4 queries.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[2]), queries = load(argv[3]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 4 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  const std::vector<int32_t> none;
  std::vector<int32_t> prims;
  std::vector<uint32_t> counts;
  if (!(tracer.*query)(queries, 4, prims, counts, none)) { std::printf("OVERLAP_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < counts.size(); ++i)
    std::printf("OVERLAP %u %d %d %d %d\n", counts[i], prims[4 * i], prims[4 * i + 1], prims[4 * i + 2], prims[4 * i + 3]);
  const std::vector<uint32_t> again = (tracer.*returning)(queries, 0);   // the returning form: counts only
  if (again != counts) { std::printf("RETURNING_FORM_DIFFERS\n"); return 1; }

  std::vector<int32_t> after(counts.size()), page;                       // the next page of every query
  for (size_t i = 0; i < after.size(); ++i) after[i] = prims[4 * i + 3];
  std::vector<uint32_t> left;
  if (!(tracer.*query)(queries, 2, page, left, after)) { std::printf("CURSOR_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < left.size(); ++i) std::printf("PAGE %u %d %d\n", left[i], page[2 * i], page[2 * i + 1]);

  std::vector<int32_t> bad(1);
  after.pop_back();
  if ((tracer.*query)(queries, 2, bad, left, after) || bad.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
