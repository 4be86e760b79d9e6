// Drives rt::RayTracer::OverlapHexahedra (include/RayTracer/RayTracer.h) from a scene file and a file of regions and
// prints every answer, for tests/test_cpp_hexoverlap.py to compare with the Python class's.
//   hexoverlap_driver scene.f4 hexa.f4 [accel]    scene: rows of 4 floats (3 per triangle); hexa: eight rows C_k xyz, - per region
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
  if (argc < 3) { std::printf("usage: hexoverlap_driver scene.f4 hexa.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), hexa = load(argv[2]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 3 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<int32_t> prims;
  std::vector<uint32_t> counts;
  if (!tracer.OverlapHexahedra(hexa, 4, prims, counts)) { std::printf("OVERLAP_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < counts.size(); ++i)
    std::printf("OVERLAP %u %d %d %d %d\n", counts[i], prims[4 * i], prims[4 * i + 1], prims[4 * i + 2], prims[4 * i + 3]);
  const std::vector<uint32_t> again = tracer.OverlapHexahedra(hexa);   // the returning form: counts only
  if (again != counts) { std::printf("RETURNING_FORM_DIFFERS\n"); return 1; }

  std::vector<int32_t> after(counts.size()), page;                       // the next page of every query
  for (size_t i = 0; i < after.size(); ++i) after[i] = prims[4 * i + 3];
  std::vector<uint32_t> left;
  if (!tracer.OverlapHexahedra(hexa, 2, page, left, after)) { std::printf("CURSOR_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < left.size(); ++i) std::printf("PAGE %u %d %d\n", left[i], page[2 * i], page[2 * i + 1]);

  std::vector<int32_t> bad(1);
  after.pop_back();
  if (tracer.OverlapHexahedra(hexa, 2, bad, left, after) || bad.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
