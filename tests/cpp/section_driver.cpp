// Drives rt::RayTracer::Section and SectionSegments (include/RayTracer/RayTracer.h) from a scene file and a file of planes and
// prints every answer, for tests/test_cpp_section.py to compare with the Python class's.
//   section_driver scene.f4 planes.f4 [accel]
// scene: rows of 4 floats (3 per triangle); planes: nx ny nz d0 d1 - - - per plane or slab
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "RayTracer/RayTracer.h"

static_assert(sizeof(rt_cut) == 32, "rt_cut is 32 bytes");

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

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: section_driver scene.f4 planes.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), planes = load(argv[2]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 3 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<int32_t> prims;
  std::vector<uint32_t> counts;
  if (!tracer.Section(planes, 4, prims, counts)) { std::printf("SECTION_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < counts.size(); ++i)
    std::printf("SECTION %u %d %d %d %d\n", counts[i], prims[4 * i], prims[4 * i + 1], prims[4 * i + 2], prims[4 * i + 3]);
  if (tracer.Section(planes, 0) != counts) { std::printf("RETURNING_FORM_DIFFERS\n"); return 1; }   // the returning form: counts only

  for (uint32_t side = 0; side < 2; ++side) {                            // the cuts of every row, bit for bit (floats as hex words)
    std::vector<rt_cut> cuts;
    if (!tracer.SectionSegments(planes, prims, 4, side, cuts)) { std::printf("SEGMENTS_FAILED %s\n", tracer.LastError().c_str()); return 1; }
    for (size_t j = 0; j < cuts.size(); ++j)
      std::printf("CUT %u %d %d %08x %08x %08x %08x %08x %08x\n", side, cuts[j].kind, cuts[j].features, bits(cuts[j].p0[0]), bits(cuts[j].p0[1]),
                  bits(cuts[j].p0[2]), bits(cuts[j].p1[0]), bits(cuts[j].p1[1]), bits(cuts[j].p1[2]));
  }

  std::vector<int32_t> after(counts.size()), page;                       // the next page of every plane
  for (size_t i = 0; i < after.size(); ++i) after[i] = prims[4 * i + 3];
  std::vector<uint32_t> left;
  if (!tracer.Section(planes, 2, page, left, after)) { std::printf("CURSOR_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < left.size(); ++i) std::printf("PAGE %u %d %d\n", left[i], page[2 * i], page[2 * i + 1]);

  std::vector<int32_t> bad(1);
  std::vector<rt_cut> kept(1);
  after.pop_back();
  if (tracer.Section(planes, 2, bad, left, after) || bad.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  if (tracer.SectionSegments(planes, prims, 3, 0, kept) || tracer.SectionSegments(planes, prims, 0, 0, kept) || kept.size() != 1) {
    std::printf("SEGMENT_MISFIT_ACCEPTED\n");
    return 1;
  }
  if (tracer.SectionSegments(planes, prims, 4, 2, kept) || kept.size() != 1 || tracer.LastError().find("side") == std::string::npos) {
    std::printf("SIDE_2_ACCEPTED\n");
    return 1;
  }
  return 0;
}
