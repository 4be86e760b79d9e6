// Drives rt::RayTracer::TriangleDistance (include/RayTracer/RayTracer.h) from a scene file and a file of query triangles and
// prints every answer bit for bit, for tests/test_cpp_tridistance.py to compare with the Python class's.
//   tridistance_driver scene.f4 tris.f4 [accel]    scene: rows of 4 floats (3 per triangle); tris: P0 xyz, d2max, P1 xyz, -, P2 xyz, -
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

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: tridistance_driver scene.f4 tris.f4 [accel]\n"); return 2; }
  rt::RayTracer tracer(math::uvec2(32, 24), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);
  if (!tracer.Valid()) { std::printf("CREATE_FAILED %s\n", tracer.LastError().c_str()); return 2; }
  const std::vector<float> rows = load(argv[1]), tris = load(argv[2]);
  std::vector<float4> scene(rows.size() / 4);
  std::memcpy(scene.data(), rows.data(), scene.size() * sizeof(float4));
  tracer.UploadScene(scene);
  if (argc > 3 && !tracer.SetQueryAcceleration(true)) { std::printf("ACCEL_FAILED %s\n", tracer.LastError().c_str()); return 1; }

  std::vector<rt_hit> hits;
  std::vector<rt_witness> witness;
  if (!tracer.TriangleDistance(tris, hits, witness)) { std::printf("DISTANCE_FAILED %s\n", tracer.LastError().c_str()); return 1; }
  for (size_t i = 0; i < hits.size(); ++i)
    std::printf("DISTANCE %d %08x %08x %08x %d %08x %08x %08x\n", hits[i].prim, bits(hits[i].t), bits(hits[i].u), bits(hits[i].v),
                witness[i].where, bits(witness[i].x), bits(witness[i].y), bits(witness[i].z));
  const std::vector<rt_hit> again = tracer.TriangleDistance(tris);       // the returning form
  if (again.size() != hits.size() || std::memcmp(again.data(), hits.data(), hits.size() * sizeof(rt_hit)) != 0) { std::printf("RETURNING_FORM_DIFFERS\n"); return 1; }

  std::vector<float> odd(tris.begin(), tris.end() - 1);
  std::vector<rt_hit> kept(1);
  if (tracer.TriangleDistance(odd, kept, witness) || kept.size() != 1) { std::printf("MISFIT_ACCEPTED\n"); return 1; }
  return 0;
}
