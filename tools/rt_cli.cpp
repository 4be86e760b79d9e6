// rt_cli -- headless front end of the trace path: the command line of the reference's wx
// app (OpenGLView/App.cpp:62-184: -w -h -s -i -u -cx -cy -cz -cxa -cya -f -l -a, integer
// values, defaults App.cpp:11-23) without the GUI, plus what a batch run needs: a scene,
// a seed and an output file written with the reference's BMP format (Common/Bitmap.h).
//
//   rt_cli -w 1920 -h 1080 -s 16 -i 1 -f 70 -l 3 --aperture 0.05 --scene cornell32 --seed 1 -o out.bmp
//
// Build: g++ -std=c++17 -Iinclude tools/rt_cli.cpp -Lraytracertest_amd/lib -lrt_mi355x -o rt_cli
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "Common/Bitmap.h"
#include "RayTracer/RayTracer.h"

namespace {

struct Args {
  uint32_t w = 3840 / 100, h = 2160 / 100;      // App.cpp:13
  uint32_t samples = 1, iterations = 100, update = 10;
  float cx = 0, cy = 0, cz = 0, cxa = 0, cya = 0, fov = 70.0f, focal = 10.0f, aperture = 4.0f;
  uint64_t seed = 0; bool have_seed = false;
  std::string scene = "demo3", scene_file, out = "image0.bmp";
  bool quiet = false, edges = false, smooth = false, nearest = false;
  bool pick = false, focus = false, accel = false, hits = false, closest = false, knn = false, sgn = false, exposure = false, overlap = false, spherecast = false;
  float exposure_p[7] = {0, 0, 0, 0, 0, 1, INFINITY};   // --exposure: x, y, z, normal, far end of the interval
  uint32_t exposure_k = 64;
  float closest_p[4] = {0, 0, 0, INFINITY};        // x, y, z, search distance
  float signed_p[4] = {0, 0, 0, INFINITY};         // --signed: the same
  float knn_p[4] = {0, 0, 0, INFINITY};            // --nearest X,Y,Z[,R[,K]]: x, y, z, search distance
  uint32_t knn_k = 8;
  float overlap_b[6] = {0, 0, 0, 0, 0, 0};         // --overlap X0,Y0,Z0,X1,Y1,Z1[,K]: lo, hi
  uint32_t overlap_k = 8;
  bool overlap_tri = false;
  float overlap_t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // --overlap-tri X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,K]: the three corners
  uint32_t overlap_tri_k = 8;
  bool overlap_hexa = false;
  float overlap_h[24] = {0};                        // --overlap-hexa 24 floats[,K]: the eight corners C0 .. C7
  uint32_t overlap_hexa_k = 8;
  bool section = false;
  float section_p[5] = {0, 0, 0, 0, 0};             // --section NX,NY,NZ,D0[,D1[,K]]: the normal and the slab's ends
  uint32_t section_k = 8;
  bool select = false;
  float select_v[6] = {0, 0, 0, 0, 0, 0};           // --select X0,Y0,X1,Y1,FAR[,NEAR]
  bool tri_distance = false;
  float tri_distance_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, INFINITY};   // --tri-distance X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,R]: the corners, search distance
  float sweep[8] = {0, 0, 0, 0, 0, 0, 0, INFINITY}; // --spherecast X,Y,Z,DX,DY,DZ,R[,TMAX]
  uint32_t pick_xy[2] = {0, 0}, focus_xy[2] = {0, 0}, hits_xy[2] = {0, 0}, hits_k = 8;
};

// "X,Y" -> two pixel coordinates
bool parse_xy(const char* s, uint32_t xy[2]) {
  char* end = nullptr;
  const unsigned long x = std::strtoul(s, &end, 10);
  if (end == s || *end != ',') return false;
  const char* s2 = end + 1;
  const unsigned long y = std::strtoul(s2, &end, 10);
  if (end == s2 || *end != 0) return false;
  xy[0] = static_cast<uint32_t>(x); xy[1] = static_cast<uint32_t>(y);
  return true;
}

// "X,Y" or "X,Y,K"
bool parse_xyk(const char* s, uint32_t xy[2], uint32_t& k) {
  const std::string v = s;
  const size_t c1 = v.find(','), c2 = c1 == std::string::npos ? c1 : v.find(',', c1 + 1);
  if (c2 == std::string::npos) return parse_xy(s, xy);
  char* end = nullptr;
  const unsigned long kk = std::strtoul(v.c_str() + c2 + 1, &end, 10);
  if (end == v.c_str() + c2 + 1 || *end != 0) return false;
  k = static_cast<uint32_t>(kk);
  return parse_xy(v.substr(0, c2).c_str(), xy);
}

// "X,Y,Z" or "X,Y,Z,R": a point and an optional search distance
bool parse_xyzr(const char* s, float out[4]) {
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    const float f = std::strtof(q, &end);
    if (end == q || n == 4) return false;
    out[n] = f;
    if (*end == 0) return n >= 2;
    if (*end != ',') return false;
    q = end + 1;
  }
}

// "X,Y,Z", "X,Y,Z,R" or "X,Y,Z,R,K": a point, an optional search distance and an optional record count
bool parse_xyzrk(const char* s, float out[4], uint32_t& k) {
  const std::string v = s;
  size_t commas = 0, last = std::string::npos;
  for (size_t i = 0; i < v.size(); ++i) if (v[i] == ',') { ++commas; last = i; }
  if (commas < 4) return parse_xyzr(s, out);
  char* end = nullptr;
  const unsigned long kk = std::strtoul(v.c_str() + last + 1, &end, 10);
  if (commas != 4 || end == v.c_str() + last + 1 || *end != 0 || v[last + 1] == '-') return false;
  k = static_cast<uint32_t>(kk);
  return parse_xyzr(v.substr(0, last).c_str(), out);               // (three commas left: four numbers or a failure)
}

// "X,Y,Z,NX,NY,NZ", "...,R" or "...,R,K": a point, its normal, an optional far end of the interval and a direction count
bool parse_exposure(const char* s, float out[7], uint32_t& k) {
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    if (n == 7) {
      if (*q == '-' || *q == '+') return false;
      const unsigned long kk = std::strtoul(q, &end, 10);
      if (end == q || *end != 0 || kk < 1 || kk > RT_MAX_DIRS) return false;
      k = static_cast<uint32_t>(kk);
      return true;
    }
    const float f = std::strtof(q, &end);
    if (end == q) return false;
    out[n] = f;
    if (*end == 0) return n >= 5;
    if (*end != ',') return false;
    q = end + 1;
  }
}

// "X,Y,Z,DX,DY,DZ,R" or "...,TMAX": a sweep as rt_tracer_sphere_cast takes it (out[7] keeps its value when TMAX is absent)
bool parse_spherecast(const char* s, float out[8]) {
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    const float f = std::strtof(q, &end);
    if (end == q || n > 7) return false;
    out[n] = f;
    if (*end == 0) return n >= 6;
    if (*end != ',') return false;
    q = end + 1;
  }
}

// "X0,Y0,Z0,X1,Y1,Z1" or "...,K": the two corners of a box (m = 6), the three of a triangle (m = 9) or the eight of a
// hexahedron (m = 24) and an optional row
// length (0 to RT_MAX_HITS is checked by the query)
bool parse_overlap(const char* s, float* out, uint32_t& k, int m = 6) {
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    if (n == m) {
      if (*q == '-' || *q == '+') return false;
      const unsigned long kk = std::strtoul(q, &end, 10);
      if (end == q || *end != 0) return false;
      k = static_cast<uint32_t>(kk);
      return true;
    }
    const float f = std::strtof(q, &end);
    if (end == q) return false;
    out[n] = f;
    if (*end == 0) return n == m - 1;
    if (*end != ',') return false;
    q = end + 1;
  }
}

// "NX,NY,NZ,D0", "...,D1" or "...,D1,K": a plane (D1 = D0) or slab and an optional row length
bool parse_section(const char* s, float out[5], uint32_t& k) {
  int commas = 0;
  for (const char* q = s; *q; ++q) commas += *q == ',';
  if (commas == 4 || commas == 5) return parse_overlap(s, out, k, 5);    // (without K the fifth float ends the string)
  uint32_t none = 0;
  if (commas != 3 || !parse_overlap(s, out, none, 4)) return false;
  out[4] = out[3];
  return true;
}

// "X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2" or "...,R": the three corners of a triangle and an optional search distance (out[9] keeps its
// value when R is absent)
bool parse_tri_distance(const char* s, float out[10]) {
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    const float f = std::strtof(q, &end);
    if (end == q || n > 9) return false;
    out[n] = f;
    if (*end == 0) return n >= 8;
    if (*end != ',') return false;
    q = end + 1;
  }
}

// what follows --nearest is the point of a k-nearest query (a number), not the next option
bool looks_like_number(const char* s) {
  if (*s == '+' || *s == '-') ++s;
  return (*s >= '0' && *s <= '9') || (*s == '.' && s[1] >= '0' && s[1] <= '9');
}

std::vector<float4> demo3() {                   // MainFrame.cpp:230-232
  return {make_float4(0, 0, 10, 1), make_float4(0, 1, 10, 0), make_float4(1, 0, 10, 0),
          make_float4(1, 0, 10, 0), make_float4(0, 1, 10, 1), make_float4(1, 1, 10, 0),
          make_float4(0, 1, 10, 0), make_float4(0.5f, 1.5f, 10, 0), make_float4(1, 1, 10, 1)};
}

// raw little-endian float32 x,y,z,w records, 3 per triangle (what UploadScene takes)
std::vector<float4> load_f4(const std::string& path) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  std::vector<float4> v;
  if (!in.good()) return v;
  const std::streamsize n = in.tellg();
  in.seekg(0);
  v.resize(static_cast<size_t>(n) / sizeof(float4));
  in.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(float4)));
  return v;
}

// "X0,Y0,X1,Y1,FAR" or "...,NEAR": two corner pixels (non-negative integers), a finite far and an optional finite near (default 0)
bool parse_select(const char* s, float out[6]) {
  out[5] = 0.0f;
  int n = 0;
  for (const char* q = s;; ++n) {
    char* end = nullptr;
    if (n >= 6) return false;
    if (n < 4) {
      if (*q == '-' || *q == '+') return false;
      const unsigned long v = std::strtoul(q, &end, 10);
      if (end == q || v > 0xFFFFFFul) return false;
      out[n] = static_cast<float>(v);
    } else {
      out[n] = std::strtof(q, &end);
      if (end == q || !std::isfinite(out[n])) return false;
    }
    if (*end == 0) return n >= 4;
    if (*end != ',') return false;
    q = end + 1;
  }
}

void usage() {
  std::puts("rt_cli [-w W] [-h H] [-s samples] [-i iterations] [-u updateInterval] [-cx N -cy N -cz N]\n"
            "       [-cxa deg] [-cya deg] [-f fovDeg] [-l focalLength] [-a aperture]      (reference flags, integers)\n"
            "       [--focal F] [--aperture A] [--fov F]                                  (float forms)\n"
            "       [--scene demo3|<file.f4>] [--seed N] [-o out.bmp] [-q]\n"
            "       [--edges] (file holds (v0,e0,e1) rows, packed vertex normals in .w)  [--smooth] [--nearest]\n"
            "       [--nearest X,Y,Z[,R[,K]]] (with a value: prints one line `prim distance u v` per primitive near the point\n"
            "                      X,Y,Z, nearest first, within the distance R when given; at most K, default 8)\n"
            "       [--pick X,Y]  (prints `pick x y prim t u v` for the pixel's pinhole ray)\n"
            "       [--hits X,Y[,K]] (prints one line `prim t u v` per hit of the pixel's pinhole ray, in order, over all t;\n"
            "                      at most K, default 8)\n"
            "       [--closest X,Y,Z[,R]] (prints `closest prim distance x y z`: the nearest surface point to the point X,Y,Z,\n"
            "                      within the distance R when given; `closest -1` when there is none)\n"
            "       [--signed X,Y,Z[,R]] (prints `signed prim distance x y z feature s signed_distance`: --closest's answer, the\n"
            "                      feature of the triangle that holds the nearest point (0 face, 1-3 vertices, 4-6 edges), the side\n"
            "                      s (> 0 in front of the surface, < 0 behind it) and the distance with that sign; `signed -1`)\n"
            "       [--exposure X,Y,Z,NX,NY,NZ[,R[,K]]] (prints `exposure mask open K`: which of K (1 to 64, default 64) cosine-weighted\n"
            "                      hemisphere directions about the normal NX,NY,NZ (used as given) are open from the point X,Y,Z over\n"
            "                      [1e-3, R] -- the mask in hex, bit j = direction j, and their count)\n"
            "       [--overlap X0,Y0,Z0,X1,Y1,Z1[,K]] (prints `overlap count`, the number of primitives that touch the box with the\n"
            "                      corners X0,Y0,Z0 and X1,Y1,Z1, then one line `prim` for each of the K lowest, default 8)\n"
            "       [--overlap-tri X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,K]] (prints `overlap-tri count`, the number of primitives that touch the\n"
            "                      triangle with those three corners, then one line `prim` for each of the K lowest, default 8)\n"
            "       [--tri-distance X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,R]] (prints `tri-distance prim distance where xq yq zq xs ys zs`: the\n"
            "                      nearest primitive to the triangle with those corners within the distance R when given, the candidate\n"
            "                      that found it, the nearest point on the triangle and on the scene; `tri-distance -1` when there is none)\n"
            "       [--overlap-hexa X0,Y0,Z0,...,X7,Y7,Z7[,K]] (prints `overlap-hexa count`, the number of primitives that touch the hexahedron\n"
            "                      with those eight corners in box-like order, then one line `prim` for each of the K lowest, default 8)\n"
            "       [--section NX,NY,NZ,D0[,D1[,K]]] (prints `section count`, the number of primitives the slab D0 <= N.x <= D1 cuts, D1\n"
            "                      defaults to D0: a plane; then for each of the K lowest, default 8, one line\n"
            "                      `prim kind features x0 y0 z0 x1 y1 z1`: its cut at D0)\n"
            "       [--select X0,Y0,X1,Y1,FAR[,NEAR]] (prints `select count`, then one line `prim` for every primitive that touches the frustum\n"
            "                      of the pixel rectangle X0,Y0 .. X1,Y1 between the ray parameters NEAR, default 0, and FAR)\n"
            "       [--focus X,Y] (focal length := distance to what pixel X,Y sees, before the trace; prints it)\n"
            "       [--spherecast X,Y,Z,DX,DY,DZ,R[,TMAX]] (prints `spherecast prim t u v x y z`: the first contact of a sphere of radius\n"
            "                      R whose centre moves from X,Y,Z along DX,DY,DZ for 0 <= t <= TMAX, and the contact point;\n"
            "                      `spherecast -1` when there is none)\n"
            "       [--accel]     (--pick / --hits / --closest / --signed / --exposure / --nearest X,Y,Z / --overlap / --overlap-tri / --section / --tri-distance / --spherecast / --focus through the scene's BVH instead of the scan)");
}

// one region query of the command line: `label count`, then up to k of its prims; false, with the error line, when it fails
using RegionQuery = bool (rt::RayTracer::*)(const std::vector<float>&, uint32_t, std::vector<int32_t>&, std::vector<uint32_t>&,
                                            const std::vector<int32_t>&);
bool print_region(rt::RayTracer& tracer, RegionQuery query, const char* label, const std::vector<float>& queries, uint32_t k) {
  std::vector<int32_t> prims;
  std::vector<uint32_t> counts;
  if (!(tracer.*query)(queries, k, prims, counts, std::vector<int32_t>())) {
    std::fprintf(stderr, "rt_cli: --%s: %s\n", label, k > RT_MAX_HITS ? "K out of range" : tracer.LastError().c_str());
    return false;
  }
  std::printf("%s %u\n", label, counts[0]);
  for (uint32_t j = 0; j < k && j < counts[0]; ++j) std::printf("%d\n", prims[j]);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  for (int i = 1; i < argc; ++i) {
    const std::string k = argv[i];
    auto next = [&](const char* what) -> const char* {
      if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", what); std::exit(2); }
      return argv[++i];
    };
    if (k == "-w") a.w = static_cast<uint32_t>(std::atol(next("-w")));
    else if (k == "-h") a.h = static_cast<uint32_t>(std::atol(next("-h")));
    else if (k == "-s") a.samples = static_cast<uint32_t>(std::atol(next("-s")));
    else if (k == "-i") a.iterations = static_cast<uint32_t>(std::atol(next("-i")));
    else if (k == "-u") a.update = static_cast<uint32_t>(std::atol(next("-u")));
    else if (k == "-cx") a.cx = static_cast<float>(std::atol(next("-cx")));
    else if (k == "-cy") a.cy = static_cast<float>(std::atol(next("-cy")));
    else if (k == "-cz") a.cz = static_cast<float>(std::atol(next("-cz")));
    else if (k == "-cxa") a.cxa = static_cast<float>(std::atol(next("-cxa"))) * 0.01745329251994329576923690768489f;  // glm::radians, App.cpp:148
    else if (k == "-cya") a.cya = static_cast<float>(std::atol(next("-cya"))) * 0.01745329251994329576923690768489f;
    else if (k == "-f") a.fov = static_cast<float>(std::atol(next("-f")));
    else if (k == "-l") a.focal = static_cast<float>(std::atol(next("-l")));
    else if (k == "-a") a.aperture = static_cast<float>(std::atol(next("-a")));
    else if (k == "--fov") a.fov = std::strtof(next("--fov"), nullptr);
    else if (k == "--focal") a.focal = std::strtof(next("--focal"), nullptr);
    else if (k == "--aperture") a.aperture = std::strtof(next("--aperture"), nullptr);
    else if (k == "--cxa-rad") a.cxa = std::strtof(next("--cxa-rad"), nullptr);
    else if (k == "--cya-rad") a.cya = std::strtof(next("--cya-rad"), nullptr);
    else if (k == "--scene") a.scene = next("--scene");
    else if (k == "--seed") { a.seed = std::strtoull(next("--seed"), nullptr, 10); a.have_seed = true; }
    else if (k == "--edges") a.edges = true;
    else if (k == "--smooth") a.smooth = true;
    else if (k == "--nearest" && i + 1 < argc && looks_like_number(argv[i + 1])) {
      if (!parse_xyzrk(next("--nearest"), a.knn_p, a.knn_k)) { std::fprintf(stderr, "--nearest wants X,Y,Z[,R[,K]]\n"); return 2; }
      a.knn = true;
    }
    else if (k == "--nearest") a.nearest = true;
    else if (k == "--overlap") {
      if (!parse_overlap(next("--overlap"), a.overlap_b, a.overlap_k)) { std::fprintf(stderr, "--overlap wants X0,Y0,Z0,X1,Y1,Z1[,K]\n"); return 2; }
      a.overlap = true;
    }
    else if (k == "--accel") a.accel = true;
    else if (k == "--pick" || k == "--focus") {
      const bool pk = k == "--pick";
      if (!parse_xy(next(k.c_str()), pk ? a.pick_xy : a.focus_xy)) { std::fprintf(stderr, "%s wants X,Y\n", k.c_str()); return 2; }
      (pk ? a.pick : a.focus) = true;
    }
    else if (k == "--hits") {
      if (!parse_xyk(next("--hits"), a.hits_xy, a.hits_k)) { std::fprintf(stderr, "--hits wants X,Y[,K]\n"); return 2; }
      a.hits = true;
    }
    else if (k == "--overlap-tri") {
      if (!parse_overlap(next("--overlap-tri"), a.overlap_t, a.overlap_tri_k, 9)) { std::fprintf(stderr, "--overlap-tri wants X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,K]\n"); return 2; }
      a.overlap_tri = true;
    }
    else if (k == "--tri-distance") {
      if (!parse_tri_distance(next("--tri-distance"), a.tri_distance_t)) { std::fprintf(stderr, "--tri-distance wants X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,R]\n"); return 2; }
      a.tri_distance = true;
    }
    else if (k == "--section") {
      if (!parse_section(next("--section"), a.section_p, a.section_k)) { std::fprintf(stderr, "--section wants NX,NY,NZ,D0[,D1[,K]]\n"); return 2; }
      a.section = true;
    }
    else if (k == "--overlap-hexa") {
      if (!parse_overlap(next("--overlap-hexa"), a.overlap_h, a.overlap_hexa_k, 24)) { std::fprintf(stderr, "--overlap-hexa wants X0,Y0,Z0,...,X7,Y7,Z7[,K]\n"); return 2; }
      a.overlap_hexa = true;
    }
    else if (k == "--select") {
      if (!parse_select(next("--select"), a.select_v)) { std::fprintf(stderr, "--select wants X0,Y0,X1,Y1,FAR[,NEAR]\n"); return 2; }
      a.select = true;
    }
    else if (k == "--spherecast") {
      if (!parse_spherecast(next("--spherecast"), a.sweep)) { std::fprintf(stderr, "--spherecast wants X,Y,Z,DX,DY,DZ,R[,TMAX]\n"); return 2; }
      a.spherecast = true;
    }
    else if (k == "--closest") {
      if (!parse_xyzr(next("--closest"), a.closest_p)) { std::fprintf(stderr, "--closest wants X,Y,Z[,R]\n"); return 2; }
      a.closest = true;
    }
    else if (k == "--signed") {
      if (!parse_xyzr(next("--signed"), a.signed_p)) { std::fprintf(stderr, "--signed wants X,Y,Z[,R]\n"); return 2; }
      a.sgn = true;
    }
    else if (k == "--exposure") {
      if (!parse_exposure(next("--exposure"), a.exposure_p, a.exposure_k)) { std::fprintf(stderr, "--exposure wants X,Y,Z,NX,NY,NZ[,R[,K]]\n"); return 2; }
      a.exposure = true;
    }
    else if (k == "-o") a.out = next("-o");
    else if (k == "-q") a.quiet = true;
    else if (k == "-v") a.quiet = false;
    else if (k == "--help") { usage(); return 0; }
    else { std::fprintf(stderr, "unknown option %s\n", k.c_str()); usage(); return 2; }
  }

  rt_options opt;
  std::memset(&opt, 0, sizeof opt);
  opt.struct_size = sizeof opt;
  opt.use_time_seed = 1;                                       // Random.cu:45 unless --seed is given
  opt.flags = (a.smooth ? RT_FLAG_SMOOTH_NORMALS : 0u) | (a.nearest ? RT_FLAG_NEAREST_HIT : 0u);
  rt::RayTracer tracer(math::uvec2(a.w, a.h), math::vec3(a.cx, a.cy, a.cz), math::vec2(a.cxa, a.cya), a.fov, a.focal,
                       a.aperture, &opt);
  if (!tracer.Valid()) { std::fprintf(stderr, "rt_cli: %s\n", tracer.LastError().c_str()); return 1; }
  if (a.have_seed) tracer.SetSeed(a.seed);

  std::vector<float4> scene = (a.scene == "demo3") ? demo3() : load_f4(a.scene);
  if (scene.size() < 3 || scene.size() % 3 != 0) {
    std::fprintf(stderr, "rt_cli: scene '%s' has %zu float4 (need a positive multiple of 3)\n", a.scene.c_str(), scene.size());
    return 1;
  }
  if (a.edges) tracer.UploadSceneEdges(scene);
  else tracer.UploadScene(scene);

  if (a.accel && !tracer.SetQueryAcceleration(true)) {
    std::fprintf(stderr, "rt_cli: --accel: %s\n", tracer.LastError().c_str());
    return 1;
  }
  if (a.pick) {
    rt_hit hit;
    if (!tracer.Pick(math::uvec2(a.pick_xy[0], a.pick_xy[1]), hit)) {
      std::fprintf(stderr, "rt_cli: --pick: %s\n", tracer.LastError().c_str());
      return 1;
    }
    std::printf("pick %u %u %d %.9g %.9g %.9g\n", a.pick_xy[0], a.pick_xy[1], hit.prim, static_cast<double>(hit.t),
                static_cast<double>(hit.u), static_cast<double>(hit.v));
  }
  if (a.hits) {
    rt_hit first;
    math::vec3 ray[2];
    std::vector<rt_hit> hits;
    std::vector<uint32_t> counts;
    if (!tracer.Pick(math::uvec2(a.hits_xy[0], a.hits_xy[1]), first, ray)) {
      std::fprintf(stderr, "rt_cli: --hits: %s\n", tracer.LastError().c_str());
      return 1;
    }
    const std::vector<float> seg = {ray[0].x, ray[0].y, ray[0].z, ray[1].x, ray[1].y, ray[1].z, -INFINITY, INFINITY};
    if (!tracer.IntersectAll(seg, a.hits_k, hits, counts)) {
      std::fprintf(stderr, "rt_cli: --hits: %s\n", a.hits_k == 0 || a.hits_k > RT_MAX_HITS ? "K out of range" : tracer.LastError().c_str());
      return 1;
    }
    for (uint32_t j = 0; j < counts[0]; ++j)
      std::printf("%d %.9g %.9g %.9g\n", hits[j].prim, static_cast<double>(hits[j].t), static_cast<double>(hits[j].u), static_cast<double>(hits[j].v));
  }
  if (a.closest) {
    const float r = a.closest_p[3];
    const std::vector<float> pts = {a.closest_p[0], a.closest_p[1], a.closest_p[2], std::copysign(r * r, r)};
    std::vector<rt_hit> hits;
    if (!tracer.ClosestPoint(pts, hits)) {
      std::fprintf(stderr, "rt_cli: --closest: %s\n", tracer.LastError().c_str());
      return 1;
    }
    const rt_hit& h = hits[0];
    if (h.prim < 0 || static_cast<size_t>(h.prim) >= scene.size() / 3) {
      std::printf("closest -1\n");
    } else {                                                    // v0 + u*e1 + v*e2 of the record the library intersects
      const float4 r0 = scene[3 * h.prim], r1 = scene[3 * h.prim + 1], r2 = scene[3 * h.prim + 2];
      const float v0[3] = {r0.x, r0.y, r0.z}, b[3] = {r1.x, r1.y, r1.z}, c[3] = {r2.x, r2.y, r2.z};
      float q[3];
      for (int i = 0; i < 3; ++i) {
        const float e1 = a.edges ? b[i] : b[i] - v0[i], e2 = a.edges ? c[i] : c[i] - v0[i];
        q[i] = (v0[i] + h.u * e1) + h.v * e2;
      }
      std::printf("closest %d %.9g %.9g %.9g %.9g\n", h.prim, static_cast<double>(std::sqrt(h.t)), static_cast<double>(q[0]),
                  static_cast<double>(q[1]), static_cast<double>(q[2]));
    }
  }
  if (a.sgn) {
    const float r = a.signed_p[3];
    const std::vector<float> pts = {a.signed_p[0], a.signed_p[1], a.signed_p[2], std::copysign(r * r, r)};
    std::vector<rt_hit> hits;
    std::vector<rt_side> sides;
    if (!tracer.SignedDistance(pts, hits, sides)) {
      std::fprintf(stderr, "rt_cli: --signed: %s\n", tracer.LastError().c_str());
      return 1;
    }
    const rt_hit& h = hits[0];
    if (h.prim < 0 || static_cast<size_t>(h.prim) >= scene.size() / 3) {
      std::printf("signed -1\n");
    } else {                                                    // --closest's line, then the side
      const float4 r0 = scene[3 * h.prim], r1 = scene[3 * h.prim + 1], r2 = scene[3 * h.prim + 2];
      const float v0[3] = {r0.x, r0.y, r0.z}, b[3] = {r1.x, r1.y, r1.z}, c[3] = {r2.x, r2.y, r2.z};
      float q[3];
      for (int i = 0; i < 3; ++i) {
        const float e1 = a.edges ? b[i] : b[i] - v0[i], e2 = a.edges ? c[i] : c[i] - v0[i];
        q[i] = (v0[i] + h.u * e1) + h.v * e2;
      }
      const float d = std::sqrt(h.t);
      std::printf("signed %d %.9g %.9g %.9g %.9g %d %.9g %.9g\n", h.prim, static_cast<double>(d), static_cast<double>(q[0]),
                  static_cast<double>(q[1]), static_cast<double>(q[2]), sides[0].feature, static_cast<double>(sides[0].s),
                  static_cast<double>(std::copysign(d, sides[0].s)));
    }
  }
  if (a.exposure) {
    const float* e = a.exposure_p;
    const std::vector<float> pts = {e[0], e[1], e[2], e[3], e[4], e[5], 1e-3f, e[6]};
    std::vector<uint64_t> masks;
    if (!tracer.Exposure(pts, rt::RayTracer::HemisphereDirections(a.exposure_k), masks)) {
      std::fprintf(stderr, "rt_cli: --exposure: %s\n", tracer.LastError().c_str());
      return 1;
    }
    int open = 0;
    for (uint32_t j = 0; j < 64; ++j) open += static_cast<int>((masks[0] >> j) & 1u);
    std::printf("exposure %016llx %d %u\n", static_cast<unsigned long long>(masks[0]), open, a.exposure_k);
  }
  if (a.knn) {
    const float r = a.knn_p[3];
    const std::vector<float> pts = {a.knn_p[0], a.knn_p[1], a.knn_p[2], std::copysign(r * r, r)};
    std::vector<rt_hit> hits;
    std::vector<uint32_t> counts;
    if (!tracer.ClosestAll(pts, a.knn_k, hits, counts)) {
      std::fprintf(stderr, "rt_cli: --nearest: %s\n", a.knn_k == 0 || a.knn_k > RT_MAX_HITS ? "K out of range" : tracer.LastError().c_str());
      return 1;
    }
    for (uint32_t j = 0; j < counts[0]; ++j)
      std::printf("%d %.9g %.9g %.9g\n", hits[j].prim, static_cast<double>(std::sqrt(hits[j].t)), static_cast<double>(hits[j].u),
                  static_cast<double>(hits[j].v));
  }
  if (a.spherecast) {
    const std::vector<float> sweeps(a.sweep, a.sweep + 8);
    std::vector<rt_hit> hits;
    if (!tracer.SphereCast(sweeps, hits)) {
      std::fprintf(stderr, "rt_cli: --spherecast: %s\n", tracer.LastError().c_str());
      return 1;
    }
    const rt_hit& h = hits[0];
    if (h.prim < 0 || static_cast<size_t>(h.prim) >= scene.size() / 3) {
      std::printf("spherecast -1\n");
    } else {                                                    // v0 + u*e1 + v*e2 of the record the library intersects
      const float4 r0 = scene[3 * h.prim], r1 = scene[3 * h.prim + 1], r2 = scene[3 * h.prim + 2];
      const float v0[3] = {r0.x, r0.y, r0.z}, b[3] = {r1.x, r1.y, r1.z}, c[3] = {r2.x, r2.y, r2.z};
      float q[3];
      for (int i = 0; i < 3; ++i) {
        const float e1 = a.edges ? b[i] : b[i] - v0[i], e2 = a.edges ? c[i] : c[i] - v0[i];
        q[i] = (v0[i] + h.u * e1) + h.v * e2;
      }
      std::printf("spherecast %d %.9g %.9g %.9g %.9g %.9g %.9g\n", h.prim, static_cast<double>(h.t), static_cast<double>(h.u),
                  static_cast<double>(h.v), static_cast<double>(q[0]), static_cast<double>(q[1]), static_cast<double>(q[2]));
    }
  }
  if (a.overlap) {
    const float* b = a.overlap_b;
    const std::vector<float> boxes = {b[0], b[1], b[2], 0.0f, b[3], b[4], b[5], 0.0f};
    if (!print_region(tracer, &rt::RayTracer::Overlap, "overlap", boxes, a.overlap_k)) return 1;
  }
  if (a.overlap_tri) {
    const float* c = a.overlap_t;
    const std::vector<float> tris = {c[0], c[1], c[2], 0.0f, c[3], c[4], c[5], 0.0f, c[6], c[7], c[8], 0.0f};
    if (!print_region(tracer, &rt::RayTracer::OverlapTriangles, "overlap-tri", tris, a.overlap_tri_k)) return 1;
  }
  if (a.tri_distance) {
    const float* c = a.tri_distance_t;
    const std::vector<float> tris = {c[0], c[1], c[2], std::copysign(c[9] * c[9], c[9]), c[3], c[4], c[5], 0.0f, c[6], c[7], c[8], 0.0f};
    std::vector<rt_hit> hits;
    std::vector<rt_witness> witness;
    if (!tracer.TriangleDistance(tris, hits, witness)) {
      std::fprintf(stderr, "rt_cli: --tri-distance: %s\n", tracer.LastError().c_str());
      return 1;
    }
    const rt_hit& h = hits[0];
    const rt_witness& w = witness[0];
    if (h.prim < 0 || static_cast<size_t>(h.prim) >= scene.size() / 3) {
      std::printf("tri-distance -1\n");
    } else {                                                    // --closest's position at the witness
      const float4 r0 = scene[3 * h.prim], r1 = scene[3 * h.prim + 1], r2 = scene[3 * h.prim + 2];
      const float v0[3] = {r0.x, r0.y, r0.z}, b[3] = {r1.x, r1.y, r1.z}, cc[3] = {r2.x, r2.y, r2.z};
      float q[3];
      for (int i = 0; i < 3; ++i) {
        const float e1 = a.edges ? b[i] : b[i] - v0[i], e2 = a.edges ? cc[i] : cc[i] - v0[i];
        q[i] = (v0[i] + h.u * e1) + h.v * e2;
      }
      std::printf("tri-distance %d %.9g %d %.9g %.9g %.9g %.9g %.9g %.9g\n", h.prim, static_cast<double>(std::sqrt(h.t)), w.where,
                  static_cast<double>(w.x), static_cast<double>(w.y), static_cast<double>(w.z), static_cast<double>(q[0]),
                  static_cast<double>(q[1]), static_cast<double>(q[2]));
    }
  }
  if (a.overlap_hexa) {
    std::vector<float> hexa(32, 0.0f);
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < 3; ++c) hexa[4 * k + c] = a.overlap_h[3 * k + c];
    if (!print_region(tracer, &rt::RayTracer::OverlapHexahedra, "overlap-hexa", hexa, a.overlap_hexa_k)) return 1;
  }
  if (a.section) {
    const float* c = a.section_p;
    const std::vector<float> planes = {c[0], c[1], c[2], c[3], c[4], 0.0f, 0.0f, 0.0f};
    std::vector<int32_t> prims;
    std::vector<uint32_t> counts;
    std::vector<rt_cut> cuts;
    if (!tracer.Section(planes, a.section_k, prims, counts) || (a.section_k != 0 && !tracer.SectionSegments(planes, prims, a.section_k, 0, cuts))) {
      std::fprintf(stderr, "rt_cli: --section: %s\n", a.section_k > RT_MAX_HITS ? "K out of range" : tracer.LastError().c_str());
      return 1;
    }
    std::printf("section %u\n", counts[0]);
    for (uint32_t j = 0; j < a.section_k && j < counts[0]; ++j) {
      const rt_cut& x = cuts[j];
      std::printf("%d %d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", prims[j], x.kind, x.features, x.p0[0], x.p0[1], x.p0[2], x.p1[0], x.p1[1], x.p1[2]);
    }
  }
  if (a.select) {
    // the frustum between the pinhole rays of the four corner pixels (x0,y0), (x1,y0), (x0,y1), (x1,y1) that holds everything
    // those pixels' rays meet between near and far: flat caps perpendicular to w = ((d0 + d1) + d2) + d3, per ray
    // near_k = (near * min_k c_k) / c_k and far_k = (far * |w|) / c_k with c_k = d_k.w, then C_k = o + near_k*d_k,
    // C_{k+4} = o + far_k*d_k; every operation rounded to float (RayTracer.cap_parameters of the Python class).  Then the
    // cursor until the count is within the row.
    const uint32_t x0 = static_cast<uint32_t>(std::min(a.select_v[0], a.select_v[2])), x1 = static_cast<uint32_t>(std::max(a.select_v[0], a.select_v[2]));
    const uint32_t y0 = static_cast<uint32_t>(std::min(a.select_v[1], a.select_v[3])), y1 = static_cast<uint32_t>(std::max(a.select_v[1], a.select_v[3]));
    const uint32_t px[4][2] = {{x0, y0}, {x1, y0}, {x0, y1}, {x1, y1}};
    float o[4][3], d[4][3];
    for (int k = 0; k < 4; ++k) {
      rt_hit hit;
      math::vec3 ray[2];
      if (!tracer.Pick(math::uvec2(px[k][0], px[k][1]), hit, ray)) {
        std::fprintf(stderr, "rt_cli: --select: %s\n", tracer.LastError().c_str());
        return 1;
      }
      o[k][0] = ray[0].x; o[k][1] = ray[0].y; o[k][2] = ray[0].z;
      d[k][0] = ray[1].x; d[k][1] = ray[1].y; d[k][2] = ray[1].z;
    }
    volatile float t;                                                     // (every operation rounded to float before the next)
    const auto dot = [&t](const float* u, const float* v) { t = u[0] * v[0]; volatile float s = u[1] * v[1]; t = t + s; s = u[2] * v[2]; t = t + s; return static_cast<float>(t); };
    float w[3], c[4];
    for (int i = 0; i < 3; ++i) { t = d[0][i] + d[1][i]; t = t + d[2][i]; t = t + d[3][i]; w[i] = t; }
    for (int k = 0; k < 4; ++k) c[k] = dot(d[k], w);
    const float cmin = std::min(std::min(std::min(c[0], c[1]), c[2]), c[3]);
    t = std::sqrt(dot(w, w));
    const float wl = t;
    t = a.select_v[5] * cmin;
    const float near_c = t;
    t = a.select_v[4] * wl;
    const float far_c = t;
    std::vector<float> hexa(32, 0.0f);
    for (int k = 0; k < 4; ++k) {
      t = near_c / c[k];
      const float nk = t;
      t = far_c / c[k];
      const float fk = t;
      for (int i = 0; i < 3; ++i) {
        t = nk * d[k][i];
        hexa[4 * k + i] = o[k][i] + t;
        t = fk * d[k][i];
        hexa[4 * (k + 4) + i] = o[k][i] + t;
      }
    }
    std::vector<int32_t> all, prims, after;
    std::vector<uint32_t> counts;
    for (;;) {
      if (!tracer.OverlapHexahedra(hexa, RT_MAX_HITS, prims, counts, after)) {
        std::fprintf(stderr, "rt_cli: --select: %s\n", tracer.LastError().c_str());
        return 1;
      }
      for (uint32_t j = 0; j < RT_MAX_HITS && j < counts[0]; ++j) all.push_back(prims[j]);
      if (counts[0] <= RT_MAX_HITS) break;
      after.assign(1, prims[RT_MAX_HITS - 1]);
    }
    std::printf("select %zu\n", all.size());
    for (const int32_t prim : all) std::printf("%d\n", prim);
  }
  if (a.focus) {
    float focal = 0.0f;
    if (!tracer.FocusAt(math::uvec2(a.focus_xy[0], a.focus_xy[1]), &focal)) {
      std::fprintf(stderr, "rt_cli: --focus: %s\n", tracer.LastError().c_str());
      return 1;
    }
    std::printf("focus %u %u focal %.9g\n", a.focus_xy[0], a.focus_xy[1], static_cast<double>(focal));
  }

  uint32_t updates = 0;
  std::vector<rt::Color> finalImage;
  tracer.SetUpdateCallback([&](rt::ColorPtr, const std::size_t) { ++updates; });
  tracer.SetFinishedCallback([&](rt::ColorPtr image, const std::size_t size) {
    finalImage.assign(image, image + size / sizeof(rt::Color));
  });
  const auto t0 = std::chrono::steady_clock::now();
  tracer.Trace(a.iterations, a.samples, a.update);          // MainFrame.cpp:254-256
  const bool done = tracer.Wait();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!done || finalImage.size() != static_cast<size_t>(a.w) * a.h) {
    std::fprintf(stderr, "rt_cli: trace did not finish: %s\n", tracer.LastError().c_str());
    return 1;
  }
  try {
    rt::Bitmap bmp(math::uvec2(a.w, a.h), finalImage);      // MainFrame.cpp:358-359
    bmp.Write(a.out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "rt_cli: %s\n", e.what());
    return 1;
  }
  if (!a.quiet) {
    const double rays = double(a.w) * a.h * a.iterations * a.samples;
    std::printf("%ux%u, %u x %u spp, %zu triangles, %u updates: %.2f ms end to end (%.1f Mray/s incl. host hand-off) -> %s\n",
                a.w, a.h, a.iterations, a.samples, scene.size() / 3, updates, ms, rays / ms / 1e3, a.out.c_str());
  }
  return 0;
}
