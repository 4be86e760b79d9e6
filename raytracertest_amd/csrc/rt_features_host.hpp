// rt_features_host.hpp -- host build of the signed queries' feature table (rt_tracer_signed_distance*, rt_tracer_closest_sides*;
// DESIGN.md 4.3h).  Plain C++, no HIP: the tracer builds with it (rt_query_api.hpp) and so does rt_dbg_feature_normals on a
// machine without a GPU.
//
// Input: the upload rows (3 per triangle: absolute vertices, or v0, e1, e2 of the edges layout).  Output: seven unit normals per
// triangle, 7 x float4 = 112 bytes, .w = 0 -- the angle-weighted pseudonormals of Baerentzen & Aanaes, whose dot product with
// p - c has the sign of the side p lies on whichever feature of the triangle the nearest point c falls on:
//   0        the face                 (region 7 of closest_triangle)
//   1, 2, 3  the vertices A = v0, B, C (regions 1, 2, 4)
//   4, 5, 6  the edges AB, AC, BC      (regions 3, 5, 6)
//
// Everything is float64 from the fp32 positions, rounded to fp32 once at the end:
//   face     (B - A) x (C - A), normalised.  A triangle whose cross product is zero or not finite CONTRIBUTES nothing anywhere
//            and its own face entry is the zero vector.
//   vertex   the sum over the incident contributing triangles, in ascending triangle index, of (the interior angle at the
//            vertex, atan2(|a x b|, a . b)) x (the unit face normal), normalised.
//   edge     the sum of the unit face normals of all contributing triangles that share the undirected edge, in ascending index,
//            normalised: one triangle at a boundary edge, three or more at a non-manifold one.
//   a zero (or non-finite) sum gives the zero vector.
// Vertices are welded by their exact fp32 bits, -0 taken as +0; for the edges layout the key is fp32 v0, v0 + e1, v0 + e2.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rtf {

constexpr size_t kFeaturesPerTri = 7u;

struct Table {
  std::vector<float> normals;       // n_tris x 7 x 4 floats
  uint64_t vertices = 0, edges = 0, contributing = 0, build_us = 0;
  size_t bytes() const { return normals.size() * sizeof(float); }
};

namespace detail {

struct Key {
  uint32_t b[3];
  bool operator<(const Key& o) const { return b[0] != o.b[0] ? b[0] < o.b[0] : b[1] != o.b[1] ? b[1] < o.b[1] : b[2] < o.b[2]; }
  bool operator==(const Key& o) const { return b[0] == o.b[0] && b[1] == o.b[1] && b[2] == o.b[2]; }
};

inline Key key_of(const float* v) {
  Key k;
  for (int a = 0; a < 3; ++a) {
    memcpy(&k.b[a], v + a, 4u);
    if (k.b[a] == 0x80000000u) k.b[a] = 0u;                              // -0 welds with +0
  }
  return k;
}

struct D3 { double x, y, z; };
inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double norm(D3 a) { return std::sqrt(dot(a, a)); }

// unit vector, or zero where the length is zero or not finite
inline D3 unit(D3 a) {
  const double l = norm(a);
  if (!(l > 0.0) || !std::isfinite(l)) return {0.0, 0.0, 0.0};
  return {a.x / l, a.y / l, a.z / l};
}

struct Ref { uint64_t id; uint32_t tri, slot; };                         // a vertex or edge id, the triangle, the feature 1..6

}  // namespace detail

// rows4: 3 x n_tris rows of 4 floats (.w is not read)
inline Table build(const float* rows4, size_t n_tris, bool edges) {
  using namespace detail;
  const auto t0 = std::chrono::steady_clock::now();
  Table tab;
  tab.normals.assign(n_tris * kFeaturesPerTri * 4u, 0.0f);

  // the fp32 corners of every triangle
  std::vector<float> pos(n_tris * 9u);
  for (size_t i = 0; i < n_tris; ++i) {
    const float* a = rows4 + 12u * i; const float* b = a + 4; const float* c = a + 8;
    float* q = pos.data() + 9u * i;
    for (int k = 0; k < 3; ++k) {
      volatile float vb = edges ? a[k] + b[k] : b[k], vc = edges ? a[k] + c[k] : c[k];   // (rounded to fp32 each)
      q[k] = a[k]; q[3 + k] = vb; q[6 + k] = vc;
    }
  }

  // weld: a vertex id per corner
  std::vector<std::pair<Key, uint32_t>> keys(n_tris * 3u);
  for (size_t c = 0; c < n_tris * 3u; ++c) keys[c] = {key_of(pos.data() + 3u * c), static_cast<uint32_t>(c)};
  std::sort(keys.begin(), keys.end(), [](const auto& x, const auto& y) { return x.first < y.first || (x.first == y.first && x.second < y.second); });
  std::vector<uint32_t> vid(n_tris * 3u);
  uint32_t n_vert = 0;
  for (size_t k = 0; k < keys.size(); ++k) {
    if (k != 0u && !(keys[k].first == keys[k - 1u].first)) ++n_vert;
    vid[keys[k].second] = n_vert;
  }

  // unit face normals and corner angles of the contributing triangles; the references of vertices and edges
  std::vector<D3> fn(n_tris);
  std::vector<double> ang(n_tris * 3u, 0.0);
  std::vector<uint8_t> contributes(n_tris, 0);
  std::vector<Ref> vrefs, erefs;
  vrefs.reserve(n_tris * 3u); erefs.reserve(n_tris * 3u);
  static const int kEdgeEnds[3][2] = {{0, 1}, {0, 2}, {1, 2}};           // AB, AC, BC
  for (size_t i = 0; i < n_tris; ++i) {
    const float* q = pos.data() + 9u * i;
    const D3 P[3] = {{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}};
    const D3 n = cross(sub(P[1], P[0]), sub(P[2], P[0]));
    fn[i] = unit(n);
    contributes[i] = (fn[i].x != 0.0 || fn[i].y != 0.0 || fn[i].z != 0.0) && std::isfinite(fn[i].x) && std::isfinite(fn[i].y) && std::isfinite(fn[i].z);
    if (!contributes[i]) { fn[i] = {0.0, 0.0, 0.0}; continue; }
    ++tab.contributing;
    for (int c = 0; c < 3; ++c) {
      const D3 a = sub(P[(c + 1) % 3], P[c]), b = sub(P[(c + 2) % 3], P[c]);
      ang[3u * i + c] = std::atan2(norm(cross(a, b)), dot(a, b));
    }
  }
  for (size_t i = 0; i < n_tris; ++i) {                                  // (every triangle looks its features up, contributing or not)
    for (int c = 0; c < 3; ++c) vrefs.push_back({vid[3u * i + c], static_cast<uint32_t>(i), static_cast<uint32_t>(1 + c)});
    for (int e = 0; e < 3; ++e) {
      const uint64_t u = vid[3u * i + kEdgeEnds[e][0]], v = vid[3u * i + kEdgeEnds[e][1]];
      erefs.push_back({std::min(u, v) << 32 | std::max(u, v), static_cast<uint32_t>(i), static_cast<uint32_t>(4 + e)});
    }
  }
  auto by_id_then_tri = [](const Ref& x, const Ref& y) { return x.id != y.id ? x.id < y.id : x.tri != y.tri ? x.tri < y.tri : x.slot < y.slot; };
  std::sort(vrefs.begin(), vrefs.end(), by_id_then_tri);
  std::sort(erefs.begin(), erefs.end(), by_id_then_tri);

  auto store = [&](uint32_t tri, uint32_t slot, D3 n) {
    float* o = tab.normals.data() + (kFeaturesPerTri * tri + slot) * 4u;
    o[0] = static_cast<float>(n.x); o[1] = static_cast<float>(n.y); o[2] = static_cast<float>(n.z); o[3] = 0.0f;
  };
  for (size_t i = 0; i < n_tris; ++i) store(static_cast<uint32_t>(i), 0u, fn[i]);

  // one group of references per vertex (per edge): sum in ascending triangle index, normalise, hand to every member
  auto groups = [&](const std::vector<Ref>& refs, bool weighted, uint64_t& count) {
    for (size_t g0 = 0; g0 < refs.size();) {
      size_t g1 = g0;
      D3 s = {0.0, 0.0, 0.0};
      for (; g1 < refs.size() && refs[g1].id == refs[g0].id; ++g1) {
        const Ref& r = refs[g1];
        if (!contributes[r.tri]) continue;
        // a triangle with two corners welded is degenerate and contributes nothing, so a contributing one appears once
        const double w = weighted ? ang[3u * r.tri + (r.slot - 1u)] : 1.0;
        s.x += w * fn[r.tri].x; s.y += w * fn[r.tri].y; s.z += w * fn[r.tri].z;
      }
      const D3 n = unit(s);
      for (size_t k = g0; k < g1; ++k) store(refs[k].tri, refs[k].slot, n);
      ++count;
      g0 = g1;
    }
  };
  groups(vrefs, true, tab.vertices);
  groups(erefs, false, tab.edges);
  tab.build_us = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return tab;
}

}  // namespace rtf
