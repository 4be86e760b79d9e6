// rt_bvh_host.hpp -- host build of the ray queries' bounding volume hierarchy (RT_QUERY_BVH).  Plain C++, no
// HIP: the tracer builds with it (rt_query_api.hpp) and so does rt_dbg_bvh_build on a machine without a GPU.
//
// Input: the records the kernel intersects -- per triangle v0, e1, e2 as prep_triangles_kernel stores them.  A triangle's box
// is the box of v0, v0 + e1, v0 + e2 evaluated in double and rounded outward to fp32.  Triangles with a non-finite record (or
// a box that leaves fp32) are in no box: they form the always-tested list behind the leaves' records.
//
// Build: top-down over the boxes' centres, binned SAH (16 bins on the axis of the largest centre extent), object-median
// splits where the SAH has nothing to say (coincident centres, an empty side) and wherever a SAH child could no longer be
// finished by median splits inside the depth bound; leaves of at most 4 triangles, records in a leaf ascending by upload
// index.  The binary tree is then collapsed to 4-wide nodes (a node's children are its binary grandchildren where the
// binary children are inner nodes), written in depth-first order.
//
// Layouts (include/rt_mi355x.h documents them for rt_dbg_bvh_build):
//   node, 128 bytes: float lo_x[4], lo_y[4], lo_z[4], hi_x[4], hi_y[4], hi_z[4]; uint32 child[4]; float cmax[4]
//     child: kBvhEmpty, or an inner node's index (< 2^31), or kBvhLeaf | (count - 1) << 28 | first record (count 1..4);
//     cmax: the largest |coordinate| of the child's box (the box test's scale); an empty child has lo = +inf, hi = -inf.
//   record, 48 bytes: float e2[3], e1[3], v0[3]; uint32 upload index; 2 x uint32 zero
//
// Refit: a re-uploaded scene of the same size keeps the tree's topology; refit() copies the new records
// into their slots and recomputes every box bottom-up.  It is the reference of the kernels of rt_refit.hpp.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace rtb {

constexpr uint32_t kBvhEmpty = 0xFFFFFFFFu;
constexpr uint32_t kBvhLeaf = 0x80000000u;
constexpr uint32_t kBvhLeafMax = 4u;                  // triangles per leaf
constexpr uint32_t kBvhMaxBinaryDepth = 32u;          // edges from the binary root to a leaf: 2^28 triangles need 26 by medians
constexpr uint32_t kBvhMaxDepth = kBvhMaxBinaryDepth / 2u;   // levels of 4-wide nodes: what the traversal stack is sized from
constexpr size_t kBvhMaxTris = size_t(1) << 28;

struct Node {
  float lo[3][4], hi[3][4];
  uint32_t child[4];
  float cmax[4];
};
struct Record {
  float e2[3], e1[3], v0[3];
  uint32_t index, pad[2];
};
static_assert(sizeof(Node) == 128 && sizeof(Record) == 48, "layouts of include/rt_mi355x.h");

struct Tree {
  std::vector<Node> nodes;
  std::vector<Record> records;      // the leaves' records, then the always-tested list (ascending upload index)
  uint32_t leaves = 0, depth = 0, always = 0;
  uint64_t build_us = 0;
  // the node indices grouped by level (root first): level l (0-based) is level_nodes[level_begin[l] .. level_begin[l + 1]),
  // depth levels in all (at most kBvhMaxDepth) -- a refit walks them deepest first
  std::vector<uint32_t> level_nodes, level_begin;
  size_t bytes() const { return nodes.size() * sizeof(Node) + records.size() * sizeof(Record); }
};

// stack entries a traversal of a tree of `depth` node levels can hold: three waiting siblings per level
inline uint32_t stack_capacity(uint32_t depth) { return 3u * (depth ? depth : 1u); }

namespace detail {

struct Box {
  float lo[3], hi[3];
  void clear() { for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; } }
  void grow(const Box& b) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
  double half_area() const {
    const double x = double(hi[0]) - lo[0], y = double(hi[1]) - lo[1], z = double(hi[2]) - lo[2];
    return x * y + y * z + z * x;
  }
};
inline float round_down(double x) { float f = static_cast<float>(x); if (double(f) > x) f = std::nextafter(f, -INFINITY); return f; }
inline float round_up(double x) { float f = static_cast<float>(x); if (double(f) < x) f = std::nextafter(f, INFINITY); return f; }

// A triangle's box from its record r (e2 xyz, e1 xyz, v0 xyz): the corners v0, v0 + e1, v0 + e2 in double, rounded outward;
// centre[a] = the box's middle before rounding.  False -- the triangle belongs to the always-tested list -- when a float of
// the record or of the rounded box is not finite (box and centre are then incomplete).
inline bool tri_box(const float* r, Box& box, double* centre) {
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(r[k]);
  for (int a = 0; a < 3 && finite; ++a) {
    const double v0 = r[6 + a], c1 = v0 + double(r[3 + a]), c2 = v0 + double(r[a]);
    const double lo = std::min(v0, std::min(c1, c2)), hi = std::max(v0, std::max(c1, c2));
    box.lo[a] = round_down(lo); box.hi[a] = round_up(hi);
    if (centre) centre[a] = 0.5 * (lo + hi);
    finite = std::isfinite(box.lo[a]) && std::isfinite(box.hi[a]);
  }
  return finite;
}

struct Prim { Box box; double c[3]; uint32_t index; };
struct BinNode { Box box; uint32_t left, right, first, count; };   // leaf: left == kBvhEmpty

// blog2(ceil(count / 4)) rounded up: binary levels a median build of `count` triangles needs below its root
inline uint32_t median_levels(size_t count) {
  size_t leaves = (count + kBvhLeafMax - 1u) / kBvhLeafMax;
  uint32_t l = 0;
  while ((size_t(1) << l) < leaves) ++l;
  return l;
}

struct Builder {
  std::vector<Prim>& prims;
  std::vector<BinNode> bin;
  uint32_t max_binary_depth = kBvhMaxBinaryDepth;                // (a test's probe build raises it to see the SAH's own depth)

  uint32_t build(size_t first, size_t count, uint32_t level) {
    const uint32_t me = static_cast<uint32_t>(bin.size());
    bin.push_back({});
    Box box; box.clear();
    double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = first; i < first + count; ++i) {
      box.grow(prims[i].box);
      for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], prims[i].c[a]); chi[a] = std::max(chi[a], prims[i].c[a]); }
    }
    bin[me].box = box;
    if (count <= kBvhLeafMax) {
      std::sort(prims.begin() + first, prims.begin() + first + count, [](const Prim& x, const Prim& y) { return x.index < y.index; });
      bin[me].left = bin[me].right = kBvhEmpty;
      bin[me].first = static_cast<uint32_t>(first); bin[me].count = static_cast<uint32_t>(count);
      return me;
    }
    int axis = 0;
    for (int a = 1; a < 3; ++a) if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
    const uint32_t room = max_binary_depth - level - 1u;         // binary levels left below a child of this node
    size_t mid = 0;
    const double ext = chi[axis] - clo[axis];
    if (ext > 0.0 && std::isfinite(ext)) {                       // binned SAH
      constexpr int kBins = 16;
      Box bb[kBins]; size_t bn[kBins] = {};
      for (Box& b : bb) b.clear();
      const double scale = kBins / ext;
      auto bin_of = [&](const Prim& p) { const int b = static_cast<int>((p.c[axis] - clo[axis]) * scale); return b < 0 ? 0 : b >= kBins ? kBins - 1 : b; };
      for (size_t i = first; i < first + count; ++i) { const int b = bin_of(prims[i]); bb[b].grow(prims[i].box); ++bn[b]; }
      double right_area[kBins]; size_t right_n[kBins];
      Box acc; acc.clear(); size_t n = 0;
      for (int b = kBins - 1; b > 0; --b) { acc.grow(bb[b]); n += bn[b]; right_area[b] = n ? acc.half_area() : 0.0; right_n[b] = n; }
      acc.clear(); n = 0;
      double best = INFINITY; int cut = -1;
      for (int b = 0; b + 1 < kBins; ++b) {
        acc.grow(bb[b]); n += bn[b];
        if (n == 0 || right_n[b + 1] == 0) continue;
        const double cost = acc.half_area() * double(n) + right_area[b + 1] * double(right_n[b + 1]);
        if (cost < best) { best = cost; cut = b; }
      }
      if (cut >= 0) {
        const auto it = std::stable_partition(prims.begin() + first, prims.begin() + first + count, [&](const Prim& p) { return bin_of(p) <= cut; });
        mid = static_cast<size_t>(it - (prims.begin() + first));
        if (mid == 0 || mid == count || median_levels(mid) > room || median_levels(count - mid) > room) mid = 0;
      }
    }
    if (mid == 0) {                                              // object median (ties by upload index: deterministic)
      // the left half takes whole leaves, so that both halves stay within median_levels(count) - 1
      const size_t leaves = (count + kBvhLeafMax - 1u) / kBvhLeafMax;
      mid = ((leaves + 1u) / 2u) * kBvhLeafMax;
      if (mid >= count) mid = count / 2u;
      std::nth_element(prims.begin() + first, prims.begin() + first + mid, prims.begin() + first + count, [axis](const Prim& x, const Prim& y) {
        return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.index < y.index);
      });
    }
    const uint32_t l = build(first, mid, level + 1u);
    const uint32_t r = build(first + mid, count - mid, level + 1u);
    bin[me].left = l; bin[me].right = r; bin[me].first = 0; bin[me].count = 0;
    return me;
  }
};

}  // namespace detail

// rec: 9 floats per triangle, e2 xyz, e1 xyz, v0 xyz (the order of the 36-byte device record)
inline Tree build(const float* rec, size_t n_tris) {
  using namespace detail;
  const auto t0 = std::chrono::steady_clock::now();
  Tree tree;
  std::vector<Prim> prims;
  std::vector<uint32_t> always;
  prims.reserve(n_tris);
  for (size_t i = 0; i < n_tris; ++i) {
    Prim p;
    p.index = static_cast<uint32_t>(i);
    if (tri_box(rec + 9u * i, p.box, p.c)) prims.push_back(p); else always.push_back(p.index);
  }
  Builder b{prims, {}};
  if (!prims.empty()) (void)b.build(0, prims.size(), 0u);

  auto record_of = [&](uint32_t index) {
    Record q;
    memcpy(q.e2, rec + 9u * size_t(index), 9u * sizeof(float));
    q.index = index; q.pad[0] = q.pad[1] = 0u;
    return q;
  };
  tree.records.reserve(n_tris);
  for (const Prim& p : prims) tree.records.push_back(record_of(p.index));
  for (uint32_t i : always) tree.records.push_back(record_of(i));
  tree.always = static_cast<uint32_t>(always.size());

  // collapse to 4-wide nodes, depth first: (binary node that becomes a 4-wide node, its level)
  if (!b.bin.empty()) {
    auto ref_of_leaf = [&](const BinNode& n) { tree.leaves++; return kBvhLeaf | (n.count - 1u) << 28 | n.first; };
    struct Todo { uint32_t bin, node, level; };
    std::vector<Todo> todo;
    std::vector<uint32_t> level_of;                                  // per node, 0-based
    tree.nodes.push_back({});
    todo.push_back({0u, 0u, 1u});
    while (!todo.empty()) {
      const Todo t = todo.back(); todo.pop_back();
      tree.depth = std::max(tree.depth, t.level);
      if (level_of.size() < tree.nodes.size()) level_of.resize(tree.nodes.size());
      level_of[t.node] = t.level - 1u;
      uint32_t kids[4]; int nk = 0;
      const BinNode& root = b.bin[t.bin];
      if (root.left == kBvhEmpty) kids[nk++] = t.bin;              // a scene of at most 4 triangles: one leaf under the root
      else
        for (uint32_t c : {root.left, root.right}) {
          const BinNode& cn = b.bin[c];
          if (cn.left == kBvhEmpty) kids[nk++] = c; else { kids[nk++] = cn.left; kids[nk++] = cn.right; }
        }
      Node nd;
      uint32_t inner[4]; int ni = 0;
      for (int k = 0; k < 4; ++k) {
        if (k >= nk) {
          for (int a = 0; a < 3; ++a) { nd.lo[a][k] = INFINITY; nd.hi[a][k] = -INFINITY; }
          nd.child[k] = kBvhEmpty; nd.cmax[k] = 0.0f;
          continue;
        }
        const BinNode& cn = b.bin[kids[k]];
        float m = 0.0f;
        for (int a = 0; a < 3; ++a) {
          nd.lo[a][k] = cn.box.lo[a]; nd.hi[a][k] = cn.box.hi[a];
          m = std::max(m, std::max(std::fabs(cn.box.lo[a]), std::fabs(cn.box.hi[a])));
        }
        nd.cmax[k] = m;
        if (cn.left == kBvhEmpty) nd.child[k] = ref_of_leaf(cn);
        else { nd.child[k] = static_cast<uint32_t>(tree.nodes.size()); tree.nodes.push_back({}); inner[ni++] = static_cast<uint32_t>(k); }
      }
      for (int i = ni - 1; i >= 0; --i) todo.push_back({kids[inner[i]], nd.child[inner[i]], t.level + 1u});
      tree.nodes[t.node] = nd;
    }
    tree.level_begin.assign(tree.depth + 1u, 0u);                    // a counting sort of the nodes by level
    for (uint32_t l : level_of) tree.level_begin[l + 1u]++;
    for (uint32_t l = 0; l < tree.depth; ++l) tree.level_begin[l + 1u] += tree.level_begin[l];
    tree.level_nodes.resize(tree.nodes.size());
    std::vector<uint32_t> at(tree.level_begin.begin(), tree.level_begin.end() - 1);
    for (uint32_t i = 0; i < level_of.size(); ++i) tree.level_nodes[at[level_of[i]]++] = i;
  }
  tree.build_us = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return tree;
}

// the records of upload rows: absolute vertices (e = v - v0 in fp32, prep_triangles_kernel's subtraction) or v0, e1, e2 rows
inline std::vector<float> records_of_rows(const float* rows4, size_t n_tris, bool edges) {
  std::vector<float> rec(n_tris * 9u);
  for (size_t i = 0; i < n_tris; ++i) {
    const float* a = rows4 + 12u * i; const float* b = a + 4; const float* c = a + 8;
    float* r = rec.data() + 9u * i;
    for (int k = 0; k < 3; ++k) {
      volatile float e1 = edges ? b[k] : b[k] - a[k], e2 = edges ? c[k] : c[k] - a[k];   // (rounded to fp32 each, whatever the host's evaluation method)
      r[k] = e2; r[3 + k] = e1; r[6 + k] = a[k];
    }
  }
  return rec;
}

// the same from the device's arrays read back: tri_a (e2.xyz, e1.x), (e1.yz, v0.xy) and tri_b v0.z
inline std::vector<float> records_of_device(const float* tri_a, const float* tri_b, size_t n_tris) {
  std::vector<float> rec(n_tris * 9u);
  for (size_t i = 0; i < n_tris; ++i) {
    memcpy(rec.data() + 9u * i, tri_a + 8u * i, 8u * sizeof(float));
    rec[9u * i + 8u] = tri_b[i];
  }
  return rec;
}

// A child's box as a node holds it
inline detail::Box child_box(const Node& nd, int k) {
  detail::Box b;
  for (int a = 0; a < 3; ++a) { b.lo[a] = nd.lo[a][k]; b.hi[a] = nd.hi[a][k]; }
  return b;
}

// The tree's cost: the half areas of all present children's boxes, summed in double, over the half area of
// the union of the root's child boxes.  0 without nodes, and 0 when that union has no area (a scene on one line).
inline double tree_cost(const Node* nodes, size_t n_nodes) {
  if (n_nodes == 0u) return 0.0;
  double sum = 0.0;
  for (size_t i = 0; i < n_nodes; ++i)
    for (int k = 0; k < 4; ++k)
      if (nodes[i].child[k] != kBvhEmpty) sum += child_box(nodes[i], k).half_area();
  detail::Box root; root.clear();
  for (int k = 0; k < 4; ++k) root.grow(child_box(nodes[0], k));
  const double area = root.half_area();
  return area > 0.0 ? sum / area : 0.0;
}
inline double tree_cost(const std::vector<Node>& nodes) { return tree_cost(nodes.data(), nodes.size()); }

// Refit: the tree keeps its topology and takes the records of `rec` (9 floats per triangle, by upload index; as many
// triangles as the tree has records).  Every slot's 36 bytes are rewritten; a leaf child's box becomes the union of its
// triangles' boxes, each computed as build() computes it; an inner child's box the union of the referenced node's four child
// boxes; cmax follows.  Children come behind their parents in the node array, so one pass from the back sees every node after
// its children.  Partition rule: a slot of the leaves must hold a finite triangle (detail::tri_box) and a slot of the
// always-tested list a non-finite one; otherwise nothing is written and the result is false -- the tree has to be built.
// The arrays must be a tree of build(): every reference in range (rt_dbg_bvh_refit checks that for its caller's arrays).
inline bool refit(Node* nodes, size_t n_nodes, Record* records, size_t n_leaf_records, size_t n_always, const float* rec) {
  using namespace detail;
  Box box;
  for (size_t s = 0; s < n_leaf_records + n_always; ++s)
    if (tri_box(rec + 9u * size_t(records[s].index), box, nullptr) != (s < n_leaf_records)) return false;
  for (size_t s = 0; s < n_leaf_records + n_always; ++s) memcpy(records[s].e2, rec + 9u * size_t(records[s].index), 9u * sizeof(float));
  for (size_t i = n_nodes; i-- > 0u;) {
    Node& nd = nodes[i];
    for (int k = 0; k < 4; ++k) {
      const uint32_t ref = nd.child[k];
      if (ref == kBvhEmpty) continue;
      Box b; b.clear();
      if (ref & kBvhLeaf) {
        const uint32_t first = ref & 0x0FFFFFFFu, count = ((ref >> 28) & 3u) + 1u;
        for (uint32_t j = first; j < first + count; ++j) { (void)tri_box(records[j].e2, box, nullptr); b.grow(box); }
      } else {
        for (int c = 0; c < 4; ++c) b.grow(child_box(nodes[ref], c));
      }
      float m = 0.0f;
      for (int a = 0; a < 3; ++a) {
        nd.lo[a][k] = b.lo[a]; nd.hi[a][k] = b.hi[a];
        m = std::max(m, std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
      }
      nd.cmax[k] = m;
    }
  }
  return true;
}
inline bool refit(std::vector<Node>& nodes, std::vector<Record>& records, size_t n_leaf_records, size_t n_always, const float* rec) {
  return refit(nodes.data(), nodes.size(), records.data(), n_leaf_records, n_always, rec);
}

}  // namespace rtb
