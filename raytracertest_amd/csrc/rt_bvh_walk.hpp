// rt_bvh_walk.hpp -- the traversal of the scene's bounding volume hierarchy (RT_QUERY_BVH) as one function
// for the walkers whose time it leaves alone: occluded_bvh_kernel, exposure_bvh_kernel and allhits_bvh_kernel call bvh_walk.
// query_bvh_kernel, closest_bvh_kernel and nearest_bvh_kernel state the same loop in their own text (rt_bvh.hpp, rt_closest.hpp,
// rt_nearest.hpp: on bvh_walk they measured slower than their parent): a change of the walk is made here and in those three.
// Included by rt_kernels.hip only, behind rt_bvh.hpp.  A query brings its own skip rule, ordering key and record test as
// callables; the loop, the node, the ray's box test and the stack are stated here.
//
// Shape: lane = query.  Each lane walks the 4-wide tree of rt_bvh_host.hpp on its own: a node is eight 16-byte loads (128
// bytes, one line), the query's child() judges the four child boxes, the children worth a visit are ordered best first, the
// best is entered and the others wait on the lane's stack, the better of them on top.  The stack lives in LDS at
// entry * STRIDE + slot (STRIDE = the block's threads): a wave's pushes and pops touch 64 consecutive entries, free of bank
// conflicts (a runtime-indexed private array would live in scratch).  An entry is the child's reference alone (4 bytes), or
// KEYED {goodness, reference} (8 bytes) where a waiting child is judged again at its pop.  The capacity is b.stack_cap = 3 x
// the tree's depth (three waiting siblings per level), which the builder bounds; a push beyond it is not stored and raises the
// overflow flag, upon which the kernel tests every leaf record instead.
//
// Ray box test (bvh_slab; restated in numpy by tests/query_accel_expect.py and tests/occluded_expect.py; fp32, operation by
// operation):
//   pad = rho * (max|o| + cmax)                 cmax: the largest |coordinate| of the child's box, from the node
//   t1 = ((lo - pad) - o) * (1 / d), t2 = ((hi + pad) - o) * (1 / d) per axis; enter = max of the min(t1, t2), exit = min
//   of the max(t1, t2); a NaN among the t1, t2 (0 * inf: the ray runs inside a slab's plane) is reported, and the query then
//   takes no pruning decision.
#pragma once
#include "rt_query.hpp"

namespace rtk {

constexpr uint32_t kBvhEmpty = 0xFFFFFFFFu;
constexpr uint32_t kBvhLeaf = 0x80000000u;

// four child boxes, transposed as the node stores them ([axis][child]), and each box's largest |coordinate|
struct BvhNode {
  float lo[3][4], hi[3][4], cmax[4];
};

__device__ __forceinline__ BvhNode bvh_load_node(const float4* __restrict__ nodes, uint32_t index, uint32_t (&ref)[4]) {
  const float4* const nd = nodes + 8u * static_cast<size_t>(index);
  const float4 lox = nd[0], loy = nd[1], loz = nd[2], hix = nd[3], hiy = nd[4], hiz = nd[5], refs = nd[6], cm = nd[7];
  ref[0] = __float_as_uint(refs.x); ref[1] = __float_as_uint(refs.y); ref[2] = __float_as_uint(refs.z); ref[3] = __float_as_uint(refs.w);
  return {{{lox.x, lox.y, lox.z, lox.w}, {loy.x, loy.y, loy.z, loy.w}, {loz.x, loz.y, loz.z, loz.w}},
          {{hix.x, hix.y, hix.z, hix.w}, {hiy.x, hiy.y, hiy.z, hiy.w}, {hiz.x, hiz.y, hiz.z, hiz.w}},
          {cm.x, cm.y, cm.z, cm.w}};
}

// one 48-byte record: the triangle as the renderer intersects it, and its upload index
struct BvhRecord {
  V3 v0, e1, e2;
  int idx;
};

__device__ __forceinline__ BvhRecord bvh_record(const float4* __restrict__ rec) {
  const float4 A0 = rec[0], A1 = rec[1], B = rec[2];
  return {{A1.z, A1.w, B.x}, {A0.w, A1.x, A1.y}, {A0.x, A0.y, A0.z}, __float_as_int(B.y)};
}

// best first (a 5-exchange network); an empty reference carries -inf, a visited one at least -FLT_MAX
__device__ __forceinline__ void bvh_order4(float (&good)[4], uint32_t (&ref)[4]) {
#define RT_BVH_CSWAP(i, j)                                                                          \
  if (good[i] < good[j]) { const float tg = good[i]; good[i] = good[j]; good[j] = tg;               \
                           const uint32_t tr = ref[i]; ref[i] = ref[j]; ref[j] = tr; }
  RT_BVH_CSWAP(0, 1) RT_BVH_CSWAP(2, 3) RT_BVH_CSWAP(0, 2) RT_BVH_CSWAP(1, 3) RT_BVH_CSWAP(1, 2)
#undef RT_BVH_CSWAP
}

// the line o + t * d against child c's box grown by pad (inv = 1 / d per component); true: a NaN among the six products
__device__ __forceinline__ bool bvh_slab(const BvhNode& nd, int c, float pad, V3 o, V3 inv, float& enter, float& exit) {
  const float t1x = ((nd.lo[0][c] - pad) - o.x) * inv.x, t2x = ((nd.hi[0][c] + pad) - o.x) * inv.x;
  const float t1y = ((nd.lo[1][c] - pad) - o.y) * inv.y, t2y = ((nd.hi[1][c] + pad) - o.y) * inv.y;
  const float t1z = ((nd.lo[2][c] - pad) - o.z) * inv.z, t2z = ((nd.hi[2][c] + pad) - o.z) * inv.z;
  enter = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  exit = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  return __builtin_isunordered(t1x, t2x) || __builtin_isunordered(t1y, t2y) || __builtin_isunordered(t1z, t2z);
}

// The walk of one lane from the root (start; false: nothing is visited), its stack at s_mem's entry * STRIDE + slot.
//   child(node, c)  the goodness of child c: +inf takes no pruning decision (always visited), -inf skips the child, anything
//                   else is a key clamped to >= -FLT_MAX, the larger the earlier
//   leaf(rec)       tests one 48-byte record; true ends the walk (an any-hit query), constant false elsewhere.  The end is a
//                   return value and not a callable of its own, which compiled to a slower leaf loop
//   stale(key)      KEYED only: a popped entry's key has fallen strictly behind what was found meanwhile; it is dropped
// child() is called for all four slots before a reference is looked at (behind `ref != empty &&` the four box tests become
// branches), and a skipped child is known by its -inf alone, its reference stays as loaded.  DESIGN.md 4.3b tells the history of
// these shapes; the runs behind it are not among the committed records.  Returns the overflow flag.
template <uint32_t STRIDE, bool KEYED, class Child, class Leaf, class Stale>
__device__ __forceinline__ bool bvh_walk(const BvhParams& b, float4* s_mem, uint32_t slot, bool start, Child child, Leaf leaf,
                                         Stale stale) {
  uint32_t* const refs = reinterpret_cast<uint32_t*>(s_mem) + slot;
  uint2* const keyed = reinterpret_cast<uint2*>(s_mem) + slot;
  const float inf = __builtin_inff();
  uint32_t sp = 0u;
  uint32_t cur = (b.n_nodes != 0u && start) ? 0u : kBvhEmpty;
  bool overflow = false, done = false;
  while (!done) {
    if (cur == kBvhEmpty) {
      if (sp == 0u) break;
      --sp;
      if constexpr (KEYED) {
        const uint2 e = keyed[sp * STRIDE];
        if (stale(__uint_as_float(e.x))) continue;
        cur = e.y;
      } else {
        cur = refs[sp * STRIDE];
      }
    }
    if ((cur & kBvhLeaf) != 0u) {
      const uint32_t first = cur & 0x0FFFFFFFu, count = ((cur >> 28) & 3u) + 1u;
      for (uint32_t j = 0; j < count && !done; ++j) done = leaf(b.records + 3u * (first + j));
      cur = kBvhEmpty;
      continue;
    }
    uint32_t ref[4];
    const BvhNode nd = bvh_load_node(b.nodes, cur, ref);
    float good[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float g = child(nd, c);                                // (judged whether or not there is a child: no branch)
      good[c] = ref[c] == kBvhEmpty ? -inf : g;
    }
    bvh_order4(good, ref);
    cur = good[0] == -inf ? kBvhEmpty : ref[0];                    // a skipped child keeps its reference; -inf marks it
    auto push = [&](float g, uint32_t r) {
      if (g == -inf) return;
      if (sp < b.stack_cap) {
        if constexpr (KEYED) keyed[sp * STRIDE] = make_uint2(__float_as_uint(g), r);
        else refs[sp * STRIDE] = r;
        ++sp;
      } else overflow = true;                                      // (cannot happen: the capacity is 3 x the tree's depth)
    };
    push(good[3], ref[3]); push(good[2], ref[2]); push(good[1], ref[1]);   // the better of them on top
  }
  return overflow;
}

// the dynamic LDS of a block of `stride` lanes' stacks, and the launch functions' refusal of one that does not fit
uint32_t bvh_stack_lds_bytes(uint32_t stack_cap, uint32_t stride, bool keyed) {
  return stack_cap * stride * (keyed ? 8u : 4u);
}

static bool bvh_stack_fits(uint32_t lds) {
  return lds <= 65536u;                                            // (3 x kBvhMaxDepth entries: 12, 24 or 48 KiB)
}

}  // namespace rtk
