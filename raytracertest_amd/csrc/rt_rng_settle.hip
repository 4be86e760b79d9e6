// rt_rng_settle.hip -- rng_settle_kernel: the RNG draws a tracer owes to its certain-winner tiles (rt_tracer::settle).
// A translation unit of its own, compiled like rt_rng_init.hip with the default machine scheduler (the max-ILP strategy
// hoists all 80 LDS look-ups of a table product).
#include "rt_device_math.hpp"
#include "rt_kernels.hpp"

namespace rtk {

using rtd::Rng;

// ------------------------------------------------------------------------------------
// Small-scene trace launches flagged TRACE_OWE_RNG leave the xorshift words v0..v4 of the pixels of certain-winner tiles
// untouched; the host sums what they would have drawn (rt_tracer::owed_draws).  This kernel pays the debt: every 8x8 tile
// whose list header has the certain bit loads v0..v4, advances them by `draws` steps and stores them.  The xorshift step
// is linear over GF(2), so `draws` steps are one product by T^draws: 40 look-ups in the 4-bit window table of that one
// matrix (rt_rng_host.hpp, 12.5 KiB, staged into LDS once per block); few draws are cheaper stepped (table == null).
// Geometry as in the trace kernel: one wave per tile, a 256-thread block covers the four tiles of 32 x 8 pixels, so that
// no 128-byte line is shared between blocks; the blocks are persistent and walk over the (half-)launch's block grid,
// (gx, gy, row_il, row_phase) being those of the trace launches that owe.  Out-of-image lanes do nothing.
// ------------------------------------------------------------------------------------
constexpr uint32_t kSettleWinEntries = 40u * 16u;

struct SettleParams {
  uint32_t* rng;               // the (half-)launch's planes: stride npix, plane k at k * npix
  const uint32_t* tile_lists;  // the (half-)launch's slots: 1 + bin_list words per tile, word 0 the header
  uint32_t W, rows, npix, bin_list;
  uint32_t gx, gy;             // block grid of the trace launch
  uint32_t row_il, row_phase;
  uint32_t draws;
  const uint32_t* table;       // window table of T^draws, or null: step
};

__global__ __launch_bounds__(256) void rng_settle_kernel(const SettleParams s) {
  extern __shared__ uint4 s_win[];                                   // kSettleWinEntries x words 0..3, then x word 4
  uint32_t* const s_w4 = reinterpret_cast<uint32_t*>(s_win + kSettleWinEntries);
  const bool tabled = s.table != nullptr;                            // block-uniform
  if (tabled) {
    for (uint32_t i = threadIdx.x; i < kSettleWinEntries; i += 256u) {
      s_win[i] = reinterpret_cast<const uint4*>(s.table)[i];
      s_w4[i] = s.table[kSettleWinEntries * 4u + i];
    }
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t blocks = s.gx * s.gy;
  for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {        // block-uniform; no barrier inside
    const uint32_t bx = b % s.gx;
    uint32_t by = b / s.gx;
    if (s.row_il != 0u) by = (by / s.row_il) * (2u * s.row_il) + s.row_phase * s.row_il + by % s.row_il;
    const size_t slot = (static_cast<size_t>(by) * s.gx + bx) * 4u + wave;
    const uint32_t word = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s.tile_lists[slot * (1u + s.bin_list)])));
    if ((word >> 31) == 0u) continue;                                // wave-uniform: the tile traced its rays and kept its states current
    const uint32_t px = bx * 32u + wave * 8u + (lane & 7u);
    const uint32_t ly = by * 8u + (lane >> 3);
    if (!(px < s.W && ly < s.rows)) continue;
    const size_t pix = static_cast<size_t>(px) + static_cast<size_t>(ly) * s.W;
    const size_t np = s.npix;
    uint32_t v[5] = {s.rng[1 * np + pix], s.rng[2 * np + pix], s.rng[3 * np + pix], s.rng[4 * np + pix], s.rng[5 * np + pix]};
    if (tabled) {
      uint32_t r0 = 0u, r1 = 0u, r2 = 0u, r3 = 0u, r4 = 0u;
#pragma unroll 1
      for (uint32_t w = 0; w < 5u; ++w) {                            // the eight nibbles of one state word at a time
        const uint32_t vw = w == 0u ? v[0] : w == 1u ? v[1] : w == 2u ? v[2] : w == 3u ? v[3] : v[4];   // (no indexed register file)
        const uint4* __restrict__ Tw = s_win + w * 128u;
        const uint32_t* __restrict__ T4w = s_w4 + w * 128u;
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
          const uint32_t n = (vw >> (q * 4u)) & 15u;
          const uint4 e = Tw[q * 16u + n];
          r0 ^= e.x; r1 ^= e.y; r2 ^= e.z; r3 ^= e.w;
          r4 ^= T4w[q * 16u + n];
        }
      }
      v[0] = r0; v[1] = r1; v[2] = r2; v[3] = r3; v[4] = r4;
    } else {
      Rng g = {0u, v[0], v[1], v[2], v[3], v[4]};
      rtd::rng_discard(g, s.draws);
      v[0] = g.v0; v[1] = g.v1; v[2] = g.v2; v[3] = g.v3; v[4] = g.v4;
    }
    s.rng[1 * np + pix] = v[0];
    s.rng[2 * np + pix] = v[1];
    s.rng[3 * np + pix] = v[2];
    s.rng[4 * np + pix] = v[3];
    s.rng[5 * np + pix] = v[4];
  }
}

hipError_t launch_rng_settle(const TraceParams& p, uint32_t draws, const uint32_t* table, hipStream_t st) {
  if (draws == 0u || p.tile_lists == nullptr || p.rng == nullptr || p.rows == 0u || p.W == 0u) return hipSuccess;
  const dim3 grid = trace_grid(p);
  if (grid.y == 0u) return hipSuccess;
  const SettleParams s = {p.rng, p.tile_lists, p.W, p.rows, p.npix, p.bin_list, grid.x, grid.y, p.row_il, p.row_phase, draws, table};
  const uint32_t blocks = grid.x * grid.y;
  // persistent blocks: with a table eight per CU stage it once each and walk the grid
  const uint32_t launch = table != nullptr && blocks > 2048u ? 2048u : blocks;
  hipLaunchKernelGGL(rng_settle_kernel, dim3(launch), dim3(256), table != nullptr ? kSettleWinEntries * 20u : 0u, st, s);
  return hipGetLastError();
}

}  // namespace rtk
