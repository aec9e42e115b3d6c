// The reduce-then-scan pieces the section builders share (hasher_section.hip, ace_section.hip): a block scans a tile of HS_TILE items,
// HS_PER_LANE consecutive ones a lane, as pairs (a saturating at HS_SAT, b plain); one wave (k_hs_carries, defined in
// hasher_section.hip) turns the tile aggregates into what every tile starts from.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

typedef uint32_t u32;

namespace {
constexpr int HS_BT = 256;
constexpr int HS_WAVES = HS_BT / 64;
constexpr int HS_PER_LANE = 4;
constexpr uint32_t HS_TILE = HS_BT * HS_PER_LANE;  // ops (plan) / permutations (ids) of a scan tile; mh_hasher_section_tile() tells the tests
constexpr uint32_t HS_SAT = 1u << 25;              // saturating sums stop here

__device__ __forceinline__ u32 hs_sat(u32 x) { return x < HS_SAT ? x : HS_SAT; }  // x = a + b, a, b <= HS_SAT

// The block's HS_TILE items, HS_PER_LANE consecutive ones a lane, as pairs (a saturating, b plain): ea/eb[j] = carry + everything
// left of the lane's item j; returns through ta/tb the carry + the whole tile.  All HS_BT threads call it.
__device__ __forceinline__ void hs_tile_scan(const u32 (&a)[HS_PER_LANE], const u32 (&b)[HS_PER_LANE], u32 carry_a, u32 carry_b,
                                             u32 (&ea)[HS_PER_LANE], u32 (&eb)[HS_PER_LANE], u32& ta, u32& tb, u32 (*s_wave)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 la = 0, lb = 0;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    la = hs_sat(la + a[j]);
    lb += b[j];
  }
  u32 ia = la, ib = lb;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u32 oa = __shfl_up(ia, off), ob = __shfl_up(ib, off);
    if (lane >= off) {
      ia = hs_sat(ia + oa);
      ib += ob;
    }
  }
  if (lane == 63) {
    s_wave[wave][0] = ia;
    s_wave[wave][1] = ib;
  }
  u32 xa = __shfl_up(ia, 1), xb = __shfl_up(ib, 1);
  if (lane == 0) xa = xb = 0;
  __syncthreads();
  u32 before_a = carry_a, before_b = carry_b;
  ta = carry_a;
  tb = carry_b;
  for (int v = 0; v < HS_WAVES; v++) {
    if (v == wave) {
      before_a = ta;
      before_b = tb;
    }
    ta = hs_sat(ta + s_wave[v][0]);
    tb += s_wave[v][1];
  }
  ea[0] = hs_sat(before_a + xa);
  eb[0] = before_b + xb;
#pragma unroll
  for (int j = 1; j < HS_PER_LANE; j++) {
    ea[j] = hs_sat(ea[j - 1] + a[j - 1]);
    eb[j] = eb[j - 1] + b[j - 1];
  }
}
}  // namespace

// one wave: agg[.][t] := the sum of the aggregates of tiles 0 .. t - 1; the sums over all tiles -> *total_a, *total_b
__global__ void k_hs_carries(uint32_t* __restrict__ agg, uint32_t tiles, unsigned long long* total_a, unsigned long long* total_b);
