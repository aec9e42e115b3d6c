// What balance.hip (mh_check_balance*), multiplicity.hip (mh_fill_multiplicities*) and range_table.hip (mh_fill_range_table*) share: the
// lane / push-id arithmetic over the planes of a statement's lookup programs, the open-addressing table in HBM and its probe, and the host stage that nets a statement exactly.
// See the header comment of balance.hip for the table's protocol.
#pragma once
#include "../../include/midenhip.h"
#include "air.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include <vector>

static constexpr int BT = 256;  // threads per workgroup of every kernel over lanes / slots

struct BalInst {
  const u64* planes;  // [2 * n_out][n]
  u64 n;              // rows = plane stride
  u64 base;           // first push id (= first lane) of the instance
  u32 K;              // fractions per row
  u32 ext_off;        // offset of its output kinds in BalArgs::ext
  int log_n;          // lane -> (fraction, row) split; 63 for the boundary instance (K = 1, any n)
};
struct BalArgs {
  const BalInst* inst;
  u32 n_inst;
  const unsigned char* ext;  // per instance [2K]: is output (m_0, d_0, m_1, ...) EF-valued?
  u64 total;                 // pushes of all instances, live or not
};
struct BalTable {
  unsigned long long* claim;  // [S] push id + 1 of the claimant, 0 = empty
  unsigned long long* lo[2];  // [S] per coordinate: sum of the multiplicities mod 2^64 (after the final reduction: the net, canonical)
  unsigned long long* hi[2];  // [S] carries out of lo
  unsigned long long* cnt;    // [S] live pushes
  u64 mask;                   // S - 1
};

__device__ __forceinline__ u32 bal_instance(const BalArgs& a, u64 id) {
  u32 i = 0;
  while (i + 1 < a.n_inst && id >= a.inst[i + 1].base) i++;
  return i;
}
// canonical value of output `out` of an instance on row r
__device__ __forceinline__ e2 bal_value(const BalArgs& a, const BalInst& in, u32 out, u64 r) {
  const u64* p = in.planes + (size_t)(2 * out) * in.n + r;
  return e2{gl_canon(p[0]), a.ext[in.ext_off + out] ? gl_canon(p[in.n]) : 0};
}
struct BalLane {
  const BalInst* in;
  u64 row, id;
  u32 k;
};
__device__ __forceinline__ BalLane bal_lane(const BalArgs& a, u64 t) {
  const BalInst& in = a.inst[bal_instance(a, t)];
  const u64 l = t - in.base;
  const u32 k = (u32)(l >> in.log_n);
  const u64 r = l & (((u64)1 << in.log_n) - 1);
  return BalLane{&in, r, in.base + r * in.K + k, k};
}
__device__ __forceinline__ e2 bal_denominator(const BalArgs& a, u64 id) {
  const BalInst& in = a.inst[bal_instance(a, id)];
  const u64 l = id - in.base;
  return bal_value(a, in, 2 * (u32)(l % in.K) + 1, l / in.K);
}
// the keys hold the challenges: uniform already; one multiply-xorshift round spreads both words over the low bits
__device__ __forceinline__ u64 bal_hash(e2 d) {
  u64 x = d.c0 ^ (d.c1 * 0x9E3779B97F4A7C15ULL);
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ULL;
  x ^= x >> 32;
  return x;
}
// INSERT: claim an empty slot on the way.  Otherwise (the table is complete) -> the slot of a key that is present.
template <bool INSERT>
__device__ __forceinline__ u64 bal_probe(const BalArgs& a, const BalTable& tb, e2 d, u64 id) {
  u64 slot = bal_hash(d) & tb.mask;
  for (;;) {  // ends: the load factor is <= 1/2, so an empty slot exists (INSERT); the key was inserted (lookup)
    unsigned long long cur = __hip_atomic_load(&tb.claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (INSERT && cur == 0) {
      cur = atomicCAS(&tb.claim[slot], 0ULL, (unsigned long long)(id + 1));
      if (cur == 0) return slot;
    }
    if (cur == id + 1) return slot;
    if (cur != 0 && e2_eq(bal_denominator(a, cur - 1), d)) return slot;
    if (!INSERT && cur == 0) return slot;  // unreachable for a complete table; never spin
    slot = (slot + 1) & tb.mask;
  }
}
// add a multiplicity to a slot's sums: a 64-bit atomic add per non-zero coordinate, the carry out of the low word on the high word
__device__ __forceinline__ void bal_accumulate(const BalTable& tb, u64 slot, e2 m) {
  const u64 mc[2] = {m.c0, m.c1};
#pragma unroll
  for (int j = 0; j < 2; j++) {
    if (!mc[j]) continue;
    const unsigned long long old = atomicAdd(&tb.lo[j][slot], (unsigned long long)mc[j]);
    if (old + mc[j] < old) atomicAdd(&tb.hi[j][slot], 1ULL);  // the low word wrapped: exactly one of the adders of a wrap sees it
  }
}
// the final reduction of a claimed slot (launch after the inserts): (hi, lo) -> the net multiplicity mod p (into lo); is it non-zero?
__device__ __forceinline__ bool bal_reduce_slot(const BalTable& tb, u64 s) {
  const u64 n0 = gl_reduce128(tb.hi[0][s], tb.lo[0][s]), n1 = gl_reduce128(tb.hi[1][s], tb.lo[1][s]);
  tb.lo[0][s] = n0;
  tb.lo[1][s] = n1;
  return (n0 | n1) != 0;
}

// ---- the host side of balance.hip that multiplicity.hip runs as its verify step ----
struct BalanceInput {
  const mh_lookup* lk;
  const mh_trace* main;
  const mh_trace* prep;
};
struct BalanceReport {
  std::vector<mh_balance_entry> entries;
  std::vector<mh_balance_push> pushes;
  size_t n_pushes = 0;  // exact, also when `pushes` was not collected
};
inline unsigned grid_for(u64 n) { return (unsigned)((n + BT - 1) / BT); }
// planes of the boundary pushes as one more instance (K = 1, m = +-1, d = the denominator): [4][n_boundary]
void balance_boundary_planes(mh_ctx* c, const std::vector<BoundaryPush>& boundary, DevBuf& planes);
// have: null, or per instance the planes of its program over its trace where the caller holds them already (taken over; .p == null: evaluate)
void balance_run(mh_ctx* c, const std::vector<BalanceInput>& in, const std::vector<e2>& rnd, const std::vector<BoundaryPush>& boundary,
                 bool exact, BalanceReport& rep, std::vector<DevBuf>* have = nullptr);
// copy out, count, name the first entry -> MH_OK | MH_ERR_UNSATISFIED
int balance_report(mh_ctx* c, const BalanceReport& rep, const char* const* names, mh_balance_entry* entries, size_t entry_cap,
                   size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);
void balance_validate(mh_ctx* c, const std::vector<BalanceInput>& in);

// ---- the host side of multiplicity.hip that range_table.hip runs as its last stage ----
struct FillInput {
  BalanceInput b;
  mh_trace* main;  // the same trace, writable
  int label;       // the caller's instance number (messages)
};
// probe, insert, resolve, verify over the slots (slots[i].instance indexes `in`); names: per label, or null
void fill_run(mh_ctx* c, const std::vector<FillInput>& in, const std::vector<e2>& rnd, const std::vector<BoundaryPush>& boundary,
              const std::vector<mh_mult_slot>& slots, const char* const* names, u64* n_written, BalanceReport& rep);
