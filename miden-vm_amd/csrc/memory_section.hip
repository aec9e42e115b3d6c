// The memory chiplet's trace section built on the device from an access list (mh_memory_section_build, mh_miden_memory_section), gfx950.
//
// Replaces Memory::fill_trace (processor/src/trace/chiplets/memory/mod.rs:308-406, segment.rs): the walk of the
// BTreeMap<ctx, BTreeMap<word, Vec<access>>> is a stable sort by (ctx, word, clk), the word carried through its accesses is a scan, the
// delta against the previous row and its inverse are row-local once the order is known.
//   keys     a lane per access, MS_KEYS_PER_BLOCK accesses per block: kind > 3 (defect 1) and an unaligned word access (defect 2) -> atomicMin on (arrival index, kind);
//            key hi = ctx << 30 | addr >> 2, lo = clk; OR and AND of all keys (wave shuffles, the block's waves through LDS, one atomic
//            per block and word).  The host reads five words back: the call's first wait.  A digit (8 bits) in which OR ^ AND has no
//            bit is the same in every key and its pass is left out.
//   sort     stable LSD radix sort of (hi, lo, arrival index), one pass per remaining digit, three launches each:
//              hist     a wave owns MS_CHUNK consecutive elements; its digit counts (LDS atomics) -> table[digit][chunk]
//              scan     one block per digit: exclusive sum of its row of the table in place, the row's total -> rowsum[digit]
//              scatter  the wave walks its chunk 64 elements at a time: the lanes with the lane's digit from eight ballots, the rank
//                       among them from the lanes below, the chunk's running count per digit in LDS (one leader lane per digit adds
//                       the group's size) -> (sum of rowsum below the digit) + table[digit][chunk] + running + rank.  Equal digits
//                       keep their order.
//   reduce   one block per tile of MS_TILE sorted rows: a row's element is (mask, 4 felts) -- read (0, -), element write (1 << idx, v),
//            word write (15, word) -- and the FIRST row of a (ctx, word) has mask 15 with zeros where it does not write, so it absorbs
//            whatever stands left of it and the plain inclusive scan is the segmented one.  combine(a, b) = (a.mask | b.mask, lane j of
//            b where b has bit j, of a otherwise).  The tile's aggregate -> agg[tile]; the same launch tests every row against its
//            predecessor (defect 3, atomicMin on the later arrival index) and counts words and contexts.
//   carries  one wave scans the aggregates 64 at a time (exclusive: what tile t starts from).
//            The host reads three words back: the second wait, and defect 3 is known before a cell is written.
//   rows     the tile scan again, started from the tile's carry; lane = row: delta, its halves, d_inv (one gl_inv where delta > 1),
//            f_scw, the address halves, 17 column-major stores (consecutive lanes, consecutive rows), row_of[arrival] = row.
// The tile scan takes MS_TILE / MS_BT rounds of one row per lane (wave scan by __shfl_up, the four waves through LDS, the round's
// total carried into the next round), so that loads and stores of a round are consecutive.
// Sums, minima, ORs, ANDs and stable ranks do not depend on the order the atomics land in; every output cell has one writer.
#include "../../include/midenhip.h"
#include "ctx.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include <memory>
#include <string>

typedef uint32_t u32;

namespace {
constexpr int MS_BT = 256;                    // every kernel but the table scan and the one-wave carries; = the digits of a pass
constexpr int MS_WAVES = MS_BT / 64;
static_assert(MS_BT == 256, "k_ms_scatter sums rowsum with one lane per digit");
constexpr u32 MS_KEYS_PER_BLOCK = 16 * MS_BT;  // k_ms_keys: four atomics per block, so few blocks
constexpr u32 MS_CHUNK = 1024;                // elements a wave owns in a sort pass
constexpr u32 MS_TILE = 1024;                 // rows of a carry tile (mh_memory_section_tile() tells the tests)
constexpr int MS_ROUNDS = MS_TILE / MS_BT;
constexpr int MS_SCAN_BT = 1024;              // k_ms_table_scan
constexpr int MS_WIDTH = 17;
constexpr int MS_CHIPLETS_WIDTH = 22;
constexpr u64 MS_MAX_N = (u64)1 << 24;
constexpr unsigned long long MS_NONE = ~0ull;

struct MsWords {                    // what the host reads back
  unsigned long long bad;           // min over defects 1, 2 of (arrival index << 2 | kind)
  unsigned long long or_hi, and_hi, or_lo, and_lo;
  unsigned long long clash;         // min arrival index of defect 3
  unsigned long long n_words, n_contexts;
};

struct MsKeys {
  u64* hi;
  u32* lo;
  u32* idx;
};

struct MsElem {
  u32 mask;
  u64 v[4];
};

__device__ __forceinline__ MsElem ms_combine(const MsElem& a, const MsElem& b) {
  MsElem r;
  r.mask = a.mask | b.mask;
#pragma unroll
  for (int j = 0; j < 4; j++) r.v[j] = ((b.mask >> j) & 1) ? b.v[j] : a.v[j];
  return r;
}
__device__ __forceinline__ MsElem ms_shfl_up(const MsElem& e, int off) {
  MsElem r;
  r.mask = __shfl_up(e.mask, off);
#pragma unroll
  for (int j = 0; j < 4; j++) r.v[j] = __shfl_up((unsigned long long)e.v[j], off);
  return r;
}
__device__ __forceinline__ MsElem ms_wave_scan(MsElem e, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const MsElem o = ms_shfl_up(e, off);
    if (lane >= off) e = ms_combine(o, e);
  }
  return e;
}

__device__ __forceinline__ u32 ms_digit(u64 hi, u32 lo, int pass) { return pass < 4 ? (lo >> (8 * pass)) & 255u : (u32)(hi >> (8 * (pass - 4))) & 255u; }
}  // namespace

// ---- keys ----
__global__ __launch_bounds__(MS_BT) void k_ms_keys(const mh_mem_access* __restrict__ acc, u32 n, MsKeys k, MsWords* __restrict__ w) {
  __shared__ u64 s[MS_WAVES][4];
  u64 or_hi = 0, and_hi = ~(u64)0, or_lo = 0, and_lo = ~(u64)0;
  const u32 first = blockIdx.x * MS_KEYS_PER_BLOCK + threadIdx.x;
#pragma unroll 4
  for (u32 j = 0; j < MS_KEYS_PER_BLOCK; j += MS_BT) {
    const u32 i = first + j;  // < 2^24 + MS_KEYS_PER_BLOCK
    if (i >= n) break;
    const uint4 h = *reinterpret_cast<const uint4*>(&acc[i]);  // ctx, addr, clk, kind
    if (h.w > 3) atomicMin(&w->bad, ((unsigned long long)i << 2) | 1);
    else if ((h.w & 2) && (h.y & 3)) atomicMin(&w->bad, ((unsigned long long)i << 2) | 2);
    const u64 hi = ((u64)h.x << 30) | (h.y >> 2);
    k.hi[i] = hi;
    k.lo[i] = h.z;
    k.idx[i] = i;
    or_hi |= hi; and_hi &= hi;
    or_lo |= h.z; and_lo &= h.z;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    or_hi |= __shfl_xor((unsigned long long)or_hi, off);
    and_hi &= __shfl_xor((unsigned long long)and_hi, off);
    or_lo |= __shfl_xor((unsigned long long)or_lo, off);
    and_lo &= __shfl_xor((unsigned long long)and_lo, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s[wave][0] = or_hi; s[wave][1] = and_hi; s[wave][2] = or_lo; s[wave][3] = and_lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < MS_WAVES; v++) {
      or_hi |= s[v][0]; and_hi &= s[v][1]; or_lo |= s[v][2]; and_lo &= s[v][3];
    }
    atomicOr(&w->or_hi, (unsigned long long)or_hi);
    atomicAnd(&w->and_hi, (unsigned long long)and_hi);
    atomicOr(&w->or_lo, (unsigned long long)or_lo);
    atomicAnd(&w->and_lo, (unsigned long long)and_lo);
  }
}

// ---- sort ----
// table[digit * chunks + chunk]; a block holds MS_WAVES chunks
__global__ __launch_bounds__(MS_BT) void k_ms_hist(MsKeys k, u32 n, int pass, u32 chunks, u32* __restrict__ table) {
  __shared__ u32 cnt[MS_WAVES][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int d = lane; d < 256; d += 64) cnt[wave][d] = 0;
  __syncthreads();
  const u32 chunk = blockIdx.x * MS_WAVES + wave;
  const u32 base = chunk * MS_CHUNK;  // chunk < 2^24 / MS_CHUNK + MS_WAVES: no overflow
  for (u32 e = lane; e < MS_CHUNK; e += 64) {
    const u32 i = base + e;
    if (chunk < chunks && i < n) atomicAdd(&cnt[wave][ms_digit(k.hi[i], k.lo[i], pass)], 1u);
  }
  __syncthreads();
  if (chunk < chunks)
    for (int d = lane; d < 256; d += 64) table[(size_t)d * chunks + chunk] = cnt[wave][d];
}

// block d: exclusive sum of row d of the table in place, the row's total -> rowsum[d]
__global__ __launch_bounds__(MS_SCAN_BT) void k_ms_table_scan(u32* __restrict__ table, u32 chunks, u32* __restrict__ rowsum) {
  __shared__ u32 s_wave[MS_SCAN_BT / 64];
  __shared__ u32 s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32* row = table + (size_t)blockIdx.x * chunks;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (u32 base = 0; base < chunks; base += MS_SCAN_BT) {
    const u32 at = base + threadIdx.x;
    const u32 mine = at < chunks ? row[at] : 0;
    u32 incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 before = s_carry;
    for (int v = 0; v < wave; v++) before += s_wave[v];
    u32 all = 0;
    for (int v = 0; v < MS_SCAN_BT / 64; v++) all += s_wave[v];
    if (at < chunks) row[at] = before + incl - mine;
    __syncthreads();
    if (threadIdx.x == 0) s_carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) rowsum[blockIdx.x] = s_carry;
}

__global__ __launch_bounds__(MS_BT) void k_ms_scatter(MsKeys src, MsKeys dst, u32 n, int pass, u32 chunks, const u32* __restrict__ table,
                                                       const u32* __restrict__ rowsum) {
  __shared__ u32 run[MS_WAVES][256];  // the chunk's elements with digit d met so far
  __shared__ u32 first[256];          // elements with a digit below d: the exclusive sum of rowsum, MS_BT = 256 lanes
  __shared__ u32 s_wave[MS_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int d = lane; d < 256; d += 64) run[wave][d] = 0;
  const u32 mine = rowsum[threadIdx.x];
  u32 incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u32 o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  u32 before = 0;
  for (int v = 0; v < wave; v++) before += s_wave[v];
  first[threadIdx.x] = before + incl - mine;
  __syncthreads();
  const u32 chunk = blockIdx.x * MS_WAVES + wave;
  if (chunk >= chunks) return;  // whole waves leave: no block barrier follows
  const u32 base = chunk * MS_CHUNK;
  const u64 below = ((u64)1 << lane) - 1;
  for (u32 e = 0; e < MS_CHUNK; e += 64) {
    const u32 i = base + e + lane;
    const bool valid = i < n;
    u64 hi = 0;
    u32 lo = 0, idx = 0, d = 0;
    if (valid) {
      hi = src.hi[i]; lo = src.lo[i]; idx = src.idx[i];
      d = ms_digit(hi, lo, pass);
    }
    u64 same = __ballot(valid);  // the valid lanes of the wave that hold this lane's digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1;
      const u64 vote = __ballot(bit);
      same &= bit ? vote : ~vote;
    }
    const u32 rank = __popcll(same & below), group = __popcll(same);
    u32 start = 0;
    if (valid && rank == 0) {  // one leader per digit: no two lanes touch one counter
      start = run[wave][d];
      run[wave][d] = start + group;
    }
    const int leader = same ? __ffsll((long long)same) - 1 : lane;
    start = __shfl(start, leader);
    if (valid) {
      const u32 to = first[d] + table[(size_t)d * chunks + chunk] + start + rank;
      if (to < n) {  // always: hist and scatter count the same digits
        dst.hi[to] = hi; dst.lo[to] = lo; dst.idx[to] = idx;
      }
    }
  }
}

// ---- carry ----
namespace {
struct MsRun {
  const mh_mem_access* acc;
  MsKeys k;  // sorted
  u32 n;
  u32 tiles;
  u32* agg_mask;  // [tiles]
  u64* agg_v;     // [4][tiles]
  MsWords* w;
};

struct MsRow {
  u64 hi, phi;    // key and the previous row's (row 0: its own)
  u32 lo, plo;
  u32 arrival, kind, addr;
  bool same_word, same_key;  // as the previous row; row 0: same_word as the reference starts it, never same_key
  MsElem e;
};

// everything row r is made of.  r < a.n
__device__ __forceinline__ MsRow ms_row(const MsRun& a, u32 r) {
  MsRow x;
  x.hi = a.k.hi[r];
  x.lo = a.k.lo[r];
  x.arrival = a.k.idx[r];
  if (x.arrival >= a.n) x.arrival = a.n - 1;  // never: the sorted indices are a permutation.  No index read from memory goes unchecked
  x.phi = r ? a.k.hi[r - 1] : x.hi;
  x.plo = r ? a.k.lo[r - 1] : x.lo;
  x.same_word = x.phi == x.hi;
  x.same_key = r && x.same_word && x.plo == x.lo;
  const mh_mem_access* p = a.acc + x.arrival;
  const uint4 h = *reinterpret_cast<const uint4*>(p);
  x.addr = h.y;
  x.kind = h.w;
  const bool first = !r || !x.same_word;
  x.e.mask = first ? 15u : 0u;
#pragma unroll
  for (int j = 0; j < 4; j++) x.e.v[j] = 0;
  if (!(x.kind & 1)) {
    if (x.kind & 2) {
      x.e.mask = 15u;
#pragma unroll
      for (int j = 0; j < 4; j++) x.e.v[j] = gl_canon(p->value[j]);
    } else {
      const u32 at = x.addr & 3;
      const u64 v = gl_canon(p->value[0]);
      x.e.mask |= 1u << at;
#pragma unroll
      for (int j = 0; j < 4; j++) x.e.v[j] = (u32)j == at ? v : 0;
    }
  }
  return x;
}

// Inclusive scan of the tile's elements from `carry`, MS_ROUNDS rounds of one row per lane.  mine[j]: the word after the row of round
// j (meaningless for a row >= n).  Returns carry . tile.  All MS_BT threads call it.
__device__ __forceinline__ MsElem ms_tile_scan(MsElem carry, const MsElem (&in)[MS_ROUNDS], MsElem (&mine)[MS_ROUNDS], MsElem (*s_wave)[MS_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MS_ROUNDS; j++) {
    MsElem e = ms_wave_scan(in[j], lane);
    if (lane == 63) s_wave[j][wave] = e;
    __syncthreads();  // s_wave[j] is this round's own: one barrier per round
    MsElem before = carry;
    for (int v = 0; v < MS_WAVES; v++) {
      if (v == wave) mine[j] = ms_combine(before, e);
      before = ms_combine(before, s_wave[j][v]);
    }
    carry = before;
  }
  return carry;
}

__device__ __forceinline__ MsElem ms_identity() { return MsElem{0u, {0, 0, 0, 0}}; }
}  // namespace

__global__ __launch_bounds__(MS_BT) void k_ms_reduce(MsRun a) {
  __shared__ MsElem s_wave[MS_ROUNDS][MS_WAVES];
  __shared__ u32 s_cnt[MS_WAVES][2];
  const u32 tile = blockIdx.x;
  MsElem in[MS_ROUNDS], mine[MS_ROUNDS];
  u32 words = 0, contexts = 0;
#pragma unroll
  for (int j = 0; j < MS_ROUNDS; j++) {
    const u32 r = tile * MS_TILE + j * MS_BT + threadIdx.x;
    in[j] = ms_identity();
    if (r < a.n) {
      const MsRow x = ms_row(a, r);
      in[j] = x.e;
      words += !r || !x.same_word;
      contexts += !r || (x.phi >> 30) != (x.hi >> 30);
      if (x.same_key) {
        // IllegalMemoryAccess: two accesses of one word in one cycle, one of them a write.  The later one is reported
        const u32 pkind = a.acc[a.k.idx[r - 1]].kind;
        if (!(x.kind & 1) || !(pkind & 1)) atomicMin(&a.w->clash, (unsigned long long)x.arrival);
      }
    }
  }
  const MsElem total = ms_tile_scan(ms_identity(), in, mine, s_wave);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    words += __shfl_xor(words, off);
    contexts += __shfl_xor(contexts, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_cnt[threadIdx.x >> 6][0] = words;
    s_cnt[threadIdx.x >> 6][1] = contexts;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.agg_mask[tile] = total.mask;
#pragma unroll
    for (int j = 0; j < 4; j++) a.agg_v[(size_t)j * a.tiles + tile] = total.v[j];
    u32 ws = 0, cs = 0;
    for (int v = 0; v < MS_WAVES; v++) {
      ws += s_cnt[v][0];
      cs += s_cnt[v][1];
    }
    if (ws) atomicAdd(&a.w->n_words, (unsigned long long)ws);
    if (cs) atomicAdd(&a.w->n_contexts, (unsigned long long)cs);
  }
}

// one wave: agg[t] := the combination of the aggregates of tiles 0 .. t - 1
__global__ __launch_bounds__(64) void k_ms_carries(MsRun a) {
  const int lane = threadIdx.x;
  MsElem carry = ms_identity();
  for (u32 base = 0; base < a.tiles; base += 64) {
    const u32 t = base + lane;
    MsElem e = ms_identity();
    if (t < a.tiles) {
      e.mask = a.agg_mask[t];
#pragma unroll
      for (int j = 0; j < 4; j++) e.v[j] = a.agg_v[(size_t)j * a.tiles + t];
    }
    const MsElem incl = ms_combine(carry, ms_wave_scan(e, lane));
    MsElem ex = ms_shfl_up(incl, 1);
    if (lane == 0) ex = carry;
    if (t < a.tiles) {
      a.agg_mask[t] = ex.mask;
#pragma unroll
      for (int j = 0; j < 4; j++) a.agg_v[(size_t)j * a.tiles + t] = ex.v[j];
    }
    carry.mask = __shfl(incl.mask, 63);
#pragma unroll
    for (int j = 0; j < 4; j++) carry.v[j] = __shfl((unsigned long long)incl.v[j], 63);
  }
}

// ---- rows ----
namespace {
struct MsOut {
  u64* base;      // column 0, row 0 of the matrix written into
  u64 height;     // its rows
  u32 col0;       // first of the 17 columns
  u64 row0;       // first of the n rows
  int selectors;  // also columns 0..2 := 1, 1, 0
  u32* row_of;    // [n]
};
}  // namespace

__global__ __launch_bounds__(MS_BT) void k_ms_rows(MsRun a, MsOut o) {
  __shared__ MsElem s_wave[MS_ROUNDS][MS_WAVES];
  const u32 tile = blockIdx.x;
  MsElem carry;
  carry.mask = a.agg_mask[tile];
#pragma unroll
  for (int j = 0; j < 4; j++) carry.v[j] = a.agg_v[(size_t)j * a.tiles + tile];
  MsElem in[MS_ROUNDS], mine[MS_ROUNDS];
  // what a row needs besides its word: kept small across the scan
  u32 ctx[MS_ROUNDS], addr[MS_ROUNDS], clk[MS_ROUNDS], kind[MS_ROUNDS], delta[MS_ROUNDS], scw[MS_ROUNDS], arrival[MS_ROUNDS];
#pragma unroll
  for (int j = 0; j < MS_ROUNDS; j++) {
    const u32 r = tile * MS_TILE + j * MS_BT + threadIdx.x;
    in[j] = ms_identity();
    ctx[j] = addr[j] = clk[j] = kind[j] = delta[j] = scw[j] = arrival[j] = 0;
    if (r < a.n) {
      const MsRow x = ms_row(a, r);
      in[j] = x.e;
      ctx[j] = (u32)(x.hi >> 30);
      addr[j] = x.addr;
      clk[j] = x.lo;
      kind[j] = x.kind;
      arrival[j] = x.arrival;
      scw[j] = x.same_word;
      const u32 pctx = (u32)(x.phi >> 30);
      // the reference starts from (ctx, word, clk - 1): row 0 has delta 1, for clk = 0 too
      if (!r) delta[j] = 1;
      else if (pctx != ctx[j]) delta[j] = ctx[j] - pctx;
      else if (!x.same_word) delta[j] = ((u32)x.hi - (u32)x.phi) << 2;  // word addresses: both word indices lie below 2^30
      else delta[j] = x.lo - x.plo;
    }
  }
  ms_tile_scan(carry, in, mine, s_wave);
#pragma unroll
  for (int j = 0; j < MS_ROUNDS; j++) {
    const u32 r = tile * MS_TILE + j * MS_BT + threadIdx.x;
    if (r >= a.n) continue;
    const u32 is_word = (kind[j] >> 1) & 1, at = is_word ? 0 : addr[j] & 3, widx = addr[j] >> 2;
    const u64 d = delta[j];
    const u64 d_inv = d > 1 ? gl_inv(d) : d;
    u64* cell = o.base + (size_t)o.col0 * o.height + o.row0 + r;
    const u64 row[MS_WIDTH] = {kind[j] & 1, is_word, ctx[j], (u64)(addr[j] & ~3u), at & 1, at >> 1, clk[j], mine[j].v[0], mine[j].v[1],
                               mine[j].v[2], mine[j].v[3], d & 0xFFFF, d >> 16, d_inv, scw[j], widx & 0xFFFF, widx >> 16};
#pragma unroll
    for (int c = 0; c < MS_WIDTH; c++) cell[(size_t)c * o.height] = row[c];
    if (o.selectors) {
      u64* sel = o.base + o.row0 + r;
      sel[0] = 1;
      sel[o.height] = 1;
      sel[2 * o.height] = 0;
    }
    o.row_of[arrival[j]] = r;
  }
}

// ---- host ----
namespace {
unsigned ms_grid(u64 n, u64 per_block) { return (unsigned)((n + per_block - 1) / per_block); }

void ms_fill_info(mh_mem_section_info* info, u64 rows, u64 words, u64 contexts, int log_n, int defect, u64 index) {
  if (!info) return;
  info->n_rows = rows;
  info->n_words = words;
  info->n_contexts = contexts;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_index = index;
}

[[noreturn]] void ms_refuse(mh_mem_section_info* info, u64 words, u64 contexts, int log_n, int defect, u64 index, const mh_mem_access* acc,
                            const char* entry) {
  ms_fill_info(info, 0, words, contexts, log_n, defect, index);
  char buf[256];
  const unsigned long long i = index;
  switch (defect) {
    case 1: snprintf(buf, sizeof buf, "%s: defect 1, access %llu has kind %u (bit 0 = read, bit 1 = word access)", entry, i, acc[index].kind); break;
    case 2: snprintf(buf, sizeof buf, "%s: defect 2, access %llu is a word access of address %u, which is not a multiple of 4", entry, i, acc[index].addr); break;
    case 3:
      snprintf(buf, sizeof buf, "%s: defect 3, access %llu meets another access of its word (context %u, address %u) in cycle %u and one of them writes",
               entry, i, acc[index].ctx, acc[index].addr & ~3u, acc[index].clk);
      break;
    default: snprintf(buf, sizeof buf, "%s: defect 4, the section does not fit: access %llu is the first without a row", entry, i);
  }
  throw MhError(MH_ERR_INVALID, buf);
}

// the section of `acc` into o (o.row_of is set here).  n >= 1, the target has room.  Returns after the second read-back with the rows
// kernel enqueued, or after the copy of row_of when the caller wants it
void ms_run(mh_ctx* c, const mh_mem_access* acc, size_t n, MsOut o, uint32_t* row_of, mh_mem_section_info* info, int log_n, const char* entry) {
  const u32 chunks = ms_grid(n, MS_CHUNK), tiles = ms_grid(n, MS_TILE);
  const size_t table_entries = (size_t)256 * chunks;
  DevBuf dacc(n * sizeof(mh_mem_access)), words(sizeof(MsWords));
  DevBuf hi[2] = {DevBuf(n * 8), DevBuf(n * 8)}, lo[2] = {DevBuf(n * 4), DevBuf(n * 4)}, idx[2] = {DevBuf(n * 4), DevBuf(n * 4)};
  DevBuf table(table_entries * 4), rowsum(256 * 4), agg_mask((size_t)tiles * 4), agg_v((size_t)tiles * 32), drow_of(n * 4);
  MsWords* dw = (MsWords*)words.p;
  const MsWords init{MS_NONE, 0, MS_NONE, 0, MS_NONE, MS_NONE, 0, 0};
  c->h2d(words.p, &init, sizeof init);
  c->h2d(dacc.p, acc, n * sizeof(mh_mem_access));
  const mh_mem_access* da = (const mh_mem_access*)dacc.p;
  MsKeys k[2] = {MsKeys{hi[0].u(), (u32*)lo[0].p, (u32*)idx[0].p}, MsKeys{hi[1].u(), (u32*)lo[1].p, (u32*)idx[1].p}};
  {
    ProfScope ps(c, "ms_keys", 32.0 * (double)n);
    MH_LAUNCH(k_ms_keys, dim3(ms_grid(n, MS_KEYS_PER_BLOCK)), dim3(MS_BT), 0, c->stream, da, (u32)n, k[0], dw);
  }
  MsWords w;
  c->d2h(&w, words.p, sizeof w);  // the first wait: defects 1 and 2, and the digits that vary
  if (w.bad != MS_NONE) ms_refuse(info, 0, 0, log_n, (int)(w.bad & 3), w.bad >> 2, acc, entry);
  int cur = 0;
  for (int pass = 0; pass < 12; pass++) {
    const u64 varies = pass < 4 ? ((w.or_lo ^ w.and_lo) >> (8 * pass)) & 255 : ((w.or_hi ^ w.and_hi) >> (8 * (pass - 4))) & 255;
    if (!varies) continue;
    {
      ProfScope ps(c, "ms_hist", 12.0 * (double)n);
      MH_LAUNCH(k_ms_hist, dim3(ms_grid(chunks, MS_WAVES)), dim3(MS_BT), 0, c->stream, k[cur], (u32)n, pass, chunks, (u32*)table.p);
    }
    {
      ProfScope ps(c, "ms_table_scan", 8.0 * (double)table_entries);
      MH_LAUNCH(k_ms_table_scan, dim3(256), dim3(MS_SCAN_BT), 0, c->stream, (u32*)table.p, chunks, (u32*)rowsum.p);
    }
    {
      ProfScope ps(c, "ms_scatter", 32.0 * (double)n);
      MH_LAUNCH(k_ms_scatter, dim3(ms_grid(chunks, MS_WAVES)), dim3(MS_BT), 0, c->stream, k[cur], k[cur ^ 1], (u32)n, pass, chunks,
                (const u32*)table.p, (const u32*)rowsum.p);
    }
    cur ^= 1;
  }
  MsRun a{da, k[cur], (u32)n, tiles, (u32*)agg_mask.p, agg_v.u(), dw};
  {
    ProfScope ps(c, "ms_reduce", 64.0 * (double)n);
    MH_LAUNCH(k_ms_reduce, dim3(tiles), dim3(MS_BT), 0, c->stream, a);
  }
  {
    ProfScope ps(c, "ms_carries", 72.0 * (double)tiles);
    MH_LAUNCH(k_ms_carries, dim3(1), dim3(64), 0, c->stream, a);
  }
  c->d2h(&w, words.p, sizeof w);  // the second wait: defect 3 before anything is written
  if (w.clash != MS_NONE) ms_refuse(info, w.n_words, w.n_contexts, log_n, 3, w.clash, acc, entry);
  o.row_of = (u32*)drow_of.p;
  {
    ProfScope ps(c, "ms_rows", (64.0 + 8.0 * MS_WIDTH) * (double)n);
    MH_LAUNCH(k_ms_rows, dim3(tiles), dim3(MS_BT), 0, c->stream, a, o);
  }
  if (row_of) c->d2h(row_of, drow_of.p, n * 4);
  ms_fill_info(info, n, w.n_words, w.n_contexts, log_n, 0, 0);
}
}  // namespace

#define MS_CATCH                    \
  catch (const MhError& e) {        \
    c->err = e.what();              \
    return e.code;                  \
  }                                 \
  catch (const std::exception& e) { \
    c->err = e.what();              \
    return MH_ERR_INTERNAL;         \
  }

extern "C" uint32_t mh_memory_section_tile(void) { return MS_TILE; }

extern "C" int mh_memory_section_build(mh_ctx* c, const mh_mem_access* accesses, size_t n, int log_n, mh_trace** out, uint32_t* row_of,
                                       mh_mem_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_memory_section_build";
    if (out) *out = nullptr;
    ms_fill_info(info, 0, 0, 0, log_n, 0, 0);
    MH_REQUIRE(out && (accesses || !n), "mh_memory_section_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_memory_section_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(n <= MS_MAX_N, "mh_memory_section_build: more than 2^24 accesses");
    if (log_n < 0)
      for (log_n = 6; ((u64)1 << log_n) < n; log_n++) {}
    const u64 height = (u64)1 << log_n;
    if (n > height) ms_refuse(info, 0, 0, log_n, 4, height, accesses, entry);
    HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<mh_trace> t = trace_new(c, log_n, MS_WIDTH);
    if (n < height)  // rows [n, height) of every column
      HIP_CHECK(hipMemset2DAsync(t->cols.u() + n, height * 8, 0, (height - n) * 8, MS_WIDTH, c->stream));
    ms_fill_info(info, 0, 0, 0, log_n, 0, 0);
    if (n) ms_run(c, accesses, n, MsOut{t->cols.u(), height, 0, 0, 0, nullptr}, row_of, info, log_n, entry);
    *out = t.release();
    return MH_OK;
  }
  MS_CATCH
}

extern "C" int mh_miden_memory_section(mh_ctx* c, mh_trace* chiplets, uint64_t start_row, const mh_mem_access* accesses, size_t n,
                                       uint32_t* row_of, mh_mem_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_miden_memory_section";
    ms_fill_info(info, 0, 0, 0, 0, 0, 0);
    MH_REQUIRE(chiplets && (accesses || !n), "mh_miden_memory_section: null argument");
    MH_REQUIRE(chiplets->ctx == c, "mh_miden_memory_section: the chiplets trace belongs to another context");
    MH_REQUIRE(chiplets->width == MS_CHIPLETS_WIDTH, "mh_miden_memory_section: the chiplets trace is 22 columns wide");
    MH_REQUIRE(chiplets->log_n >= 0 && chiplets->log_n <= 32, "mh_miden_memory_section: bad chiplets height");
    MH_REQUIRE(n <= MS_MAX_N, "mh_miden_memory_section: more than 2^24 accesses");
    const u64 height = (u64)1 << chiplets->log_n;
    ms_fill_info(info, 0, 0, 0, chiplets->log_n, 0, 0);
    if (start_row > height || n > height - start_row)
      ms_refuse(info, 0, 0, chiplets->log_n, 4, start_row < height ? height - start_row : 0, accesses, entry);
    if (!n) return MH_OK;
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    ms_run(c, accesses, n, MsOut{chiplets->cols.u(), height, 3, start_row, 1, nullptr}, row_of, info, chiplets->log_n, entry);
    return MH_OK;
  }
  MS_CATCH
}
