// The hasher controller's trace section built on the device from an op list (mh_hasher_section_build, mh_miden_hasher_section), gfx950.
//
// Replaces the controller side of Hasher (processor/src/trace/chiplets/hasher/mod.rs:131-480: permute, hash_control_block,
// hash_basic_block, build_merkle_root, update_merkle_root, append_controller_permutation, record_perm_request; trace.rs:91-139 for the
// padding): two rows per permutation, the second of which is a Poseidon2 output, and the first-appearance numbering of the distinct
// pre-states.
//   plan     a lane per op, four consecutive ops a lane, HS_TILE ops a block: kind, count, index and operand range are checked (the
//            lowest (op, defect) -> one atomicMin), the op's permutations and its MRUPDATE flag are summed per tile -> agg[tile].
//   carries  one wave scans the tile aggregates 64 at a time (exclusive: what tile t starts from); the totals -> two words.
//   offsets  the tile scan again, started from the tile's carry: first_perm[op], mru[op] (the mrupdate_id its rows carry),
//            chain_op[op + updates before it (+ 1 for the new leg)] = op << 1 | leg, and the lowest op whose rows end beyond the target
//            (defect 5), and the number of chains per length (a histogram of 64 buckets, summed per block in LDS first).  The host
//            reads the words back: the first wait.  Nothing but scratch has been written.
//   order    a lane per chain: the chains laid out by length, longest first (bucket = 64 - min(length, 64); a block counts its chains
//            per bucket in LDS, reserves its range of every bucket with one atomicAdd and places its chains inside it).  Which place
//            a chain gets inside its bucket depends on the order the atomics land in; no output does, because every chain writes by
//            permutation index.  Why: a wave of the chains kernel takes as long as its longest lane, and in program order a depth-32
//            path sits next to single permutations (2.98 ms -> 1.64 ms on the mixed list of 2^20 rows).
//   chains   a lane per dependent chain (a permute, a control block, a basic block, a Merkle leg; the two legs of an update are two
//            chains), one wave a block: the lane walks its chain with p2_permute and writes per permutation the canonical pre- and
//            post-state, 192 consecutive bytes, perm_op[perm] = op, and at the end the op's mh_hash_result.
//   insert   a lane per permutation: open addressing (linear probing from a 64-bit mix of the pre-state) into a table of permutation
//            indices; a slot is won by atomicCAS, an occupied slot is compared by its owner's FULL pre-state.  slot_of[perm] = the slot
//            of the perm's state, least[slot] = atomicMin of the perms that met there: the first appearance, whoever won the slot.
//   flags    perm is a representative when least[slot_of[perm]] == perm; their count per tile -> agg[tile]
//   carries  as above; the total is n_requests.  The host reads it back: the second wait (n_requests is part of `info` and is not
//            known before the chains have run).
//   ranks    the tile scan again: rank[perm] = representatives below perm, so perm_id(perm) = rank[least[slot_of[perm]]]
//   rows     a lane per controller row, padding included: the op from perm_op, the position from first_perm, selectors, node_index,
//            boundary and direction from the op header, the state from the chains' scratch (96 consecutive bytes a row), 20 (or 21)
//            column-major stores, consecutive lanes on consecutive rows.
// The permutation count is a saturating sum (min(a + b, 2^25): associative and commutative on [0, 2^25]), so a count field of 2^32 - 1
// overflows nothing and "more than 2^24 permutations" is read from the same words.  Sums, minima and slot winners' states do not depend
// on the order the atomics land in (which perm wins a slot does, the slot's least member does not); every output cell has one writer.
#include "../../include/midenhip.h"
#include "ctx.hpp"
#include "gl.cuh"
#include "hs_scan.cuh"
#include "kernels.hpp"
#include "poseidon2.cuh"
#include <memory>
#include <string>

typedef uint32_t u32;

static_assert(sizeof(mh_hash_op) == 24, "mh_hash_op is 24 bytes");
static_assert(sizeof(mh_hash_result) == 136, "mh_hash_result is 17 words");

namespace {
constexpr int HS_CHAIN_BT = 64;               // k_hs_chains: one wave a block, so that long chains spread over the CUs
constexpr int HS_WIDTH = 20;
constexpr int HS_CHIPLETS_WIDTH = 22;
constexpr u32 HS_MAX_PERMS = 1u << 24;
constexpr u32 HS_BUCKETS = 64;                // chain lengths 64.., 63, .., 1
constexpr u32 HS_EMPTY = 0xFFFFFFFFu;
constexpr unsigned long long HS_NONE = ~0ull;

struct HsWords {                 // what the host reads back
  unsigned long long bad;        // min over defects 1..4 of (op << 3 | kind)
  unsigned long long nofit;      // lowest op whose rows end beyond the target
  unsigned long long n_perms;    // saturating
  unsigned long long n_updates;  // = the final mrupdate_id
  unsigned long long n_requests;
  unsigned long long unused;
};

struct HsPlan {
  u32 perms, mru, defect;
};

// what op `o` asks for, and the first defect it has in the order 1, 2, 3, 4
__device__ __forceinline__ HsPlan hs_plan_op(const mh_hash_op& o, u64 n_felts) {
  HsPlan p{0, 0, 0};
  u64 need;
  if (o.kind > 4) {
    p.defect = 1;
    return p;
  }
  if (o.kind == 0) {
    p.perms = 1;
    need = 12;
  } else if (o.kind == 1) {
    p.perms = 1;
    need = 8;
  } else if (o.kind == 2) {
    if (o.count == 0) {
      p.defect = 2;
      return p;
    }
    p.perms = o.count < HS_SAT ? o.count : HS_SAT;
    need = 8 * (u64)o.count;
  } else {
    if (o.count == 0 || o.count > 64) {
      p.defect = 2;
      return p;
    }
    const u32 legs = o.kind == 4 ? 2 : 1;
    p.perms = legs * o.count;
    p.mru = o.kind == 4;
    need = 4 * legs + 4 * (u64)o.count;
    if (o.index >= GL_P || (o.count < 64 && (o.index >> o.count) != 0)) {
      p.defect = 3;
      return p;
    }
  }
  if (o.payload > n_felts || need > n_felts - o.payload) p.defect = 4;
  return p;
}

struct HsRun {
  const mh_hash_op* ops;
  u32 n_ops;
  const u64* felts;
  u64 n_felts;
  u64 cap_rows;     // rows of the target
  u32* agg;         // [2][tiles]
  u32 tiles;
  u32* first_perm;  // [n_ops]
  u32* mru;         // [n_ops]
  u32* chain_op;    // [2 * n_ops]
  u32* hist;        // [HS_BUCKETS] chains per length bucket, then [HS_BUCKETS] cursors of k_hs_order
  HsWords* w;
};

// the bucket of a chain of op `o`: longest first
__device__ __forceinline__ u32 hs_bucket(const mh_hash_op& o) {
  const u32 len = o.kind < 2 ? 1 : o.count;
  return HS_BUCKETS - (len < 1 ? 1 : len > HS_BUCKETS ? HS_BUCKETS : len);
}
}  // namespace

// ---- plan ----
__global__ __launch_bounds__(HS_BT) void k_hs_plan(HsRun r) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 a[HS_PER_LANE], b[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;  // < 2^24 + HS_TILE
    a[j] = b[j] = 0;
    if (i < r.n_ops) {
      const mh_hash_op o = r.ops[i];
      const HsPlan p = hs_plan_op(o, r.n_felts);
      a[j] = p.perms;
      b[j] = p.mru;
      if (p.defect) atomicMin(&r.w->bad, ((unsigned long long)i << 3) | p.defect);
    }
  }
  hs_tile_scan(a, b, 0, 0, ea, eb, ta, tb, s_wave);
  if (threadIdx.x == 0) {
    r.agg[blockIdx.x] = ta;
    r.agg[r.tiles + blockIdx.x] = tb;
  }
}

// one wave: agg[.][t] := the sum of the aggregates of tiles 0 .. t - 1; the sums over all tiles -> *total_a, *total_b
__global__ __launch_bounds__(64) void k_hs_carries(u32* __restrict__ agg, u32 tiles, unsigned long long* total_a, unsigned long long* total_b) {
  const int lane = threadIdx.x;
  u32 ca = 0, cb = 0;
  for (u32 base = 0; base < tiles; base += 64) {
    const u32 t = base + lane;
    const u32 ma = t < tiles ? agg[t] : 0, mb = t < tiles ? agg[tiles + t] : 0;
    u32 ia = ma, ib = mb;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 oa = __shfl_up(ia, off), ob = __shfl_up(ib, off);
      if (lane >= off) {
        ia = hs_sat(ia + oa);
        ib += ob;
      }
    }
    u32 xa = __shfl_up(ia, 1), xb = __shfl_up(ib, 1);
    if (lane == 0) xa = xb = 0;
    if (t < tiles) {
      agg[t] = hs_sat(ca + xa);
      agg[tiles + t] = cb + xb;
    }
    ca = hs_sat(ca + __shfl(ia, 63));
    cb += __shfl(ib, 63);
  }
  if (lane == 0) {
    *total_a = ca;
    *total_b = cb;
  }
}

__global__ __launch_bounds__(HS_BT) void k_hs_offsets(HsRun r) {
  __shared__ u32 s_wave[HS_WAVES][2];
  __shared__ u32 s_hist[HS_BUCKETS];
  u32 a[HS_PER_LANE], b[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
  if (threadIdx.x < HS_BUCKETS) s_hist[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    a[j] = b[j] = 0;
    if (i < r.n_ops) {
      const mh_hash_op o = r.ops[i];
      const HsPlan p = hs_plan_op(o, r.n_felts);
      a[j] = p.perms;
      b[j] = p.mru;
      atomicAdd(&s_hist[hs_bucket(o)], 1u + p.mru);  // an update is two chains of one length
    }
  }
  hs_tile_scan(a, b, r.agg[blockIdx.x], r.agg[r.tiles + blockIdx.x], ea, eb, ta, tb, s_wave);
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    if (i >= r.n_ops) continue;
    r.first_perm[i] = ea[j];
    r.mru[i] = eb[j] + b[j];
    const u32 chain = i + eb[j];  // eb[j] <= i: < 2 * n_ops
    r.chain_op[chain] = i << 1;
    if (b[j]) r.chain_op[chain + 1] = (i << 1) | 1;
    if (2 * ((u64)ea[j] + a[j]) > r.cap_rows) atomicMin(&r.w->nofit, (unsigned long long)i);
  }
  __syncthreads();  // the tile scan's barrier lies between the LDS atomics and here, this one after the last of them for every wave
  if (threadIdx.x < HS_BUCKETS && s_hist[threadIdx.x]) atomicAdd(&r.hist[threadIdx.x], s_hist[threadIdx.x]);
}

// a launch of its own: hist is complete.  sorted[] := chain_op[] by bucket
__global__ __launch_bounds__(HS_BT) void k_hs_order(HsRun r, u32 n_chains, u32* __restrict__ sorted) {
  __shared__ u32 s_cnt[HS_BUCKETS], s_base[HS_BUCKETS];
  if (threadIdx.x < HS_BUCKETS) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const u32 chain = blockIdx.x * HS_BT + threadIdx.x;
  u32 code = 0, bucket = 0, local = 0;
  bool valid = chain < n_chains;
  if (valid) {
    code = r.chain_op[chain];
    valid = (code >> 1) < r.n_ops;  // always
  }
  if (valid) {
    bucket = hs_bucket(r.ops[code >> 1]);
    local = atomicAdd(&s_cnt[bucket], 1u);
  }
  __syncthreads();
  if (threadIdx.x < HS_BUCKETS) {
    u32 start = 0;
    for (u32 t = 0; t < threadIdx.x; t++) start += r.hist[t];
    s_base[threadIdx.x] = s_cnt[threadIdx.x] ? start + atomicAdd(&r.hist[HS_BUCKETS + threadIdx.x], s_cnt[threadIdx.x]) : 0;
  }
  __syncthreads();
  if (valid) {
    const u32 to = s_base[bucket] + local;
    if (to < n_chains) sorted[to] = code;  // always: the buckets' counts are the histogram's
  }
}

// ---- chains ----
namespace {
struct HsChains {
  const mh_hash_op* ops;
  u32 n_ops;
  const u64* felts;
  const u32* first_perm;
  const u32* chain_op;
  u32 n_chains;
  u32 n_perms;
  u64* states;     // [n_perms][2][12]: pre-state, post-state
  u32* perm_op;    // [n_perms]
  mh_hash_result* results;  // [n_ops] or null
};
}  // namespace

__global__ __launch_bounds__(HS_CHAIN_BT) void k_hs_chains(HsChains c) {
  const u32 chain = blockIdx.x * HS_CHAIN_BT + threadIdx.x;
  if (chain >= c.n_chains) return;
  const u32 code = c.chain_op[chain], op = code >> 1, leg = code & 1;
  if (op >= c.n_ops) return;  // never: no index read from memory goes unchecked
  const mh_hash_op o = c.ops[op];
  const u64* f = c.felts + o.payload;  // the plan has checked the operand range
  const bool merkle = o.kind >= 3;
  const u32 n = o.kind < 2 ? 1 : o.count;  // permutations of this chain
  const u32 perm0 = c.first_perm[op] + (leg ? o.count : 0);
  const u64* sib = f + (o.kind == 4 ? 8 : 4);
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = 0;
  if (merkle) {
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = gl_canon(f[4 * leg + i]);
  } else if (o.kind == 0) {
#pragma unroll
    for (int i = 8; i < 12; i++) s[i] = gl_canon(f[i]);
  } else if (o.kind == 1) {
    s[9] = gl_canon(o.index);
  }
#pragma unroll 1
  for (u32 t = 0; t < n; t++) {
    if (merkle) {
      const bool right = (o.index >> t) & 1;  // t < count <= 64
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u64 x = gl_canon(sib[4 * (size_t)t + i]), root = s[i];
        s[i] = right ? x : root;
        s[4 + i] = right ? root : x;
      }
#pragma unroll
      for (int i = 8; i < 12; i++) s[i] = 0;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) s[i] = gl_canon(f[8 * (size_t)t + i]);
    }
    const u32 perm = perm0 + t;
    if (perm >= c.n_perms) return;  // never: the offsets are the scan of these counts
    u64* at = c.states + (size_t)perm * 24;
#pragma unroll
    for (int i = 0; i < 12; i += 2) *reinterpret_cast<ulonglong2*>(at + i) = make_ulonglong2(s[i], s[i + 1]);
    c.perm_op[perm] = op;
    p2_permute(s);
#pragma unroll
    for (int i = 0; i < 12; i += 2) *reinterpret_cast<ulonglong2*>(at + 12 + i) = make_ulonglong2(s[i], s[i + 1]);
  }
  if (c.results) {
    mh_hash_result* res = c.results + op;
    if (o.kind == 4 && leg == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++) res->old_root[i] = s[i];
    } else {
      res->addr = 2 * (u64)c.first_perm[op] + 1;
#pragma unroll
      for (int i = 0; i < 12; i++) res->state[i] = s[i];
      if (o.kind != 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) res->old_root[i] = 0;
      }
    }
  }
}

// ---- ids ----
namespace {
struct HsIds {
  const u64* states;
  u32 n_perms;
  u32 tiles;       // of HS_TILE permutations
  u32* table;      // [mask + 1]: the permutation that won the slot
  u32* least;      // [mask + 1]: the lowest permutation with the slot's state
  u32 mask;
  u32* slot_of;    // [n_perms]
  u32* agg;        // [2][tiles]
  u32* rank;       // [n_perms]
};

__device__ __forceinline__ u64 hs_mix(const u64* s) {
  u64 h = 0x9E3779B97F4A7C15ULL;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    h ^= s[i];
    h *= 0xD6E8FEB86659FD93ULL;
    h ^= h >> 32;
  }
  return h;
}
}  // namespace

__global__ __launch_bounds__(HS_BT) void k_hs_insert(HsIds a) {
  const u32 p = blockIdx.x * HS_BT + threadIdx.x;
  if (p >= a.n_perms) return;
  u64 s[12];
  const u64* mine = a.states + (size_t)p * 24;
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = mine[i];
  u32 slot = (u32)hs_mix(s) & a.mask;
  for (u32 tries = 0; tries <= a.mask; tries++, slot = (slot + 1) & a.mask) {  // the table has more slots than permutations
    u32 owner = __atomic_load_n(&a.table[slot], __ATOMIC_RELAXED);
    if (owner == HS_EMPTY) {
      owner = atomicCAS(&a.table[slot], HS_EMPTY, p);
      if (owner == HS_EMPTY) owner = p;
    }
    bool same = owner == p;
    if (!same && owner < a.n_perms) {
      const u64* other = a.states + (size_t)owner * 24;  // written by the launch before this one
      same = true;
#pragma unroll
      for (int i = 0; i < 12; i++) same = same && other[i] == s[i];
    }
    if (same) {
      a.slot_of[p] = slot;
      if (__atomic_load_n(&a.least[slot], __ATOMIC_RELAXED) > p) atomicMin(&a.least[slot], p);  // least only falls
      return;
    }
  }
}

__device__ __forceinline__ u32 hs_is_rep(const HsIds& a, u32 p) {
  const u32 slot = a.slot_of[p];
  return slot <= a.mask && a.least[slot] == p;
}

__global__ __launch_bounds__(HS_BT) void k_hs_flags(HsIds a) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 f[HS_PER_LANE], z[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 p = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    f[j] = p < a.n_perms ? hs_is_rep(a, p) : 0;
    z[j] = 0;
  }
  hs_tile_scan(f, z, 0, 0, ea, eb, ta, tb, s_wave);
  if (threadIdx.x == 0) {
    a.agg[blockIdx.x] = ta;
    a.agg[a.tiles + blockIdx.x] = 0;
  }
}

__global__ __launch_bounds__(HS_BT) void k_hs_ranks(HsIds a) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 f[HS_PER_LANE], z[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 p = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    f[j] = p < a.n_perms ? hs_is_rep(a, p) : 0;
    z[j] = 0;
  }
  hs_tile_scan(f, z, a.agg[blockIdx.x], 0, ea, eb, ta, tb, s_wave);
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 p = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    if (p < a.n_perms) a.rank[p] = ea[j];
  }
}

// ---- rows ----
namespace {
struct HsOut {
  u64* base;     // column 0, row 0 of the matrix written into
  u64 height;    // its rows
  u32 col0;      // first of the 20 columns
  int selector;  // also column 0 := 0 (the chiplets trace's hasher selector)
};

struct HsRows {
  const mh_hash_op* ops;
  u32 n_ops;
  const u32* first_perm;
  const u32* mru;
  const u32* perm_op;
  const u64* states;
  HsIds ids;
  u32 n_perms;
  u64 n_rows;    // multiple of 8, <= o.height
  u64 final_mru;
  HsOut o;
};
}  // namespace

__global__ __launch_bounds__(HS_BT) void k_hs_rows(HsRows a) {
  const u64 r = (u64)blockIdx.x * HS_BT + threadIdx.x;
  if (r >= a.n_rows) return;
  u64 row[HS_WIDTH];
#pragma unroll
  for (int i = 0; i < HS_WIDTH; i++) row[i] = 0;
  const u32 perm = (u32)(r >> 1);
  const bool out = r & 1;
  if (perm >= a.n_perms) {  // padding: selectors (0, 1, 0), the final mrupdate_id
    row[1] = 1;
    row[16] = a.final_mru;
  } else {
    u32 op = a.perm_op[perm];
    if (op >= a.n_ops) op = a.n_ops - 1;  // never
    const mh_hash_op o = a.ops[op];
    const u32 pos = perm - a.first_perm[op];
    const bool merkle = o.kind >= 3;
    const u32 leg = merkle && pos >= o.count;
    const u32 level = pos - (leg ? o.count : 0);
    const u32 last = (o.kind == 2 || merkle) ? o.count - 1 : 0;  // of the chain
    const u32 at = o.kind == 2 ? pos : level;
    const u32 shift = level + out;  // <= 64
    const u64 node = !merkle || shift >= 64 ? 0 : o.index >> shift;
    if (!out) {
      row[0] = 1;
      row[1] = o.kind == 4;
      row[2] = o.kind == 3 || (o.kind == 4 && leg);
      row[17] = at == 0;
      row[18] = node & 1;
    } else {
      row[2] = o.kind == 0 || at != last;  // RETURN_STATE; RETURN_HASH is (0, 0, 0)
      row[17] = at == last;
      row[18] = at == last ? 0 : node & 1;
    }
    row[15] = node;
    row[16] = a.mru[op];
    const u64* s = a.states + (size_t)r * 12;  // [perm][out][12]
#pragma unroll
    for (int i = 0; i < 12; i += 2) {
      const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(s + i);
      row[3 + i] = v.x;
      row[4 + i] = v.y;
    }
    const u32 slot = a.ids.slot_of[perm];
    u32 rep = slot <= a.ids.mask ? a.ids.least[slot] : perm;
    if (rep >= a.n_perms) rep = perm;  // never
    row[19] = a.ids.rank[rep];
  }
  u64* cell = a.o.base + (size_t)a.o.col0 * a.o.height + r;
#pragma unroll
  for (int i = 0; i < HS_WIDTH; i++) cell[(size_t)i * a.o.height] = row[i];
  if (a.o.selector) a.o.base[r] = 0;
}

// ---- host ----
namespace {
unsigned hs_grid(u64 n, u64 per_block) { return (unsigned)((n + per_block - 1) / per_block); }

void hs_fill_info(mh_hasher_section_info* info, u64 rows, u64 perms, u64 requests, u64 mru, int log_n, int defect, u64 index) {
  if (!info) return;
  info->n_rows = rows;
  info->n_permutations = perms;
  info->n_requests = requests;
  info->mrupdate_id = mru;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_index = index;
}

[[noreturn]] void hs_refuse(mh_hasher_section_info* info, u64 perms, u64 mru, int log_n, int defect, u64 index, const mh_hash_op* ops, size_t n_ops,
                            const char* entry) {
  hs_fill_info(info, 0, perms, 0, mru, log_n, defect, index);
  char buf[256];
  const unsigned long long i = index;
  const mh_hash_op o = index < n_ops ? ops[index] : mh_hash_op{0, 0, 0, 0};
  switch (defect) {
    case 1: snprintf(buf, sizeof buf, "%s: defect 1, op %llu has kind %u (0 permute .. 4 merkle update)", entry, i, o.kind); break;
    case 2:
      snprintf(buf, sizeof buf, "%s: defect 2, op %llu (kind %u) has count %u: %s", entry, i, o.kind, o.count,
               o.kind == 2 ? "a basic block has at least one batch" : "the path is empty or deeper than 64");
      break;
    case 3:
      snprintf(buf, sizeof buf, "%s: defect 3, op %llu: invalid index %llu for a path of depth %u", entry, i, (unsigned long long)o.index, o.count);
      break;
    case 4:
      snprintf(buf, sizeof buf, "%s: defect 4, the operands of op %llu (kind %u, count %u, payload %llu) do not lie inside the felts", entry, i,
               o.kind, o.count, (unsigned long long)o.payload);
      break;
    default: snprintf(buf, sizeof buf, "%s: defect 5, the section does not fit: op %llu is the first without its rows", entry, i);
  }
  throw MhError(MH_ERR_INVALID, buf);
}

struct HsTarget {
  virtual ~HsTarget() {}
  virtual u64 cap_rows() const = 0;                 // rows the target has; ~0 when it is sized by the section
  virtual HsOut resolve(u64 n_rows, int* log_n) = 0;  // called once the section is known to fit
};

// The section of `ops`.  n_ops >= 1.  Returns after the second read-back with the rows kernel enqueued, or after the copy of the
// results when the caller wants them
void hs_run(mh_ctx* c, const mh_hash_op* ops, size_t n_ops, const uint64_t* felts, size_t n_felts, HsTarget& target, int shown_log_n,
            mh_hash_result* results, mh_hasher_section_info* info, const char* entry) {
  const u32 tiles = hs_grid(n_ops, HS_TILE);
  DevBuf dops(n_ops * sizeof(mh_hash_op)), dfelts((n_felts ? n_felts : 1) * 8), words(sizeof(HsWords));
  DevBuf agg((size_t)tiles * 8), first_perm(n_ops * 4), mru(n_ops * 4), chain_op(n_ops * 8), hist(2 * HS_BUCKETS * 4);
  HsWords* dw = (HsWords*)words.p;
  const HsWords init{HS_NONE, HS_NONE, 0, 0, 0, 0};
  c->h2d(words.p, &init, sizeof init);
  c->h2d(dops.p, ops, n_ops * sizeof(mh_hash_op));
  if (n_felts) c->h2d(dfelts.p, felts, n_felts * 8);
  HsRun r{(const mh_hash_op*)dops.p, (u32)n_ops, dfelts.u(), n_felts, target.cap_rows(), (u32*)agg.p, tiles, (u32*)first_perm.p, (u32*)mru.p,
          (u32*)chain_op.p, (u32*)hist.p, dw};
  {
    ProfScope ps(c, "hs_plan", 24.0 * (double)n_ops);
    HIP_CHECK(hipMemsetAsync(hist.p, 0, 2 * HS_BUCKETS * 4, c->stream));
    MH_LAUNCH(k_hs_plan, dim3(tiles), dim3(HS_BT), 0, c->stream, r);
  }
  {
    ProfScope ps(c, "hs_carries", 16.0 * (double)tiles);
    MH_LAUNCH(k_hs_carries, dim3(1), dim3(64), 0, c->stream, (u32*)agg.p, tiles, &dw->n_perms, &dw->n_updates);
  }
  {
    ProfScope ps(c, "hs_offsets", 40.0 * (double)n_ops);
    MH_LAUNCH(k_hs_offsets, dim3(tiles), dim3(HS_BT), 0, c->stream, r);
  }
  HsWords w;
  c->d2h(&w, words.p, sizeof w);  // the first wait: the defects and the sizes, before anything but scratch is written
  hs_fill_info(info, 0, w.n_perms, 0, w.n_updates, shown_log_n, 0, 0);
  MH_REQUIRE(w.n_perms <= HS_MAX_PERMS, std::string(entry) + ": more than 2^24 permutations");
  const u32 n_perms = (u32)w.n_perms;
  const u64 n_rows = (2 * (u64)n_perms + 7) & ~(u64)7;
  if (shown_log_n < 0)  // what the section would get
    for (shown_log_n = 6; ((u64)1 << shown_log_n) < n_rows; shown_log_n++) {}
  if (w.bad != HS_NONE) hs_refuse(info, n_perms, w.n_updates, shown_log_n, (int)(w.bad & 7), w.bad >> 3, ops, n_ops, entry);
  if (w.nofit != HS_NONE || n_rows > target.cap_rows())
    hs_refuse(info, n_perms, w.n_updates, shown_log_n, 5, w.nofit != HS_NONE ? w.nofit : n_ops, ops, n_ops, entry);
  int log_n = shown_log_n;
  const HsOut out = target.resolve(n_rows, &log_n);

  const u32 n_chains = (u32)(n_ops + w.n_updates), ptiles = hs_grid(n_perms, HS_TILE);
  u32 slots = 64;
  while (slots < 2 * n_perms) slots <<= 1;  // <= 2^25
  DevBuf states((size_t)n_perms * 192), perm_op((size_t)n_perms * 4), dres(results ? n_ops * sizeof(mh_hash_result) : 0);
  DevBuf table((size_t)slots * 8), slot_of((size_t)n_perms * 4), pagg((size_t)ptiles * 8), rank((size_t)n_perms * 4), sorted((size_t)n_chains * 4);
  {
    ProfScope ps(c, "hs_order", 12.0 * (double)n_chains);
    HIP_CHECK(hipMemsetAsync(sorted.p, 0xFF, (size_t)n_chains * 4, c->stream));  // a place nobody took is no op (never)
    MH_LAUNCH(k_hs_order, dim3(hs_grid(n_chains, HS_BT)), dim3(HS_BT), 0, c->stream, r, n_chains, (u32*)sorted.p);
  }
  HsChains ch{r.ops, r.n_ops, r.felts, r.first_perm, (const u32*)sorted.p, n_chains, n_perms, states.u(), (u32*)perm_op.p, (mh_hash_result*)dres.p};
  {
    ProfScope ps(c, "hs_chains", 196.0 * (double)n_perms);
    MH_LAUNCH(k_hs_chains, dim3(hs_grid(n_chains, HS_CHAIN_BT)), dim3(HS_CHAIN_BT), 0, c->stream, ch);
  }
  HsIds ids{states.u(), n_perms, ptiles, (u32*)table.p, (u32*)table.p + slots, slots - 1, (u32*)slot_of.p, (u32*)pagg.p, (u32*)rank.p};
  {
    ProfScope ps(c, "hs_insert", 100.0 * (double)n_perms + 8.0 * (double)slots);
    HIP_CHECK(hipMemsetAsync(table.p, 0xFF, (size_t)slots * 8, c->stream));
    HIP_CHECK(hipMemsetAsync(slot_of.p, 0xFF, (size_t)n_perms * 4, c->stream));
    MH_LAUNCH(k_hs_insert, dim3(hs_grid(n_perms, HS_BT)), dim3(HS_BT), 0, c->stream, ids);
  }
  {
    ProfScope ps(c, "hs_ranks", 20.0 * (double)n_perms);
    MH_LAUNCH(k_hs_flags, dim3(ptiles), dim3(HS_BT), 0, c->stream, ids);
    MH_LAUNCH(k_hs_carries, dim3(1), dim3(64), 0, c->stream, (u32*)pagg.p, ptiles, &dw->n_requests, &dw->unused);
    MH_LAUNCH(k_hs_ranks, dim3(ptiles), dim3(HS_BT), 0, c->stream, ids);
  }
  HsWords w2;
  c->d2h(&w2, words.p, sizeof w2);  // the second wait: n_requests
  HsRows rows{r.ops, r.n_ops, r.first_perm, r.mru, (const u32*)perm_op.p, states.u(), ids, n_perms, n_rows, w.n_updates, out};
  {
    ProfScope ps(c, "hs_rows", (96.0 + 8.0 * HS_WIDTH) * (double)n_rows);
    MH_LAUNCH(k_hs_rows, dim3(hs_grid(n_rows, HS_BT)), dim3(HS_BT), 0, c->stream, rows);
  }
  if (results) c->d2h(results, dres.p, n_ops * sizeof(mh_hash_result));
  hs_fill_info(info, n_rows, n_perms, w2.n_requests, w.n_updates, log_n, 0, 0);
}

struct HsBuildTarget : HsTarget {
  mh_ctx* c;
  int log_n;  // -1: sized by the section
  std::unique_ptr<mh_trace> t;
  HsBuildTarget(mh_ctx* ctx, int l) : c(ctx), log_n(l) {}
  u64 cap_rows() const override { return log_n < 0 ? ~(u64)0 : (u64)1 << log_n; }
  HsOut resolve(u64 n_rows, int* out_log_n) override {
    int l = log_n;
    if (l < 0)
      for (l = 6; ((u64)1 << l) < n_rows; l++) {}  // n_rows <= 2^25
    const u64 height = (u64)1 << l;
    t = trace_new(c, l, HS_WIDTH);
    if (n_rows < height)  // rows [n_rows, height) of every column
      HIP_CHECK(hipMemset2DAsync(t->cols.u() + n_rows, height * 8, 0, (height - n_rows) * 8, HS_WIDTH, c->stream));
    *out_log_n = l;
    return HsOut{t->cols.u(), height, 0, 0};
  }
};

struct HsChipletsTarget : HsTarget {
  mh_trace* chiplets;
  explicit HsChipletsTarget(mh_trace* t) : chiplets(t) {}
  u64 cap_rows() const override { return (u64)1 << chiplets->log_n; }
  HsOut resolve(u64, int* out_log_n) override {
    *out_log_n = chiplets->log_n;
    return HsOut{chiplets->cols.u(), (u64)1 << chiplets->log_n, 1, 1};
  }
};
}  // namespace

#define HS_CATCH                    \
  catch (const MhError& e) {        \
    c->err = e.what();              \
    return e.code;                  \
  }                                 \
  catch (const std::exception& e) { \
    c->err = e.what();              \
    return MH_ERR_INTERNAL;         \
  }

extern "C" uint32_t mh_hasher_section_tile(void) { return HS_TILE; }

extern "C" int mh_hasher_section_build(mh_ctx* c, const mh_hash_op* ops, size_t n_ops, const uint64_t* felts, size_t n_felts, int log_n,
                                       mh_trace** out, mh_hash_result* results, mh_hasher_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_hasher_section_build";
    if (out) *out = nullptr;
    hs_fill_info(info, 0, 0, 0, 0, log_n, 0, 0);
    MH_REQUIRE(out && (ops || !n_ops) && (felts || !n_felts), "mh_hasher_section_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_hasher_section_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(n_ops <= HS_MAX_PERMS, "mh_hasher_section_build: more than 2^24 permutations");
    HIP_CHECK(hipSetDevice(c->device));
    HsBuildTarget target(c, log_n);
    if (n_ops) {
      hs_run(c, ops, n_ops, felts, n_felts, target, log_n, results, info, entry);
    } else {
      int l = log_n;
      target.resolve(0, &l);
      hs_fill_info(info, 0, 0, 0, 0, l, 0, 0);
    }
    *out = target.t.release();
    return MH_OK;
  }
  HS_CATCH
}

extern "C" int mh_miden_hasher_section(mh_ctx* c, mh_trace* chiplets, const mh_hash_op* ops, size_t n_ops, const uint64_t* felts, size_t n_felts,
                                       mh_hash_result* results, mh_hasher_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_miden_hasher_section";
    hs_fill_info(info, 0, 0, 0, 0, 0, 0, 0);
    MH_REQUIRE(chiplets && (ops || !n_ops) && (felts || !n_felts), "mh_miden_hasher_section: null argument");
    MH_REQUIRE(chiplets->ctx == c, "mh_miden_hasher_section: the chiplets trace belongs to another context");
    MH_REQUIRE(chiplets->width == HS_CHIPLETS_WIDTH, "mh_miden_hasher_section: the chiplets trace is 22 columns wide");
    MH_REQUIRE(chiplets->log_n >= 3 && chiplets->log_n <= 32, "mh_miden_hasher_section: bad chiplets height");
    MH_REQUIRE(n_ops <= HS_MAX_PERMS, "mh_miden_hasher_section: more than 2^24 permutations");
    hs_fill_info(info, 0, 0, 0, 0, chiplets->log_n, 0, 0);
    if (!n_ops) return MH_OK;
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    HsChipletsTarget target(chiplets);
    hs_run(c, ops, n_ops, felts, n_felts, target, chiplets->log_n, results, info, entry);
    return MH_OK;
  }
  HS_CATCH
}
