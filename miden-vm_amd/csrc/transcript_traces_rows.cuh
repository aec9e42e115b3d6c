// The per-lane bodies of the ChunkNode and TranscriptEval traces' device stage (transcript_traces.hip): the checking and counting passes
// and the two row writers, as host-device functions (as ec_traces_rows.cuh's are).  The kernels of transcript_traces.hip are their only
// callers in the library; tools/transcript_traces_cpu.cpp runs the same bodies lane by lane on the host for
// tests/test_transcript_traces_cpu.py.
//
// Column orders: ChunkAir hash/chunk/mod.rs:55-83, KeccakNodeAir hash/keccak/node/mod.rs:122-153 (behind the chunk side's 12 columns,
// hash/chunk_node/mod.rs), TranscriptEvalAir transcript/eval/mod.rs:110-306; the rule hash/chunk/trace.rs:133-175,
// hash/keccak/node/trace.rs:52-113, hash/chunk_node/trace.rs:24-45, transcript/eval/trace.rs:895-1155.
#pragma once
#include "../../include/midenhip.h"
#include "gl.cuh"
#include "ledger_stage.cuh"
#include "wave_count.cuh"

namespace {
constexpr int CN_WIDTH = 42, CN_CHUNK_WIDTH = 12, TE_WIDTH = 39, P2_WIDTH = 32, P2_PERIOD = 16;
constexpr int P2_COL_IS_ABSORB = 3, P2_COL_STATE = 4;

// the device-resident Poseidon2 chiplet trace, column-major: what mh_poseidon2_chiplet_trace_build returned
struct P2View {
  const u64* cols;
  u64 n;       // rows
  u64 cycles;  // n / 16
};

GL_HD u64 p2_is_absorb(const P2View& p, u64 c) { return p.cols[(size_t)P2_COL_IS_ABSORB * p.n + P2_PERIOD * c]; }
// lane j of the digest on cycle c: the permutation's output, row 15 of the cycle
GL_HD u64 p2_digest(const P2View& p, u64 c, int j) { return p.cols[(size_t)(P2_COL_STATE + j) * p.n + P2_PERIOD * c + (P2_PERIOD - 1)]; }
// cycle c < cycles is the last of an absorption: the next cycle starts one (or there is none), and c is not padding (all zero)
GL_HD bool p2_ends(const P2View& p, u64 c) {
  if (c + 1 < p.cycles && p2_is_absorb(p, c + 1) != 0) return false;
  return (p2_digest(p, c, 0) | p2_digest(p, c, 1) | p2_digest(p, c, 2) | p2_digest(p, c, 3)) != 0;
}

// These two builders have no sections: section 0, and an index held in 64 bits cut to its low 32.  (The bodies call this and not
// ledger_report itself: with the cut at each call te_row_check's instruction stream changed, through here it is the one it was.)
GL_HD void tt_report(unsigned long long* defect, int kind, u64 index, int operand) { ledger_report(defect, kind, 0, (u32)index, operand); }

// ================================================ ChunkNode ================================================
struct CnLists {
  const uint8_t* bytes;
  const uint8_t* digests;       // [n][32]
  const mh_kn_record* records;
  u32 n;
  u32 total_chunks;             // the chunk side's active rows
  u64 next_perm;                // where the dead rows' perm counter starts
  P2View p2;
  unsigned long long* defect;
};

GL_HD u64 cn_n_chunks(u64 len) { return len ? (len + 31) / 32 : 1; }

// the record whose chain holds chunk row t < total_chunks: the last i with chunk_head[i] <= t (the heads are the running sum)
GL_HD u32 cn_record_of(const CnLists& L, u32 t) {
  u32 lo = 0, hi = L.n;
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (L.records[mid].chunk_head <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// a lane per chunk row: its cycle continues the chain's absorption, or starts it
GL_HD void cn_chunk_check(const CnLists& L, u32 t) {
  const u32 i = cn_record_of(L, t);
  const u64 c = t - L.records[i].chunk_head;
  const u64 a = p2_is_absorb(L.p2, L.records[i].perm_chunks + c);
  if (c == 0 ? a != 0 : a != 1) tt_report(L.defect, 8, i, c == 0 ? 0 : 1);
}

// a lane per record: the three digests it reads end an absorption
GL_HD void cn_record_check(const CnLists& L, u32 i) {
  const mh_kn_record r = L.records[i];
  const u64 cyc[3] = {r.perm_chunks + cn_n_chunks(r.len) - 1, r.perm_digest_chunks, r.perm_keccak};
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (!p2_ends(L.p2, cyc[k])) {
      tt_report(L.defect, 9, i, k);
      return;
    }
}

GL_HD u64 tt_le32(const uint8_t* b, u64 at, u64 end) {  // the little-endian u32 at `at`, bytes at and past `end` read as 0
  u64 v = 0;
  for (int k = 0; k < 4; k++)
    if (at + k < end) v |= (u64)b[at + k] << (8 * k);
  return v;
}

// row t of the 42-column trace: the chunk side, then the node side
GL_HD void cn_row(const CnLists& L, u64 n, u64* out, u64 t) {
  u64 row[CN_WIDTH];
  for (int k = 0; k < CN_WIDTH; k++) row[k] = 0;
  row[0] = t;
  if (t < L.total_chunks) {
    const u32 i = cn_record_of(L, (u32)t);
    const mh_kn_record r = L.records[i];
    const u64 c = t - r.chunk_head;
    row[1] = r.perm_chunks + c;
    row[2] = 1;
    row[3] = c == 0;
    for (int k = 0; k < 8; k++) row[4 + k] = tt_le32(L.bytes, r.offset + 32 * c + 4 * k, r.offset + r.len);
  } else {
    row[1] = L.next_perm + (t - L.total_chunks);
  }
  if (t < L.n) {
    const mh_kn_record r = L.records[t];
    const u64 n_chunks = cn_n_chunks(r.len);
    u64* nd = row + CN_CHUNK_WIDTH;
    nd[0] = 1;
    nd[1] = r.sponge_head;
    nd[2] = r.len / 136 + 1;
    nd[3] = r.chunk_head;
    nd[4] = n_chunks;
    nd[5] = r.perm_chunks;
    nd[6] = r.len;
    nd[7] = r.perm_digest_chunks;
    nd[8] = r.perm_keccak;
    for (int k = 0; k < 8; k++) nd[9 + k] = tt_le32(L.digests, 32 * t + 4 * k, 32 * t + 32);
    for (int j = 0; j < 4; j++) {
      nd[17 + j] = p2_digest(L.p2, r.perm_chunks + n_chunks - 1, j);
      nd[21 + j] = p2_digest(L.p2, r.perm_digest_chunks, j);
      nd[25 + j] = p2_digest(L.p2, r.perm_keccak, j);
    }
    nd[29] = r.out_mult;
  }
  for (int k = 0; k < CN_WIDTH; k++) out[(size_t)k * n + t] = gl_canon(row[k]);  // the records' words are any uint64_t
}

// ================================================ TranscriptEval ================================================
enum : u32 { TE_ZERO = 0, TE_AND, TE_UINT_LEAF, TE_UINT_PIN, TE_UINT_OP, TE_EC_CREATE, TE_EC_PAI, TE_EC_OP, TE_EC_MSM, TE_N_KINDS };
enum : int { TE_CLASS_TRUTHY = 0, TE_CLASS_UINT = 1, TE_CLASS_EC = 2 };
// TranscriptEvalAir's columns (transcript/eval/mod.rs:110-306)
enum : int {
  TEC_ACT = 0, TEC_PERM, TEC_LHS = 2, TEC_RHS = 6, TEC_H = 10, TEC_IS_ZERO = 14, TEC_OUT_MULT, TEC_IS_AND, TEC_IS_UINT_LEAF, TEC_IS_UINT_OP,
  TEC_IS_EC_CREATE, TEC_IS_EC_PAI, TEC_IS_EC_OP, TEC_IS_ADD, TEC_IS_SUB, TEC_IS_MUL, TEC_IS_IS, TEC_IS_PINNED, TEC_PTR, TEC_BOUND_PTR,
  TEC_TAG_ARG1, TEC_A_PTR, TEC_B_PTR, TEC_TAG_ARG0, TEC_EC_GROUP_PTR, TEC_IS_EC_MSM, TEC_IS_MSM_LAST, TEC_MSM_IDX, TEC_MSM_EXPR,
  TEC_MSM_IS_HEAD
};
static_assert(TEC_MSM_IS_HEAD == TE_WIDTH - 1, "39 columns");

struct TeLists {
  const mh_te_node* nodes;
  const mh_te_term* terms;
  const uint32_t* limbs;   // [n_lit][8]
  const u32* row_start;    // [n_nodes]: the planner's; rows 1 .. n_body - 1 hold the nodes other than the root and the ZEROs, in list order
  u32 n_nodes, n_terms, root;
  u32 n_body;              // the root's row and the other nodes' rows
  u64 n_zero;              // ZERO nodes other than the root: the merged row's out_mult
  u32* count;              // [n_nodes]: the reads of a node
  P2View p2;
  unsigned long long* defect;
};

GL_HD int te_class(const mh_te_node& x) {
  switch (x.kind) {
    case TE_UINT_LEAF: return TE_CLASS_UINT;
    case TE_UINT_OP: return x.op == 4 ? TE_CLASS_TRUTHY : TE_CLASS_UINT;
    case TE_EC_CREATE: case TE_EC_PAI: case TE_EC_MSM: return TE_CLASS_EC;
    case TE_EC_OP: return x.op == 3 ? TE_CLASS_TRUTHY : TE_CLASS_EC;
    default: return TE_CLASS_TRUTHY;  // ZERO, AND, UINT_PIN
  }
}

// the cycle whose digest is the node's hash (an MSM's: its last); ZERO has none
GL_HD u64 te_hash_cycle(const mh_te_node& x) { return x.kind == TE_EC_MSM ? x.perm + (u64)x.rhs - 1 : x.perm; }

GL_HD u64 te_src_hash(const TeLists& L, int64_t src, int j) {
  if (src < 0) return p2_digest(L.p2, (u64)(-1 - src), j);
  const mh_te_node x = L.nodes[src];
  return x.kind == TE_ZERO ? 0 : p2_digest(L.p2, te_hash_cycle(x), j);
}

// the node of trace row 1 <= r < n_body (row 0 is the root's) and the row's place in it: the last i with row_start[i] <= r.  The root
// and the ZEROs take no row here: they share their start with the node behind them, which the search prefers.
GL_HD u32 te_node_of(const TeLists& L, u32 r, u32* idx) {
  if (r == 0) {
    *idx = 0;
    return L.root;
  }
  u32 lo = 0, hi = L.n_nodes;
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (L.row_start[mid] <= r) lo = mid; else hi = mid;
  }
  *idx = r - L.row_start[lo];
  return lo;
}

// one binary operand of node i: its class, and its read.  -> false after a report
GL_HD bool te_operand(const TeLists& L, u32 i, int64_t src, int want, int operand) {
  if (te_class(L.nodes[src]) != want) {
    tt_report(L.defect, 8, i, operand);
    return false;
  }
  wave_count(&L.count[src]);
  return true;
}

// a lane per body row: the node's operands (class, modulus, `is`), its cycles against the absorptions of p2, and its reads of its operands
GL_HD void te_row_check(const TeLists& L, u32 r) {
  u32 idx;
  const u32 i = te_node_of(L, r, &idx);
  const mh_te_node x = L.nodes[i];
  switch (x.kind) {
    case TE_ZERO: return;
    case TE_AND:
      for (int s = 0; s < 2; s++) {
        const int64_t src = s ? x.rhs : x.lhs;
        if (src >= 0) {
          if (!te_operand(L, i, src, TE_CLASS_TRUTHY, s)) return;
        } else if (!p2_ends(L.p2, (u64)(-1 - src))) {
          tt_report(L.defect, 15, i, s);
        }
      }
      break;
    case TE_UINT_OP: case TE_EC_CREATE: case TE_EC_OP: {
      const int want = x.kind == TE_EC_OP ? TE_CLASS_EC : TE_CLASS_UINT;
      if (!te_operand(L, i, x.lhs, want, 0) || !te_operand(L, i, x.rhs, want, 1)) return;
      const mh_te_node a = L.nodes[x.lhs], b = L.nodes[x.rhs];
      if (x.kind != TE_EC_OP && (a.bound_ptr != x.bound_ptr || b.bound_ptr != x.bound_ptr)) tt_report(L.defect, 9, i, a.bound_ptr != x.bound_ptr ? 0 : 1);
      if (x.kind != TE_EC_CREATE && x.op == (x.kind == TE_UINT_OP ? 4u : 3u) && a.ptr != b.ptr) tt_report(L.defect, 10, i, 0);
      break;
    }
    case TE_EC_MSM: {
      const u64 t = (u64)x.lhs + idx, n_terms = (u64)x.rhs;
      const mh_te_term term = L.terms[t];
      if (!te_operand(L, (u32)t, term.base_node, TE_CLASS_EC, 2) || !te_operand(L, (u32)t, term.scalar_node, TE_CLASS_UINT, 3)) return;
      if (L.nodes[term.scalar_node].bound_ptr != x.bound_ptr) tt_report(L.defect, 9, t, 3);
      const u64 a = p2_is_absorb(L.p2, x.perm + idx);
      if (idx == 0 ? a != 0 : a != 1) tt_report(L.defect, 14, idx == 0 ? i : t, idx == 0 ? 0 : 1);
      if (idx + 1 == n_terms && !p2_ends(L.p2, x.perm + idx)) tt_report(L.defect, 14, i, 2);
      return;
    }
    default: break;  // a leaf, a pin, a point at infinity: no operand
  }
  if (p2_is_absorb(L.p2, x.perm) != 0) tt_report(L.defect, 13, i, 0);
  else if (!p2_ends(L.p2, x.perm)) tt_report(L.defect, 13, i, 1);
}

// a lane per node, behind the counting: a truthy node is read once (the root never), a value node at least once
GL_HD void te_read_check(const TeLists& L, u32 i) {
  const u32 reads = L.count[i];
  if (te_class(L.nodes[i]) == TE_CLASS_TRUTHY) {
    if (i == L.root) {
      if (reads) tt_report(L.defect, 11, i, 2);
    } else if (reads != 1) {
      tt_report(L.defect, 11, i, reads ? 1 : 0);
    }
  } else if (!reads) {
    tt_report(L.defect, 12, i, 0);
  }
}

// row r of the 39-column trace
GL_HD void te_row(const TeLists& L, u64 n, u64* out, u64 r) {
  u64 row[TE_WIDTH];
  for (int k = 0; k < TE_WIDTH; k++) row[k] = 0;
  if (r < L.n_body) {
    u32 idx;
    const u32 i = te_node_of(L, (u32)r, &idx);
    const mh_te_node x = L.nodes[i];
    const int cls = te_class(x);
    const u64 out_mult = i == L.root ? 0 : cls == TE_CLASS_TRUTHY ? 1 : (u64)L.count[i];  // a count is below 2^32: canonical
    row[TEC_ACT] = 1;
    if (x.kind == TE_EC_MSM) {
      const u64 n_terms = (u64)x.rhs;
      const mh_te_term term = L.terms[(u64)x.lhs + idx];
      const mh_te_node base = L.nodes[term.base_node], scalar = L.nodes[term.scalar_node];
      row[TEC_PERM] = x.perm + idx;
      for (int j = 0; j < 4; j++) {
        row[TEC_LHS + j] = p2_digest(L.p2, te_hash_cycle(base), j);
        row[TEC_RHS + j] = p2_digest(L.p2, te_hash_cycle(scalar), j);
        row[TEC_H + j] = p2_digest(L.p2, x.perm + idx, j);
      }
      row[TEC_IS_EC_MSM] = 1;
      row[TEC_IS_MSM_LAST] = idx + 1 == n_terms;
      row[TEC_MSM_IS_HEAD] = idx == 0;
      row[TEC_A_PTR] = base.ptr;
      row[TEC_B_PTR] = scalar.ptr;
      row[TEC_MSM_IDX] = idx;
      row[TEC_MSM_EXPR] = x.expr;
      row[TEC_EC_GROUP_PTR] = x.group;
      row[TEC_BOUND_PTR] = x.bound_ptr;
      if (idx + 1 == n_terms) {
        row[TEC_PTR] = x.ptr;
        row[TEC_OUT_MULT] = out_mult;
      }
    } else {
      row[TEC_OUT_MULT] = out_mult;
      if (x.kind == TE_ZERO) {
        row[TEC_IS_ZERO] = 1;
      } else {
        row[TEC_PERM] = x.perm;
        for (int j = 0; j < 4; j++) row[TEC_H + j] = p2_digest(L.p2, x.perm, j);
        if (x.kind == TE_UINT_LEAF || x.kind == TE_UINT_PIN) {
          const bool pinned = x.kind == TE_UINT_PIN;
          for (int j = 0; j < 4; j++) {
            row[TEC_LHS + j] = L.limbs[8 * (u64)x.lhs + j];
            row[TEC_RHS + j] = L.limbs[8 * (u64)x.lhs + 4 + j];
          }
          row[TEC_IS_UINT_LEAF] = 1;
          row[TEC_IS_PINNED] = pinned;
          row[TEC_PTR] = x.ptr;
          row[TEC_BOUND_PTR] = x.bound_ptr;
          row[TEC_TAG_ARG0] = pinned ? x.bound_ptr : 0;
          row[TEC_TAG_ARG1] = pinned ? x.ptr : x.bound_ptr;
        } else if (x.kind == TE_EC_PAI) {
          row[TEC_IS_EC_PAI] = 1;
          row[TEC_PTR] = x.ptr;
          row[TEC_TAG_ARG1] = x.group;
        } else {
          for (int j = 0; j < 4; j++) {
            row[TEC_LHS + j] = te_src_hash(L, x.lhs, j);
            row[TEC_RHS + j] = te_src_hash(L, x.rhs, j);
          }
          if (x.kind == TE_AND) {
            row[TEC_IS_AND] = 1;
          } else {
            row[TEC_PTR] = x.ptr;
            row[TEC_A_PTR] = L.nodes[x.lhs].ptr;
            row[TEC_B_PTR] = L.nodes[x.rhs].ptr;
            if (x.kind == TE_UINT_OP) {
              row[TEC_IS_UINT_OP] = 1;
              row[TEC_IS_ADD] = x.op == 1;
              row[TEC_IS_SUB] = x.op == 2;
              row[TEC_IS_MUL] = x.op == 3;
              row[TEC_IS_IS] = x.op == 4;
              row[TEC_BOUND_PTR] = x.bound_ptr;
              row[TEC_TAG_ARG0] = x.op;
            } else if (x.kind == TE_EC_CREATE) {
              row[TEC_IS_EC_CREATE] = 1;
              row[TEC_BOUND_PTR] = x.bound_ptr;
              row[TEC_TAG_ARG1] = x.group;
            } else {
              row[TEC_IS_EC_OP] = 1;
              row[TEC_IS_ADD] = x.op == 1;
              row[TEC_IS_SUB] = x.op == 2;
              row[TEC_IS_IS] = x.op == 3;
              row[TEC_TAG_ARG0] = x.op;
              row[TEC_EC_GROUP_PTR] = x.group;
            }
          }
        }
      }
    }
  } else if (r == L.n_body && L.n_zero) {  // every ZERO leaf but the root, merged
    row[TEC_ACT] = 1;
    row[TEC_IS_ZERO] = 1;
    row[TEC_OUT_MULT] = L.n_zero;
  }
  for (int k = 0; k < TE_WIDTH; k++) out[(size_t)k * n + r] = gl_canon(row[k]);  // the records' words are any uint64_t
}
}  // namespace
