// The planners of the precompile prover's ChunkNode and TranscriptEval traces (mh_chunk_node_plan, mh_transcript_eval_plan): host only,
// no device pass.
//
// They validate what the records show by themselves plus prefix sums -- so that the device stage (transcript_traces.hip) never reads
// past a list, a literal, a message or the Poseidon2 trace -- and give the heights and, for the transcript, every node's first row.
// Defects are looked for kind by kind, the lowest kind first and within it the lowest index; a later kind is only looked for once the
// earlier ones are absent.  The kinds are the header's (include/midenhip.h): 1 a NULL pointer .. 7 a log_n below the height needed.
// Whether a cycle sits on an absorption's boundary, and everything that compares two nodes (kinds 8..), is the device pass's to judge.
#include "ledger_plan.hpp"

namespace {
// the height: kinds 6 and 7
template <class Info>
int tt_height(Info* info, uint64_t active, int log_n) {
  if (active > PLAN_MAX_ROWS) return plan_defect(info, 6, active);
  if (log_n > 24) return plan_defect(info, 6, (uint64_t)log_n);
  info->rows_needed = pow2_at_least(active, 2);
  if (!plan_height(log_n, info->rows_needed, &info->rows)) return plan_defect(info, 7, info->rows_needed);
  return MH_OK;
}

uint64_t kn_chunks(uint64_t len) { return len ? (len - 1) / 32 + 1 : 1; }
}  // namespace

extern "C" int mh_chunk_node_plan(const uint8_t* bytes, size_t n_bytes, const uint8_t* digests, const mh_kn_record* records, size_t n,
                                  uint64_t p2_cycles, int log_n, mh_chunk_node_info* info) {
  if (!info) return MH_ERR_INVALID;
  *info = mh_chunk_node_info{};
  info->n_records = n;
  info->p2_cycles = p2_cycles;
  if (!bytes && n_bytes) return plan_defect(info, 1, 0, 0);
  if (!digests && n) return plan_defect(info, 1, 0, 1);
  if (!records && n) return plan_defect(info, 1, 0, 2);
  for (size_t i = 0; i < n; i++)
    if (records[i].offset > n_bytes || records[i].len > n_bytes - records[i].offset) return plan_defect(info, 2, i);
  // a len is at most n_bytes from here on.  The running sum saturates far above what a trace holds (kind 6) and below a wrap.
  constexpr uint64_t SATURATED = (uint64_t)1 << 62;
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    if (records[i].chunk_head != at) return plan_defect(info, 3, i);
    at += kn_chunks(records[i].len);
    if (at > SATURATED) at = SATURATED;
  }
  info->n_chunks = at;
  for (size_t i = 0; i < n; i++)
    if (records[i].sponge_head % 32) return plan_defect(info, 4, i);
  for (size_t i = 0; i < n; i++) {
    const mh_kn_record& r = records[i];
    const uint64_t k = kn_chunks(r.len);
    if (r.perm_chunks >= p2_cycles || k > p2_cycles - r.perm_chunks) return plan_defect(info, 5, i, 0);
    if (r.perm_digest_chunks >= p2_cycles) return plan_defect(info, 5, i, 1);
    if (r.perm_keccak >= p2_cycles) return plan_defect(info, 5, i, 2);
  }
  return tt_height(info, at > n ? at : (uint64_t)n, log_n);
}

namespace {
enum : uint32_t { TE_ZERO = 0, TE_AND, TE_UINT_LEAF, TE_UINT_PIN, TE_UINT_OP, TE_EC_CREATE, TE_EC_PAI, TE_EC_OP, TE_EC_MSM, TE_N_KINDS };

bool te_truthy(const mh_te_node& x) {
  return x.kind == TE_ZERO || x.kind == TE_AND || x.kind == TE_UINT_PIN || (x.kind == TE_UINT_OP && x.op == 4) || (x.kind == TE_EC_OP && x.op == 3);
}
}  // namespace

extern "C" int mh_transcript_eval_plan(const mh_te_node* nodes, size_t n_nodes, const mh_te_term* terms, size_t n_terms, const uint32_t* limbs,
                                       size_t n_lit, uint64_t root, uint64_t p2_cycles, int log_n, uint32_t* row_start,
                                       mh_transcript_eval_info* info) {
  if (!info) return MH_ERR_INVALID;
  *info = mh_transcript_eval_info{};
  info->n_nodes = n_nodes;
  info->n_terms = n_terms;
  info->n_lit = n_lit;
  info->p2_cycles = p2_cycles;
  if (!nodes && n_nodes) return plan_defect(info, 1, 0, 0);
  if (!terms && n_terms) return plan_defect(info, 1, 0, 1);
  if (!limbs && n_lit) return plan_defect(info, 1, 0, 2);
  for (size_t i = 0; i < n_nodes; i++) {
    const mh_te_node& x = nodes[i];
    if (x.kind >= TE_N_KINDS) return plan_defect(info, 2, i, 0);
    if ((x.kind == TE_UINT_OP && (x.op < 1 || x.op > 4)) || (x.kind == TE_EC_OP && (x.op < 1 || x.op > 3))) return plan_defect(info, 2, i, 1);
  }
  for (size_t i = 0; i < n_nodes; i++) {
    const mh_te_node& x = nodes[i];
    switch (x.kind) {
      case TE_AND:  // a node below the own index, or any external cycle (ranged below: kind 5)
        if (x.lhs >= 0 && (uint64_t)x.lhs >= i) return plan_defect(info, 3, i, 0);
        if (x.rhs >= 0 && (uint64_t)x.rhs >= i) return plan_defect(info, 3, i, 1);
        break;
      case TE_UINT_LEAF: case TE_UINT_PIN:
        if (x.lhs < 0 || (uint64_t)x.lhs >= n_lit) return plan_defect(info, 3, i, 0);
        break;
      case TE_UINT_OP: case TE_EC_CREATE: case TE_EC_OP:
        if (x.lhs < 0 || (uint64_t)x.lhs >= i) return plan_defect(info, 3, i, 0);
        if (x.rhs < 0 || (uint64_t)x.rhs >= i) return plan_defect(info, 3, i, 1);
        break;
      case TE_EC_MSM: {
        if (x.rhs <= 0) return plan_defect(info, 3, i, 1);
        if (x.lhs < 0 || (uint64_t)x.lhs > n_terms || (uint64_t)x.rhs > n_terms - (uint64_t)x.lhs) return plan_defect(info, 3, i, 0);
        for (uint64_t t = (uint64_t)x.lhs; t < (uint64_t)x.lhs + (uint64_t)x.rhs; t++) {
          if (terms[t].base_node >= i) return plan_defect(info, 3, t, 2);
          if (terms[t].scalar_node >= i) return plan_defect(info, 3, t, 3);
        }
        break;
      }
      default: break;
    }
  }
  if (root >= n_nodes || !te_truthy(nodes[root])) return plan_defect(info, 4, root);
  for (size_t i = 0; i < n_nodes; i++) {
    const mh_te_node& x = nodes[i];
    if (x.kind == TE_ZERO) continue;
    const uint64_t span = x.kind == TE_EC_MSM ? (uint64_t)x.rhs : 1;
    if (x.perm >= p2_cycles || span > p2_cycles - x.perm) return plan_defect(info, 5, i, 0);
    if (x.kind == TE_AND) {
      // -1 - src without overflow: src = INT64_MIN gives 2^63 - 1
      if (x.lhs < 0 && (uint64_t)(-(x.lhs + 1)) >= p2_cycles) return plan_defect(info, 5, i, 1);
      if (x.rhs < 0 && (uint64_t)(-(x.rhs + 1)) >= p2_cycles) return plan_defect(info, 5, i, 2);
    }
  }
  // rows: the root's, then the other nodes' (a ZERO none, an MSM n_terms), then the merged ZERO row
  if (n_nodes > 2 * PLAN_MAX_ROWS) return plan_defect(info, 6, n_nodes);  // every ZERO is read by an AND of its own: more nodes than that fit no trace
  uint64_t at = 1, n_zero = 0;
  for (size_t i = 0; i < n_nodes; i++) {
    const mh_te_node& x = nodes[i];
    if (at > PLAN_MAX_ROWS) return plan_defect(info, 6, at);  // before a row_start that does not fit 32 bits, and before the sum can wrap
    if (row_start) row_start[i] = (uint32_t)at;
    if (i == root) continue;
    if (x.kind == TE_ZERO) n_zero++;
    else at += x.kind == TE_EC_MSM ? (uint64_t)x.rhs : 1;
  }
  info->n_zero = n_zero;
  info->active_rows = at + (n_zero ? 1 : 0);
  return tt_height(info, info->active_rows, log_n);
}
