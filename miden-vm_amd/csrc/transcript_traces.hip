// The precompile prover's ChunkNode (42 columns) and TranscriptEval (39) main traces built on the device from the ledgers and the
// device-resident Poseidon2 chiplet trace (mh_chunk_node_trace_build, mh_transcript_eval_trace_build), gfx950.
//
// Replaces generate_trace_padded_to (hash/chunk/trace.rs:133-175), generate_trace / push_row (hash/keccak/node/trace.rs:52-113), their
// union (hash/chunk_node/trace.rs:24-45) and generate_trace / push_node_row (transcript/eval/trace.rs:895-1155).  A node row holds three
// Poseidon2 digests, an eval row its operands' hashes and its own: the generators permute on the host for them.  Here every digest is
// read where it already lies, on row 15 of a cycle of the Poseidon2 trace that mh_poseidon2_chiplet_trace_build laid (with digest
// references: no permutation on the host there either), on the context's stream behind the kernels that wrote it.  The host sends the
// message bytes, the Keccak digests and 64 bytes a record; the transcript as 64 bytes a node, 8 a term row and 32 a literal.  The
// planners (transcript_traces_plan.cpp, host only) have ranged every index and cycle and given the heights and every node's first row.
// Each build has two stages with one read-back between them:
//   check    cn_chunk_check     a lane per chunk row: is_absorb of its cycle is 0 on a chain's head and 1 behind it.
//            cn_record_check    a lane per record: the three digest cycles end an absorption.
//            te_row_check       a lane per active row: its node by a search over the first rows; the operands' classes, moduli and
//                               `is` pointers, the node's cycle (an MSM row's: its place in the span) against the absorptions, and the
//                               reads of the operands, integers added once per wave where the lanes agree (wave_count.cuh).
//            te_read_check      a lane per node, behind the counting: a truthy node is read once, the root never, a value node at all.
//            Defects (kinds 8..) go into one packed 64-bit minimum: kind, index, operand.
//   rows     after the minimum has been read back clean and the trace is allocated: cn_row, te_row, a lane per trace row, padding
//            included.  Consecutive lanes hold consecutive rows of a column-major column: every store is a whole line.
// The bodies named above are in transcript_traces_rows.cuh; their kernels are ledger_stage.cuh's lane_per_record<body> and
// lane_per_row<body>, as the defect word, its read-back and the refusal's message are.  The counters and the minimum are scratch that the call clears itself; every cell has
// exactly one writer: a second call leaves the same bytes.  No LDS.
#include "section_out.cuh"
#include "transcript_traces_rows.cuh"
#include <vector>

static_assert(sizeof(mh_kn_record) == 64, "mh_kn_record is 64 bytes");
static_assert(sizeof(mh_chunk_node_info) == 56, "mh_chunk_node_info is 56 bytes");
static_assert(sizeof(mh_te_node) == 64, "mh_te_node is 64 bytes");
static_assert(sizeof(mh_te_term) == 8, "mh_te_term is 8 bytes");
static_assert(sizeof(mh_transcript_eval_info) == 80, "mh_transcript_eval_info is 80 bytes");

namespace {
constexpr int TT_BT = 256;
const char* const CN_WHAT[] = {"",
                               "a null pointer where one is required, or a p2 that is not a 32-column trace of this context",
                               "offset + len past n_bytes",
                               "a chunk_head that is not the running sum of the chunk counts",
                               "a sponge_head that is not a multiple of 32",
                               "a cycle at or beyond the cycles of p2",
                               "more than 2^24 rows, or a log_n above 24",
                               "the trace does not fit its log_n (index: rows needed)",
                               "a chunk chain that is not one absorption of p2",
                               "a digest cycle that does not end an absorption of p2"};
const char* const TE_WHAT[] = {"",
                               "a null pointer where one is required, or a p2 that is not a 32-column trace of this context",
                               "an unknown kind, or an op outside the kind's range",
                               "a source, literal, term span or term node out of range or not below the own index",
                               "a root index out of range, or a root that is not of a truthy kind",
                               "a cycle at or beyond the cycles of p2",
                               "more than 2^24 rows or 2^25 nodes, or a log_n above 24",
                               "the trace does not fit its log_n (index: rows needed)",
                               "an operand of the wrong class",
                               "operands under different moduli",
                               "an `is` over distinct pointers",
                               "a truthy node not read exactly once, or the root read",
                               "a value node nobody reads",
                               "a perm that is not a one-block absorption of p2",
                               "an MSM span that is not one absorption of n_terms blocks",
                               "an external cycle that does not end an absorption"};

template <class Info>
[[noreturn]] void tt_refuse(const char* entry, const Info* info, const char* const* what) {
  ledger_refuse(entry, {info->defect_kind, -1, info->defect_index, info->defect_operand}, what[info->defect_kind]);
}

// kind 1, operands 3 and 4: the Poseidon2 trace and the out pointer
template <class Info>
void tt_require_args(mh_ctx* c, const mh_trace* p2, const void* out, const char* entry, Info* info, const char* const* what) {
  const bool bad_p2 = !p2 || p2->ctx != c || p2->width != (size_t)P2_WIDTH || p2->log_n < 4 || p2->log_n > 24;
  if (bad_p2 || !out) {
    info->defect_kind = 1;
    info->defect_operand = bad_p2 ? 3 : 4;
    tt_refuse(entry, info, what);
  }
}

template <class Info>
void tt_read_defect(mh_ctx* c, const DevBuf& ddefect, int last_kind, const char* entry, Info* info, const char* const* what) {
  const LedgerDefect d = ledger_read_defect(c, ddefect.p, 8, last_kind, entry, "checking");
  if (!d.kind) return;
  info->defect_kind = d.kind; info->defect_index = d.index; info->defect_operand = d.operand;
  tt_refuse(entry, info, what);
}

P2View tt_p2(const mh_trace* p2) { return P2View{p2->cols.u(), (u64)1 << p2->log_n, ((u64)1 << p2->log_n) / P2_PERIOD}; }
}  // namespace

extern "C" int mh_chunk_node_trace_build(mh_ctx* c, const mh_trace* p2, const uint8_t* bytes, size_t n_bytes, const uint8_t* digests,
                                         const mh_kn_record* records, size_t n, int log_n, mh_trace** out, mh_chunk_node_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_chunk_node_info local;
  if (!info) info = &local;
  const char* const entry = "mh_chunk_node_trace_build";
  try {
    *info = mh_chunk_node_info{};
    info->n_records = n;
    tt_require_args(c, p2, out, entry, info, CN_WHAT);
    const P2View view = tt_p2(p2);
    if (mh_chunk_node_plan(bytes, n_bytes, digests, records, n, view.cycles, log_n, info) != MH_OK) tt_refuse(entry, info, CN_WHAT);
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, p2);
    DevBuf dbytes(n_bytes), ddig(n * 32), drec(n * sizeof(mh_kn_record)), ddefect(8);
    c->h2d(dbytes.p, bytes, n_bytes);
    c->h2d(ddig.p, digests, n * 32);
    c->h2d(drec.p, records, n * sizeof(mh_kn_record));
    HIP_CHECK(hipMemsetAsync(ddefect.p, 0xff, 8, c->stream));
    const u64 next_perm = n ? records[n - 1].perm_chunks + (info->n_chunks - records[n - 1].chunk_head) : 0;
    const CnLists L{(const uint8_t*)dbytes.p, (const uint8_t*)ddig.p, (const mh_kn_record*)drec.p, (u32)n, (u32)info->n_chunks, next_perm, view,
                    (unsigned long long*)ddefect.p};
    if (n) {
      {
        ProfScope ps(c, "cn_chunk_check", (double)info->n_chunks * 8);
        launch_per_record<CnLists, &CnLists::total_chunks, cn_chunk_check, TT_BT>(c, L);
      }
      {
        ProfScope ps(c, "cn_record_check", (double)n * (sizeof(mh_kn_record) + 15 * 8));
        launch_per_record<CnLists, &CnLists::n, cn_record_check, TT_BT>(c, L);
      }
    }
    tt_read_defect(c, ddefect, 9, entry, info, CN_WHAT);
    std::unique_ptr<mh_trace> t = trace_new(c, ceil_log2(info->rows), CN_WIDTH);
    {
      ProfScope ps(c, "cn_rows", 8.0 * CN_WIDTH * (double)info->rows);
      launch_per_row<CnLists, cn_row, TT_BT>(c, L, info->rows, t->cols.u());
    }
    // the lists are pooled buffers: they go back to the pool when this scope ends, ordered behind the row kernel on the stream
    *out = t.release();
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_transcript_eval_trace_build(mh_ctx* c, const mh_trace* p2, const mh_te_node* nodes, size_t n_nodes, const mh_te_term* terms,
                                              size_t n_terms, const uint32_t* limbs, size_t n_lit, uint64_t root, int log_n, mh_trace** out,
                                              uint64_t* root_felts, mh_transcript_eval_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_transcript_eval_info local;
  if (!info) info = &local;
  const char* const entry = "mh_transcript_eval_trace_build";
  try {
    *info = mh_transcript_eval_info{};
    info->n_nodes = n_nodes; info->n_terms = n_terms; info->n_lit = n_lit;
    tt_require_args(c, p2, out, entry, info, TE_WHAT);
    const P2View view = tt_p2(p2);
    std::vector<u32> row_start(n_nodes <= ((size_t)1 << 25) ? n_nodes : 0);  // more nodes than that: the planner refuses (kind 6)
    if (mh_transcript_eval_plan(nodes, n_nodes, terms, n_terms, limbs, n_lit, root, view.cycles, log_n, row_start.empty() ? nullptr : row_start.data(),
                                info) != MH_OK)
      tt_refuse(entry, info, TE_WHAT);
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, p2);
    DevBuf dnodes(n_nodes * sizeof(mh_te_node)), dterms(n_terms * sizeof(mh_te_term)), dlimbs(n_lit * 32), dstart(n_nodes * 4), dcount(n_nodes * 4),
        ddefect(8);
    c->h2d(dnodes.p, nodes, n_nodes * sizeof(mh_te_node));
    c->h2d(dterms.p, terms, n_terms * sizeof(mh_te_term));
    c->h2d(dlimbs.p, limbs, n_lit * 32);
    c->h2d(dstart.p, row_start.data(), n_nodes * 4);
    HIP_CHECK(hipMemsetAsync(dcount.p, 0, n_nodes * 4, c->stream));
    HIP_CHECK(hipMemsetAsync(ddefect.p, 0xff, 8, c->stream));
    const u32 n_body = (u32)(info->active_rows - (info->n_zero ? 1 : 0));
    const TeLists L{(const mh_te_node*)dnodes.p, (const mh_te_term*)dterms.p, (const uint32_t*)dlimbs.p, (const u32*)dstart.p, (u32)n_nodes, (u32)n_terms,
                    (u32)root, n_body, info->n_zero, (u32*)dcount.p, view, (unsigned long long*)ddefect.p};
    {
      ProfScope ps(c, "te_row_check", (double)n_body * 3 * sizeof(mh_te_node));
      launch_per_record<TeLists, &TeLists::n_body, te_row_check, TT_BT>(c, L);
    }
    {
      ProfScope ps(c, "te_read_check", (double)n_nodes * (sizeof(mh_te_node) + 4));
      launch_per_record<TeLists, &TeLists::n_nodes, te_read_check, TT_BT>(c, L);
    }
    tt_read_defect(c, ddefect, 15, entry, info, TE_WHAT);
    std::unique_ptr<mh_trace> t = trace_new(c, ceil_log2(info->rows), TE_WIDTH);
    {
      ProfScope ps(c, "te_rows", 8.0 * TE_WIDTH * (double)info->rows);
      launch_per_row<TeLists, te_row, TT_BT>(c, L, info->rows, t->cols.u());
    }
    if (root_felts) {  // the statement's public input: row 0's h, four columns a height apart, in one copy
      HIP_CHECK(hipMemcpy2DAsync(root_felts, 8, t->cols.u() + (size_t)TEC_H * info->rows, info->rows * 8, 8, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    *out = t.release();
    return MH_OK;
  }
  SEC_CATCH
}
