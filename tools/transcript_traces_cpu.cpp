// The ChunkNode and TranscriptEval traces' per-lane bodies (miden-vm_amd/csrc/transcript_traces_rows.cuh) run lane by lane on the host:
// what mh_chunk_node_trace_build and mh_transcript_eval_trace_build do, without a device.  tests/test_transcript_traces_cpu.py loads
// this as a shared library and compares every cell with the Python generators and every refusal with the one it expects of the device.
// The planners are compiled in; `p2` is the Poseidon2 chiplet trace column-major (the device's layout) of 2^log_p2 rows; the out matrix
// is the caller's, column-major, of the height the planner gives.  Host side only (--offload-host-only): no kernel, no GPU call.
#include "../miden-vm_amd/csrc/transcript_traces_rows.cuh"
#include <vector>

namespace {
template <class Info>
int unpack(unsigned long long defect, Info* info) {
  const LedgerDefect d = ledger_unpack(defect);
  info->defect_kind = d.kind; info->defect_index = d.index; info->defect_operand = d.operand;
  return MH_ERR_INVALID;
}
}  // namespace

extern "C" int chunk_node_cpu(const u64* p2, int log_p2, const uint8_t* bytes, size_t n_bytes, const uint8_t* digests, const mh_kn_record* records,
                              size_t n, int log_n, u64* out, mh_chunk_node_info* info) {
  const P2View view{p2, (u64)1 << log_p2, ((u64)1 << log_p2) / P2_PERIOD};
  if (mh_chunk_node_plan(bytes, n_bytes, digests, records, n, view.cycles, log_n, info) != MH_OK) return MH_ERR_INVALID;
  unsigned long long defect = ~0ull;
  const u64 next_perm = n ? records[n - 1].perm_chunks + (info->n_chunks - records[n - 1].chunk_head) : 0;
  const CnLists L{bytes, digests, records, (u32)n, (u32)info->n_chunks, next_perm, view, &defect};
  for (u32 t = 0; t < L.total_chunks; t++) cn_chunk_check(L, t);
  for (u32 i = 0; i < L.n; i++) cn_record_check(L, i);
  if (defect != ~0ull) return unpack(defect, info);
  for (u64 t = 0; t < info->rows; t++) cn_row(L, info->rows, out, t);
  return MH_OK;
}

extern "C" int transcript_eval_cpu(const u64* p2, int log_p2, const mh_te_node* nodes, size_t n_nodes, const mh_te_term* terms, size_t n_terms,
                                   const uint32_t* limbs, size_t n_lit, uint64_t root, int log_n, u64* out, u64* root_felts,
                                   mh_transcript_eval_info* info) {
  const P2View view{p2, (u64)1 << log_p2, ((u64)1 << log_p2) / P2_PERIOD};
  std::vector<u32> row_start(n_nodes);
  if (mh_transcript_eval_plan(nodes, n_nodes, terms, n_terms, limbs, n_lit, root, view.cycles, log_n, row_start.data(), info) != MH_OK)
    return MH_ERR_INVALID;
  std::vector<u32> count(n_nodes, 0);
  unsigned long long defect = ~0ull;
  const u32 n_body = (u32)(info->active_rows - (info->n_zero ? 1 : 0));
  const TeLists L{nodes, terms, limbs, row_start.data(), (u32)n_nodes, (u32)n_terms, (u32)root, n_body, info->n_zero, count.data(), view, &defect};
  for (u32 r = 0; r < n_body; r++) te_row_check(L, r);
  for (u32 i = 0; i < L.n_nodes; i++) te_read_check(L, i);
  if (defect != ~0ull) return unpack(defect, info);
  for (u64 r = 0; r < info->rows; r++) te_row(L, info->rows, out, r);
  if (root_felts)
    for (int j = 0; j < 4; j++) root_felts[j] = out[(size_t)(TEC_H + j) * info->rows];
  return MH_OK;
}
