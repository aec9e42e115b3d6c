// The EC traces' per-lane bodies (miden-vm_amd/csrc/ec_traces_rows.cuh) run lane by lane on the host: what mh_ec_traces_build does,
// without a device.  tests/test_ec_traces_cpu.py loads this as a shared library and compares every cell with the Python generators and
// every refusal with the one it expects of the device.  The planner is compiled in; the out matrices are the caller's, column-major, of
// the heights mh_ec_traces_plan gives.  Host side only (--offload-host-only): no kernel is compiled and no GPU call is made.
#include "../miden-vm_amd/csrc/ec_traces_rows.cuh"
#include <vector>

extern "C" int ec_traces_cpu(const mh_ec_group* groups, size_t n_groups, const mh_ec_point* points, size_t n_points, const mh_ec_add_op* adds, size_t n_add,
                             const mh_msm_expr* exprs, size_t n_exprs, const mh_msm_term* terms, size_t n_terms, int log_groups, int log_points,
                             int log_add, int log_msm, u64* groups_out, u64* points_out, u64* add_out, u64* msm_out, mh_ec_traces_info* info) {
  std::vector<u32> row_start(n_exprs);
  if (mh_ec_traces_plan(groups, n_groups, points, n_points, adds, n_add, exprs, n_exprs, terms, n_terms, log_groups, log_points, log_add, log_msm,
                        row_start.data(), info) != MH_OK)
    return MH_ERR_INVALID;
  std::vector<u32> count(n_groups + n_points + n_exprs + 1, 0);
  unsigned long long defect = ~0ull;
  const EcLists L{groups, points, adds, exprs, terms, row_start.data(), (u32)n_groups, (u32)n_points, (u32)n_add, (u32)n_exprs, (u32)n_terms,
                  count.data(), count.data() + n_groups, count.data() + n_groups + n_points, &defect};
  for (u32 i = 0; i < L.n_points; i++) ec_point_check(L, i);
  for (u32 i = 0; i < L.n_add; i++) ec_add_check(L, i);
  for (u32 i = 0; i < L.n_exprs; i++) ec_expr_check(L, i);
  for (u32 i = 0; i < L.n_terms; i++) ec_term_check(L, i);
  if (const LedgerDefect d = ledger_unpack(defect); d.kind) {
    info->defect_kind = d.kind; info->defect_section = d.section; info->defect_index = d.index; info->defect_operand = d.operand;
    return MH_ERR_INVALID;
  }
  for (u64 t = 0; t < info->groups_rows; t++) ec_groups_row(L, info->groups_rows, groups_out, t);
  for (u64 t = 0; t < info->points_rows; t++) ec_points_row(L, info->points_rows, points_out, t);
  for (u64 t = 0; t < info->add_rows; t++) ec_add_row(L, info->add_rows, add_out, t);
  for (u64 t = 0; t < info->msm_rows; t++) ec_msm_row(L, info->msm_rows, msm_out, t);
  return MH_OK;
}
