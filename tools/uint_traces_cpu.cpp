// The uint traces' per-lane bodies (miden-vm_amd/csrc/uint_traces_rows.cuh) run lane by lane on the host: what mh_uint_traces_build
// does, without a device.  tests/test_uint_traces_cpu.py loads this as a shared library and compares every cell with the Python
// generators and every refusal with the one it expects of the device.  The planner is compiled in; the out matrices are the caller's,
// column-major, of the heights mh_uint_traces_plan gives.  Host side only (--offload-host-only): no kernel is compiled and no GPU call
// is made.
#include "../miden-vm_amd/csrc/uint_traces_rows.cuh"
#include <vector>

extern "C" int uint_traces_cpu(const mh_uint_row* rows, size_t n_store, const mh_uint_mul_op* muls, size_t n_mul, const mh_uint_add_op* adds, size_t n_add,
                               int log_usm, int log_add, u64* usm_out, u64* add_out, mh_uint_traces_info* info) {
  std::vector<u32> bound_index(n_store);
  if (mh_uint_traces_plan(rows, n_store, muls, n_mul, adds, n_add, log_usm, log_add, bound_index.data(), info) != MH_OK) return MH_ERR_INVALID;
  std::vector<u32> count(2 * n_store + 1, 0), mrec(n_mul * UT_MREC + 1), arec(n_add * UT_AREC + 1);
  unsigned long long defect = ~0ull;
  const UtLists L{rows, bound_index.data(), muls, adds, (u32)n_store, (u32)n_mul, (u32)n_add, count.data(), mrec.data(), arec.data(), &defect};
  for (u32 i = 0; i < L.n_store; i++) ut_self(L, i);
  for (u32 i = 0; i < L.n_mul; i++) ut_mul_witness(L, i);
  for (u32 i = 0; i < L.n_add; i++) ut_add_witness(L, i);
  if (const LedgerDefect d = ledger_unpack(defect); d.kind) {
    info->defect_kind = d.kind; info->defect_section = d.section; info->defect_index = d.index; info->defect_operand = d.operand;
    return MH_ERR_INVALID;
  }
  for (u64 t = 0; t < info->usm_rows; t++) ut_usm_row(L, info->usm_rows, usm_out, t);
  for (u64 t = 0; t < info->add_rows; t++) ut_add_row(L, info->add_rows, add_out, t);
  return MH_OK;
}
