// The planner of the precompile prover's UintStoreMul and UintAdd traces (mh_uint_traces_plan): host only, no device pass.
//
// Validates what the device stage (uint_traces.hip) indexes with and gives the two heights and, for every store row, the index of its
// bound's row.  Nothing here multiplies or divides a 256-bit value; kind 7 is one eight-limb compare per row.  Defects are looked for kind
// by kind, the lowest kind first and within it the lowest index; a later kind is only looked for once the earlier ones are absent:
//   1 a NULL pointer where a count is nonzero     2 more than 2^24 rows in either trace, or padding pointers reaching 2^32
//   3 log_usm / log_add below the height needed   4 a store ptr that is 0 or not above the one before
//   5 a gap to the next ptr >= 2^16               6 a bound_ptr that is not stored     7 a value above its bound's
// The relations' own pointers and operands (kinds 8..14) are the witness pass's to judge.
#include "ledger_plan.hpp"
#include <vector>

namespace {
// the index of the row with pointer `ptr`, or n
size_t ut_find(const mh_uint_row* rows, size_t n, uint32_t ptr) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (rows[mid].ptr < ptr) lo = mid + 1; else hi = mid;
  }
  return lo < n && rows[lo].ptr == ptr ? lo : n;
}
}  // namespace

extern "C" int mh_uint_traces_plan(const mh_uint_row* rows, size_t n_store, const mh_uint_mul_op* muls, size_t n_mul, const mh_uint_add_op* adds,
                                   size_t n_add, int log_usm, int log_add, uint32_t* bound_index, mh_uint_traces_info* info) {
  if (!info) return MH_ERR_INVALID;
  *info = mh_uint_traces_info{};
  info->n_store = n_store;
  info->n_mul = n_mul;
  info->n_add = n_add;
  if (!rows && n_store) return plan_defect_in(info, 0, 1, 0);
  if (!muls && n_mul) return plan_defect_in(info, 1, 1, 0);
  if (!adds && n_add) return plan_defect_in(info, 2, 1, 0);
  // heights: a count above 2^24 cannot fit whatever the factor, and is not multiplied
  if (n_store > PLAN_MAX_ROWS / 4) return plan_defect_in(info, 0, 2, n_store);
  if (n_mul > PLAN_MAX_ROWS / 8) return plan_defect_in(info, 1, 2, n_mul);
  if (n_add > PLAN_MAX_ROWS / 2) return plan_defect_in(info, 2, 2, n_add);
  const uint64_t mul_rows = pow2_at_least(8 * (uint64_t)n_mul, 8);
  uint64_t blocks = pow2_at_least(n_store, 1);
  if (blocks < mul_rows / 4) blocks = mul_rows / 4;
  info->usm_rows_needed = 4 * blocks;
  info->add_rows_needed = pow2_at_least(2 * (uint64_t)n_add, 2);
  if (log_usm > 24) return plan_defect_in(info, 0, 2, log_usm);
  if (log_add > 24) return plan_defect_in(info, 2, 2, log_add);
  const bool usm_fits = plan_height(log_usm, info->usm_rows_needed, &info->usm_rows), add_fits = plan_height(log_add, info->add_rows_needed, &info->add_rows);
  {  // padding blocks take last ptr + 1 + k: the last of them must stay a 32-bit pointer
    const uint64_t taken = info->usm_rows > info->usm_rows_needed ? info->usm_rows : info->usm_rows_needed;
    const uint64_t last = n_store ? rows[n_store - 1].ptr : 0;
    if (last + (taken / 4 - n_store) > 0xffffffffull) return plan_defect_in(info, 0, 2, taken / 4 - n_store);
  }
  if (!usm_fits) return plan_defect_in(info, 0, 3, info->usm_rows_needed);
  if (!add_fits) return plan_defect_in(info, 2, 3, info->add_rows_needed);
  for (size_t i = 0; i < n_store; i++)
    if (rows[i].ptr == 0 || (i && rows[i].ptr <= rows[i - 1].ptr)) return plan_defect_in(info, 0, 4, i);
  for (size_t i = 0; i + 1 < n_store; i++)
    if (rows[i + 1].ptr - rows[i].ptr - 1 >= 0x10000u) return plan_defect_in(info, 0, 5, i);
  std::vector<uint32_t> own;
  uint32_t* bi = bound_index;
  if (!bi) {
    own.resize(n_store);
    bi = own.data();
  }
  for (size_t i = 0; i < n_store; i++) {
    const size_t b = rows[i].bound_ptr == rows[i].ptr ? i : ut_find(rows, n_store, rows[i].bound_ptr);
    if (b == n_store) return plan_defect_in(info, 0, 6, i);
    bi[i] = (uint32_t)b;
  }
  for (size_t i = 0; i < n_store; i++) {
    const uint32_t* v = rows[i].value;
    const uint32_t* b = rows[bi[i]].value;
    for (int j = 7; j >= 0; j--) {
      if (v[j] > b[j]) return plan_defect_in(info, 0, 7, i);
      if (v[j] < b[j]) break;
    }
  }
  return MH_OK;
}
