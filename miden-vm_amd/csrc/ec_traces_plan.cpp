// The planner of the precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces (mh_ec_traces_plan): host only, no device
// pass.
//
// Validates what can be judged one record at a time plus prefix sums, and gives the four heights and every expression's first term row
// (what the device stage, ec_traces.hip, searches to find a row's expression).  Defects are looked for kind by kind, the lowest kind
// first, within it the lowest section and then the lowest index; a later kind is only looked for once the earlier ones are absent:
//   1 a NULL list where a count is nonzero        2 more than 2^24 rows in a trace, or a log_* above 24
//   3 a log_* below the height needed             4 a point's group that is 0 or above n_groups
//   5 a point kind outside 0..2, or pointers a point at infinity / a certified point does not have
//   6 an expression kind outside 0..2, n_rows = 0, an intro of more than one row, the n_rows not summing to n_terms
//   7 an operand that is 0 or not an earlier expression, or nonzero where the kind has none
// Whatever dereferences another record (kinds 8..15) is the device pass's to judge.
#include "ledger_plan.hpp"

extern "C" int mh_ec_traces_plan(const mh_ec_group* groups, size_t n_groups, const mh_ec_point* points, size_t n_points, const mh_ec_add_op* adds,
                                 size_t n_add, const mh_msm_expr* exprs, size_t n_exprs, const mh_msm_term* terms, size_t n_terms, int log_groups,
                                 int log_points, int log_add, int log_msm, uint32_t* row_start, mh_ec_traces_info* info) {
  if (!info) return MH_ERR_INVALID;
  *info = mh_ec_traces_info{};
  info->n_groups = n_groups;
  info->n_points = n_points;
  info->n_add = n_add;
  info->n_exprs = n_exprs;
  info->n_terms = n_terms;
  if (!groups && n_groups) return plan_defect_in(info, 0, 1, 0);
  if (!points && n_points) return plan_defect_in(info, 1, 1, 0);
  if (!adds && n_add) return plan_defect_in(info, 2, 1, 0);
  if (!exprs && n_exprs) return plan_defect_in(info, 3, 1, 0, 0);
  if (!terms && n_terms) return plan_defect_in(info, 3, 1, 0, 1);
  // heights: a count above the limit is not multiplied
  if (n_groups > PLAN_MAX_ROWS) return plan_defect_in(info, 0, 2, n_groups);
  if (n_points > PLAN_MAX_ROWS) return plan_defect_in(info, 1, 2, n_points);
  if (n_add > PLAN_MAX_ROWS / 4) return plan_defect_in(info, 2, 2, n_add);
  if (n_terms > PLAN_MAX_ROWS) return plan_defect_in(info, 3, 2, n_terms);
  const int logs[4] = {log_groups, log_points, log_add, log_msm};
  for (int s = 0; s < 4; s++)
    if (logs[s] > 24) return plan_defect_in(info, s, 2, (uint64_t)logs[s]);
  info->groups_rows_needed = pow2_at_least(n_groups, 2);
  info->points_rows_needed = pow2_at_least(n_points, 2);
  info->add_rows_needed = pow2_at_least(4 * (uint64_t)n_add, 4);
  info->msm_rows_needed = pow2_at_least(n_terms, 2);
  // all four heights are written before the first that does not fit is refused
  const uint64_t needed[4] = {info->groups_rows_needed, info->points_rows_needed, info->add_rows_needed, info->msm_rows_needed};
  uint64_t* const rows[4] = {&info->groups_rows, &info->points_rows, &info->add_rows, &info->msm_rows};
  bool fits[4];
  for (int s = 0; s < 4; s++) fits[s] = plan_height(logs[s], needed[s], rows[s]);
  for (int s = 0; s < 4; s++)
    if (!fits[s]) return plan_defect_in(info, s, 3, needed[s]);
  for (size_t i = 0; i < n_points; i++)
    if (points[i].group == 0 || points[i].group > n_groups) return plan_defect_in(info, 1, 4, i);
  for (size_t i = 0; i < n_points; i++) {
    const mh_ec_point& p = points[i];
    if (p.kind > 2) return plan_defect_in(info, 1, 5, i, 0);
    if (p.kind == 1 && (p.x_ptr || p.y_ptr)) return plan_defect_in(info, 1, 5, i, p.x_ptr ? 1 : 2);
    if (p.kind != 0 && (p.u_ptr || p.w_ptr)) return plan_defect_in(info, 1, 5, i, p.u_ptr ? 3 : 4);
  }
  {
    uint64_t sum = 0;
    for (size_t k = 0; k < n_exprs; k++) {
      const mh_msm_expr& e = exprs[k];
      if (e.kind > 2) return plan_defect_in(info, 3, 6, k, 0);
      if (e.n_rows == 0 || (e.kind == 0 && e.n_rows != 1)) return plan_defect_in(info, 3, 6, k, 1);
      sum += e.n_rows;  // at most 2^64 / 2^32 records of less than 2^32 each: no wrap
    }
    if (sum != n_terms) return plan_defect_in(info, 3, 6, n_exprs, 2);
  }
  for (size_t k = 0; k < n_exprs; k++) {
    const mh_msm_expr& e = exprs[k];
    const bool a_bad = e.kind == 0 ? e.a_expr != 0 : (e.a_expr == 0 || e.a_expr > k);  // expression k is pointer k + 1: the earlier ones are 1..k
    const bool b_bad = e.kind == 1 ? (e.b_expr == 0 || e.b_expr > k) : e.b_expr != 0;
    if (a_bad || b_bad) return plan_defect_in(info, 3, 7, k, a_bad ? 0 : 1);
  }
  if (row_start) {
    uint32_t at = 0;
    for (size_t k = 0; k < n_exprs; k++) {
      row_start[k] = at;
      at += exprs[k].n_rows;
    }
  }
  return MH_OK;
}
