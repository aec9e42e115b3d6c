// The precompile prover's EcGroups (6 columns), EcPointStore (14), EcGroupAdd (21) and EcMsm (38) main traces built on the device from
// the ledgers (mh_ec_traces_build), gfx950.
//
// Replaces EcStoreRequires::generate_traces (ec/trace.rs:347-411), EcAddRequires::generate_trace / op_block (ec/add/trace.rs:146-251)
// and EcMsmRequires::generate_trace (ec/msm/trace.rs:390-500).  These four traces hold pointers only: the host sends the group table,
// the point store, one 56-byte record per addition, one 48-byte record per expression and (base, scalar) per term row; the planner
// (ec_traces_plan.cpp, host only) has validated what one record shows and given the heights and every expression's first term row.
// Two stages with one read-back between them:
//   check    ec_point_check    a lane per point: its read of its group.
//            ec_add_check      a lane per addition: p, q, r and the group in range, the kind against which operands are points at
//                              infinity, the mint's ordering; then its reads of p, q and, in the live cases, of r and the group.
//            ec_expr_check     a lane per expression: val and group in range and consistent, an intro's base; its reads of the group,
//                              of its operands and (neg) of the two value points.
//            ec_term_check     a lane per term row: its expression by a search over the first rows, the bases' order, and for a combine
//                              the merge: this row's cursors (two binary searches) advanced by its takes against the next row's.
//            The counters are integers added once per wave where the lanes agree (wave_count.cuh): in a session every point and every
//            live addition reads ONE group.  Defects (kinds 8..15) go into one packed 64-bit minimum: kind, section, index, operand.
//   rows     after the minimum has been read back clean and the traces are allocated: ec_groups_row, ec_points_row,
//            ec_add_row (four roles per block) and ec_msm_row, a lane per trace row, padding included.  Consecutive lanes hold
//            consecutive rows of a column-major column: every store is a whole line.
// The bodies named above are in ec_traces_rows.cuh; their kernels are ledger_stage.cuh's lane_per_record<body> and lane_per_row<body>, as
// the defect word, its read-back and the refusal's message are.  The counters and the minimum are scratch that the call clears itself; every cell of the four
// traces has exactly one writer: a second call leaves the same bytes.  No LDS, no scratch memory.
#include "section_out.cuh"
#include "ec_traces_rows.cuh"
#include <vector>

static_assert(sizeof(mh_ec_group) == 24, "mh_ec_group is 24 bytes");
static_assert(sizeof(mh_ec_point) == 32, "mh_ec_point is 32 bytes");
static_assert(sizeof(mh_ec_add_op) == 56, "mh_ec_add_op is 56 bytes");
static_assert(sizeof(mh_msm_expr) == 48, "mh_msm_expr is 48 bytes");
static_assert(sizeof(mh_msm_term) == 8, "mh_msm_term is 8 bytes");
static_assert(sizeof(mh_ec_traces_info) == 128, "mh_ec_traces_info is 128 bytes");

namespace {
constexpr int EC_BT = 256;
const char* const EC_WHAT[] = {"",
                               "a null list where a count is nonzero",
                               "more than 2^24 rows in a trace, or a log_* above 24",
                               "the trace does not fit its log_* (index: rows needed)",
                               "a point's group that is 0 or above n_groups",
                               "a point kind outside 0..2, or pointers a point at infinity / a certified point does not have",
                               "an expression kind outside 0..2, n_rows = 0, an intro of more than one row, or the n_rows not summing to n_terms",
                               "an operand that is 0 or not an earlier expression, or nonzero where the kind has none",
                               "a point or group pointer that is 0 or out of range",
                               "an addition kind outside 0..5, or mints outside {0, 1} or on a kind other than double / generic",
                               "an operand, result or value stored under another group",
                               "an addition whose kind disagrees with which of p, q are points at infinity",
                               "mints with r <= p, r <= q or an r that is not a certified row",
                               "an expression's bases not strictly ascending",
                               "a row neither operand holds, a merge that skips a term, or a neg that does not follow its operand's rows",
                               "an intro whose val is not its base"};

[[noreturn]] void ec_refuse(const mh_ec_traces_info* info) {
  ledger_refuse("mh_ec_traces_build", {info->defect_kind, info->defect_section, info->defect_index, info->defect_operand}, EC_WHAT[info->defect_kind]);
}
}  // namespace

extern "C" int mh_ec_traces_build(mh_ctx* c, const mh_ec_group* groups, size_t n_groups, const mh_ec_point* points, size_t n_points,
                                  const mh_ec_add_op* adds, size_t n_add, const mh_msm_expr* exprs, size_t n_exprs, const mh_msm_term* terms,
                                  size_t n_terms, int log_groups, int log_points, int log_add, int log_msm, mh_trace** groups_out,
                                  mh_trace** points_out, mh_trace** add_out, mh_trace** msm_out, mh_ec_traces_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_ec_traces_info local;
  if (!info) info = &local;
  try {
    *info = mh_ec_traces_info{};
    info->n_groups = n_groups; info->n_points = n_points; info->n_add = n_add; info->n_exprs = n_exprs; info->n_terms = n_terms;
    if (!groups_out || !points_out || !add_out || !msm_out) {
      info->defect_kind = 1;
      ec_refuse(info);
    }
    std::vector<u32> row_start(n_exprs <= ((size_t)1 << 24) ? n_exprs : 0);  // more expressions than rows: the planner refuses (kind 6)
    if (mh_ec_traces_plan(groups, n_groups, points, n_points, adds, n_add, exprs, n_exprs, terms, n_terms, log_groups, log_points, log_add, log_msm,
                          row_start.empty() ? nullptr : row_start.data(), info) != MH_OK)
      ec_refuse(info);
    HIP_CHECK(hipSetDevice(c->device));
    const size_t n_count = n_groups + n_points + n_exprs;
    DevBuf dgroups(n_groups * sizeof(mh_ec_group)), dpoints(n_points * sizeof(mh_ec_point)), dadds(n_add * sizeof(mh_ec_add_op)),
        dexprs(n_exprs * sizeof(mh_msm_expr)), dterms(n_terms * sizeof(mh_msm_term)), dstart(n_exprs * 4), dcount(n_count * 4), ddefect(8);
    c->h2d(dgroups.p, groups, n_groups * sizeof(mh_ec_group));
    c->h2d(dpoints.p, points, n_points * sizeof(mh_ec_point));
    c->h2d(dadds.p, adds, n_add * sizeof(mh_ec_add_op));
    c->h2d(dexprs.p, exprs, n_exprs * sizeof(mh_msm_expr));
    c->h2d(dterms.p, terms, n_terms * sizeof(mh_msm_term));
    c->h2d(dstart.p, row_start.data(), n_exprs * 4);
    if (n_count) HIP_CHECK(hipMemsetAsync(dcount.p, 0, n_count * 4, c->stream));
    HIP_CHECK(hipMemsetAsync(ddefect.p, 0xff, 8, c->stream));
    u32* count = (u32*)dcount.p;
    const EcLists L{(const mh_ec_group*)dgroups.p, (const mh_ec_point*)dpoints.p, (const mh_ec_add_op*)dadds.p, (const mh_msm_expr*)dexprs.p,
                    (const mh_msm_term*)dterms.p, (const u32*)dstart.p, (u32)n_groups, (u32)n_points, (u32)n_add, (u32)n_exprs, (u32)n_terms,
                    count, count + n_groups, count + n_groups + n_points, (unsigned long long*)ddefect.p};
    if (n_points) {
      ProfScope ps(c, "ec_point_check", (double)n_points * sizeof(mh_ec_point));
      launch_per_record<EcLists, &EcLists::n_points, ec_point_check, EC_BT>(c, L);
    }
    if (n_add) {
      ProfScope ps(c, "ec_add_check", (double)n_add * (sizeof(mh_ec_add_op) + 3 * sizeof(mh_ec_point)));
      launch_per_record<EcLists, &EcLists::n_add, ec_add_check, EC_BT>(c, L);
    }
    if (n_exprs) {
      ProfScope ps(c, "ec_expr_check", (double)n_exprs * 3 * sizeof(mh_msm_expr));
      launch_per_record<EcLists, &EcLists::n_exprs, ec_expr_check, EC_BT>(c, L);
    }
    if (n_terms) {
      ProfScope ps(c, "ec_term_check", (double)n_terms * (sizeof(mh_msm_expr) + 3 * sizeof(mh_msm_term)));
      launch_per_record<EcLists, &EcLists::n_terms, ec_term_check, EC_BT>(c, L);
    }
    const LedgerDefect d = ledger_read_defect(c, ddefect.p, 8, 15, "mh_ec_traces_build", "checking");
    if (d.kind) {
      info->defect_kind = d.kind; info->defect_section = d.section; info->defect_index = d.index; info->defect_operand = d.operand;
      ec_refuse(info);
    }
    std::unique_ptr<mh_trace> tg = trace_new(c, ceil_log2(info->groups_rows), EC_GROUPS_WIDTH), tp = trace_new(c, ceil_log2(info->points_rows), EC_POINTS_WIDTH),
                              ta = trace_new(c, ceil_log2(info->add_rows), EC_ADD_WIDTH), tm = trace_new(c, ceil_log2(info->msm_rows), EC_MSM_WIDTH);
    {
      ProfScope ps(c, "ec_groups_rows", 8.0 * EC_GROUPS_WIDTH * (double)info->groups_rows);
      launch_per_row<EcLists, ec_groups_row, EC_BT>(c, L, info->groups_rows, tg->cols.u());
    }
    {
      ProfScope ps(c, "ec_points_rows", 8.0 * EC_POINTS_WIDTH * (double)info->points_rows);
      launch_per_row<EcLists, ec_points_row, EC_BT>(c, L, info->points_rows, tp->cols.u());
    }
    {
      ProfScope ps(c, "ec_add_rows", 8.0 * EC_ADD_WIDTH * (double)info->add_rows);
      launch_per_row<EcLists, ec_add_row, EC_BT>(c, L, info->add_rows, ta->cols.u());
    }
    {
      ProfScope ps(c, "ec_msm_rows", 8.0 * EC_MSM_WIDTH * (double)info->msm_rows);
      launch_per_row<EcLists, ec_msm_row, EC_BT>(c, L, info->msm_rows, tm->cols.u());
    }
    // the lists and counters are pooled buffers: they go back to the pool when this scope ends, ordered behind the row kernels on the stream
    *groups_out = tg.release();
    *points_out = tp.release();
    *add_out = ta.release();
    *msm_out = tm.release();
    return MH_OK;
  }
  SEC_CATCH
}
