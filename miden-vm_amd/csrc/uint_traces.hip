// The precompile prover's UintStoreMul (44 columns) and UintAdd (30 columns) main traces built on the device from the ledgers
// (mh_uint_traces_build), gfx950.
//
// Replaces UintStoreRequires / UintMulRequires / UintAddRequires' generate_trace (uint/trace.rs:273-386, uint/mul/trace.rs:90-180 and
// 278-384, uint/store_mul/trace.rs:43-72, uint/add/trace.rs:104-215).  The planner (uint_traces_plan.cpp, host only) has validated the
// store and given the heights and every row's bound index.  Two stages with one read-back between them:
//   witness  ut_self             a lane per store row: one UintVal read of its bound (integer atomic on the bound's counter, added
//                                once per wave where the lanes agree: ut_count).
//            ut_mul_witness      a lane per multiply relation: the five pointers by binary search, the 544-bit numerator
//                                kappa_a a b +- kappa_c c from 32-bit limb products, its quotient and remainder by bound + 1 (a restoring
//                                shift-subtract division: no digit estimate, hence no correction step and no case split for a modulus of
//                                2^256, 1, 2 or one with 255 leading zeros), the borrow, then the 32 coefficients of the identity's
//                                polynomial in 16-bit limbs and the carry chain of its division by X - 2^16 -- in the same lane, a
//                                coefficient consumed as soon as it is formed.  Leaves a 192-byte record (quotient, borrow, 31 offset
//                                carries, the five row indices) and counts its reads.
//            ut_add_witness      a lane per addition: the four pointers, k, the identity in 288 bits; a 32-byte record (indices, k).
//            Defects (kinds 8..14) go into one packed 64-bit minimum: kind, section, index, operand, from the top.  The chain is the
//            division's self-check: an inexact step or a last coefficient that does not cancel is reported as kind 10.
//   rows     after the minimum has been read back clean and the traces are allocated: ut_usm_row, a lane per row of the 44-column
//            trace (store half: value, complement, carries, gap and the two multiplicities from the finished counters, recomputed by each
//            of a block's four lanes; multiply half: the record and the operands' rows), and ut_add_row, a lane per row of the adder's.
//            Consecutive lanes hold consecutive rows of a column: every store is coalesced.
// All limb arrays are indexed by compile-time constants (the division unrolls over the numerator's 17 limbs and loops over the bits of
// the one in hand).  The counters and the minimum are scratch that the call clears itself; every cell of both traces has exactly one
// writer: a second call leaves the same bytes.
// The bodies named above are in uint_traces_rows.cuh; their kernels are ledger_stage.cuh's lane_per_record<body> and lane_per_row<body>,
// as the defect word, its read-back and the refusal's message are.
#include "section_out.cuh"
#include "uint_traces_rows.cuh"
#include <vector>

static_assert(sizeof(mh_uint_row) == 48, "mh_uint_row is 48 bytes");
static_assert(sizeof(mh_uint_mul_op) == 40, "mh_uint_mul_op is 40 bytes");
static_assert(sizeof(mh_uint_add_op) == 32, "mh_uint_add_op is 32 bytes");
static_assert(sizeof(mh_uint_traces_info) == 80, "mh_uint_traces_info is 80 bytes");

namespace {
const char* const UT_WHAT[] = {"",
                               "a null pointer where a count is nonzero",
                               "more than 2^24 rows in a trace, or padding pointers reaching 2^32",
                               "the trace does not fit log_usm / log_add (index: rows needed)",
                               "a store ptr that is 0 or not above the one before",
                               "a gap to the next ptr of 2^16 or more",
                               "a bound_ptr that is not stored",
                               "a value above its bound's",
                               "a relation's pointer that is not stored",
                               "a kappa of 2^16 or more",
                               "r is not the canonical remainder / a + b is not c + k (bound + 1) for k in {0, 1}",
                               "a quotient of 2^272 or more",
                               "a subtractive underflow beyond two moduli",
                               "a carry outside the +-2^31 window",
                               "nz with b = 0"};

[[noreturn]] void ut_refuse(const mh_uint_traces_info* info) {
  ledger_refuse("mh_uint_traces_build", {info->defect_kind, info->defect_section, info->defect_index, info->defect_operand}, UT_WHAT[info->defect_kind]);
}
}  // namespace

extern "C" int mh_uint_traces_build(mh_ctx* c, const mh_uint_row* rows, size_t n_store, const mh_uint_mul_op* muls, size_t n_mul, const mh_uint_add_op* adds,
                                    size_t n_add, int log_usm, int log_add, mh_trace** usm_out, mh_trace** add_out, mh_uint_traces_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_uint_traces_info local;
  if (!info) info = &local;
  try {
    *info = mh_uint_traces_info{};
    info->n_store = n_store; info->n_mul = n_mul; info->n_add = n_add;
    if (!usm_out || !add_out) {
      info->defect_kind = 1;
      ut_refuse(info);
    }
    std::vector<u32> bound_index(n_store);
    if (mh_uint_traces_plan(rows, n_store, muls, n_mul, adds, n_add, log_usm, log_add, bound_index.data(), info) != MH_OK) ut_refuse(info);
    const u64 usm_rows = info->usm_rows, add_rows = info->add_rows;
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf drows(n_store * sizeof(mh_uint_row)), dbound(n_store * 4), dmuls(n_mul * sizeof(mh_uint_mul_op)), dadds(n_add * sizeof(mh_uint_add_op)),
        dcount(n_store * 8), dmrec(n_mul * UT_MREC * 4), darec(n_add * UT_AREC * 4), ddefect(8);
    c->h2d(drows.p, rows, n_store * sizeof(mh_uint_row));
    c->h2d(dbound.p, bound_index.data(), n_store * 4);
    c->h2d(dmuls.p, muls, n_mul * sizeof(mh_uint_mul_op));
    c->h2d(dadds.p, adds, n_add * sizeof(mh_uint_add_op));
    if (n_store) HIP_CHECK(hipMemsetAsync(dcount.p, 0, n_store * 8, c->stream));
    HIP_CHECK(hipMemsetAsync(ddefect.p, 0xff, 8, c->stream));
    const UtLists L{(const mh_uint_row*)drows.p, (const u32*)dbound.p, (const mh_uint_mul_op*)dmuls.p, (const mh_uint_add_op*)dadds.p,
                    (u32)n_store, (u32)n_mul, (u32)n_add, (u32*)dcount.p, (u32*)dmrec.p, (u32*)darec.p, (unsigned long long*)ddefect.p};
    if (n_store) {
      ProfScope ps(c, "ut_self", 12.0 * (double)n_store);
      launch_per_record<UtLists, &UtLists::n_store, ut_self, UT_ROWS_BT>(c, L);
    }
    if (n_mul) {
      ProfScope ps(c, "ut_mul_witness", (double)n_mul * (sizeof(mh_uint_mul_op) + 5 * 32.0 + 4.0 * UT_MREC));
      launch_per_record<UtLists, &UtLists::n_mul, ut_mul_witness, UT_WITNESS_BT>(c, L);
    }
    if (n_add) {
      ProfScope ps(c, "ut_add_witness", (double)n_add * (sizeof(mh_uint_add_op) + 4 * 32.0 + 4.0 * UT_AREC));
      launch_per_record<UtLists, &UtLists::n_add, ut_add_witness, UT_WITNESS_BT>(c, L);
    }
    const LedgerDefect d = ledger_read_defect(c, ddefect.p, 8, 14, "mh_uint_traces_build", "witness");
    if (d.kind) {
      info->defect_kind = d.kind; info->defect_section = d.section; info->defect_index = d.index; info->defect_operand = d.operand;
      ut_refuse(info);
    }
    std::unique_ptr<mh_trace> usm = trace_new(c, ceil_log2(usm_rows), UT_USM_WIDTH), add = trace_new(c, ceil_log2(add_rows), UT_ADD_WIDTH);
    {
      ProfScope ps(c, "ut_usm_rows", 8.0 * UT_USM_WIDTH * (double)usm_rows);
      launch_per_row<UtLists, ut_usm_row, UT_ROWS_BT>(c, L, usm_rows, usm->cols.u());
    }
    {
      ProfScope ps(c, "ut_add_rows", 8.0 * UT_ADD_WIDTH * (double)add_rows);
      launch_per_row<UtLists, ut_add_row, UT_ROWS_BT>(c, L, add_rows, add->cols.u());
    }
    // the lists and records are pooled buffers: they go back to the pool when this scope ends, ordered behind the row kernels on the stream
    *usm_out = usm.release();
    *add_out = add.release();
    return MH_OK;
  }
  SEC_CATCH
}
