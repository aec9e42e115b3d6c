// What the planners of the ledger trace builders share (uint_traces_plan.cpp, ec_traces_plan.cpp, transcript_traces_plan.cpp): host
// only.  A planner looks for defects kind by kind and returns the first; its info struct names the defect.
#pragma once
#include "../../include/midenhip.h"

namespace {
constexpr uint64_t PLAN_MAX_ROWS = (uint64_t)1 << 24;  // no trace is taller, so no log_* is above 24

template <class Info>
int plan_defect(Info* info, int kind, uint64_t index, int operand = 0) {
  info->defect_kind = kind;
  info->defect_index = index;
  info->defect_operand = operand;
  return MH_ERR_INVALID;
}

// for a builder of several traces: `section` says which list or trace
template <class Info>
int plan_defect_in(Info* info, int section, int kind, uint64_t index, int operand = 0) {
  info->defect_section = section;
  return plan_defect(info, kind, index, operand);
}

inline uint64_t pow2_at_least(uint64_t v, uint64_t least) {  // the least power of two >= max(least, v), `least` one itself; v stays far below 2^63
  uint64_t p = least;
  while (p < v) p <<= 1;
  return p;
}

// One trace's height from log_n <= 24 (the caller has refused a larger one): 2^log_n, or the rows needed where it is -1.
// -> false where log_n is below -1 or the trace does not fit; *rows is written either way.
inline bool plan_height(int log_n, uint64_t rows_needed, uint64_t* rows) {
  *rows = log_n >= 0 ? (uint64_t)1 << log_n : rows_needed;
  return log_n >= -1 && *rows >= rows_needed;
}
}  // namespace
