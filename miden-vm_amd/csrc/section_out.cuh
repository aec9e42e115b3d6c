// Where a chiplet section's rows go (bitwise_section.hip, ace_section.hip, kernel_rom_section.hip): a column-major matrix, either the
// section's own trace (prefix < 0) or the width-22 chiplets trace, where the section's selector prefix is `prefix` ones and a zero in
// columns 0 .. prefix and the payload starts at column prefix + 1 (processor/src/trace/utils.rs: ChipletTraceFragment).
#pragma once
#include "../../include/midenhip.h"
#include "ctx.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include <memory>
#include <string>

namespace {
constexpr size_t SEC_CHIPLETS_WIDTH = 22;
constexpr u64 SEC_MAX_ROWS = (u64)1 << 24;

struct SecOut {
  u64* base;   // column 0, row 0 of the matrix written into
  u64 height;  // its rows
  u64 row0;    // first row of the section
  u32 col0;    // first payload column
  int prefix;  // chiplets trace: columns 0 .. prefix - 1 := 1, column prefix := 0; < 0: no selectors
};

// row r of the section: `W` payload cells, then the selector prefix.  Consecutive lanes hold consecutive r: every store is coalesced
template <int W>
__device__ __forceinline__ void sec_store_row(const SecOut& o, u64 r, const u64 (&row)[W]) {
  u64* cell = o.base + (size_t)o.col0 * o.height + o.row0 + r;
#pragma unroll
  for (int i = 0; i < W; i++) cell[(size_t)i * o.height] = row[i];
  if (o.prefix >= 0) {
    u64* sel = o.base + o.row0 + r;
    for (int i = 0; i < o.prefix; i++) sel[(size_t)i * o.height] = 1;
    sel[(size_t)o.prefix * o.height] = 0;
  }
}

inline unsigned sec_grid(u64 n, u64 per_block) { return (unsigned)((n + per_block - 1) / per_block); }

inline int sec_log_n(u64 rows) {  // max(6, ceil log2 rows)
  int l = 6;
  while (((u64)1 << l) < rows) l++;
  return l;
}

// a fresh trace of `width` columns whose rows [n_rows, 2^log_n) are zero; rows [0, n_rows) are the caller's to write
inline std::unique_ptr<mh_trace> sec_new_trace(mh_ctx* c, int log_n, size_t width, u64 n_rows) {
  const u64 height = (u64)1 << log_n;
  std::unique_ptr<mh_trace> t = trace_new(c, log_n, width);
  if (n_rows < height) HIP_CHECK(hipMemset2DAsync(t->cols.u() + n_rows, height * 8, 0, (height - n_rows) * 8, width, c->stream));
  return t;
}

// the checks every in-place entry makes of its target
inline void sec_require_chiplets(mh_ctx* c, const mh_trace* chiplets, const char* entry) {
  MH_REQUIRE(chiplets, std::string(entry) + ": null argument");
  MH_REQUIRE(chiplets->ctx == c, std::string(entry) + ": the chiplets trace belongs to another context");
  MH_REQUIRE(chiplets->width == SEC_CHIPLETS_WIDTH, std::string(entry) + ": the chiplets trace is 22 columns wide");
  MH_REQUIRE(chiplets->log_n >= 0 && chiplets->log_n <= 32, std::string(entry) + ": bad chiplets height");
}
}  // namespace

#define SEC_CATCH                   \
  catch (const MhError& e) {        \
    c->err = e.what();              \
    return e.code;                  \
  }                                 \
  catch (const std::exception& e) { \
    c->err = e.what();              \
    return MH_ERR_INTERNAL;         \
  }
