// The device stage every ledger trace builder shares (uint_traces.hip, ec_traces.hip, transcript_traces.hip and their *_rows.cuh):
// a checking pass with a lane per record reports the lowest defect through ONE packed 64-bit minimum, one read-back waits for it, and
// row writers with a lane per trace row follow.  Here are the defect word (packed by the bodies, unpacked by the builders and by the
// host runners under tools/), its read-back, the refusal's message and the two lane kernels.
#pragma once
#include "ctx.hpp"
#include "gl.cuh"

namespace {
// ---- the defect word: kind at bit 56, section at bit 54, index at bit 8, operand in the low 8 bits; all ones: no defect ----
struct LedgerDefect {
  int kind;     // 0: none
  int section;  // a builder without sections reports 0 and passes -1 to ledger_refuse
  u64 index;
  int operand;
};

GL_HD void ledger_report(unsigned long long* defect, int kind, int section, u32 index, int operand) {
  const unsigned long long key = ((unsigned long long)kind << 56) | ((unsigned long long)section << 54) | ((unsigned long long)index << 8) | (unsigned long long)operand;
#ifdef __HIP_DEVICE_COMPILE__
  atomicMin(defect, key);
#else
  if (key < *defect) *defect = key;
#endif
}

inline LedgerDefect ledger_unpack(unsigned long long defect) {
  if (defect == ~0ull) return LedgerDefect{0, 0, 0, 0};
  return LedgerDefect{(int)(defect >> 56), (int)((defect >> 54) & 3), (defect >> 8) & 0xffffffffull, (int)(defect & 0xff)};
}

// The one wait of a build: nothing is allocated for the traces before the pass (`pass`: "checking", "witness") is known clean.
inline LedgerDefect ledger_read_defect(mh_ctx* c, const void* device_word, int first_kind, int last_kind, const char* entry, const char* pass) {
  unsigned long long defect = 0;
  c->d2h(&defect, device_word, 8);
  const LedgerDefect d = ledger_unpack(defect);
  MH_REQUIRE(defect == ~0ull || (d.kind >= first_kind && d.kind <= last_kind), std::string(entry) + ": the " + pass + " pass left an unreadable defect word");
  return d;
}

// "<entry>: section S, defect K, index I, operand O: <what>", without the section where it is negative
[[noreturn]] inline void ledger_refuse(const char* entry, const LedgerDefect& d, const char* what) {
  char where[32] = "";
  if (d.section >= 0) snprintf(where, sizeof where, "section %d, ", d.section);
  char buf[400];
  snprintf(buf, sizeof buf, "%s: %sdefect %d, index %llu, operand %d: %s", entry, where, d.kind, (unsigned long long)d.index, d.operand, what);
  throw MhError(MH_ERR_INVALID, buf);
}
}  // namespace

// ---- the lane kernels: `Body` is a host-device function of a *_rows.cuh, inlined; the kernel's name carries the body's ----
// a lane per record: `Count` is the member of the lists that says how many
template <class Lists, u32 Lists::*Count, void (*Body)(const Lists&, u32), int BT>
__global__ __launch_bounds__(BT) void lane_per_record(Lists L) {
  const u32 i = blockIdx.x * BT + threadIdx.x;
  if (i < L.*Count) Body(L, i);
}

// a lane per trace row, padding included
template <class Lists, void (*Body)(const Lists&, u64, u64*, u64), int BT>
__global__ __launch_bounds__(BT) void lane_per_row(Lists L, u64 n, u64* __restrict__ out) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t < n) Body(L, n, out, t);
}

namespace {
template <class Lists, u32 Lists::*Count, void (*Body)(const Lists&, u32), int BT>
void launch_per_record(mh_ctx* c, const Lists& L) {
  MH_LAUNCH((lane_per_record<Lists, Count, Body, BT>), dim3((L.*Count + BT - 1) / BT), dim3(BT), 0, c->stream, L);
}

template <class Lists, void (*Body)(const Lists&, u64, u64*, u64), int BT>
void launch_per_row(mh_ctx* c, const Lists& L, u64 n, u64* out) {
  MH_LAUNCH((lane_per_row<Lists, Body, BT>), dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, c->stream, L, n, out);
}
}  // namespace
