// The planner of the precompile prover's Poseidon2 chiplet trace (mh_poseidon2_chiplet_plan): host only, no device pass.
//
// Validates the absorption ledger the device stage (poseidon2_chiplet.hip) is about to index with, and gives every absorption its
// start cycle (the n_blocks before it) and its level (0 without a digest reference, else one above the highest level referenced).
// Nothing here hashes.  Defects are looked for kind by kind, the lowest kind first and within it the lowest index; a later kind is
// only looked for once the earlier ones are absent, so every index it computes with is in range:
//   1 a NULL pointer where one is required   2 n_blocks = 0   3 the n_blocks do not add up to n_cycles
//   4 a reference that is neither -1 nor an earlier absorption   5 more than 2^20 cycles
// (6, a log_n below the height, belongs to the build entry.)
#include "../../include/midenhip.h"
#include <vector>

namespace {
constexpr uint64_t P2C_MAX_CYCLES = (uint64_t)1 << 20;  // 2^24 rows

int p2c_defect(mh_p2c_info* info, int kind, uint64_t index) {
  info->defect_kind = kind;
  info->defect_index = index;
  return MH_ERR_INVALID;
}
}  // namespace

extern "C" int mh_poseidon2_chiplet_plan(const mh_p2c_absorption* abs, size_t n_abs, const int64_t* refs, size_t n_cycles, uint64_t* start,
                                         uint32_t* level, mh_p2c_info* info) {
  if (!info) return MH_ERR_INVALID;
  *info = mh_p2c_info{};
  info->n_absorptions = n_abs;
  info->n_cycles = n_cycles;
  if (!abs && n_abs) return p2c_defect(info, 1, 0);
  for (size_t i = 0; i < n_abs; i++)
    if (abs[i].n_blocks == 0) return p2c_defect(info, 2, i);
  uint64_t total = 0;
  for (size_t i = 0; i < n_abs; i++) {
    if (abs[i].n_blocks > (uint64_t)n_cycles - total) return p2c_defect(info, 3, i);  // no sum is formed that could wrap
    total += abs[i].n_blocks;
  }
  if (total != n_cycles) return p2c_defect(info, 3, n_abs);
  if (refs) {
    size_t a = 0;
    uint64_t end = n_abs ? abs[0].n_blocks : 0;  // one past the last cycle of absorption a
    for (size_t c = 0; c < n_cycles; c++) {
      while (c >= end) end += abs[++a].n_blocks;
      for (int h = 0; h < 2; h++) {
        const int64_t r = refs[2 * c + h];
        if (r < -1 || (r >= 0 && (uint64_t)r >= a)) return p2c_defect(info, 4, 2 * (uint64_t)c + h);
      }
    }
  }
  if (n_cycles > P2C_MAX_CYCLES) return p2c_defect(info, 5, n_cycles);
  uint64_t rows = 16;
  while (rows < 16 * (uint64_t)n_cycles) rows <<= 1;
  info->rows_needed = rows;
  while (((uint64_t)1 << info->log_n) < rows) info->log_n++;
  // starts and levels: a reference points below, so one pass in order knows every level it reads
  std::vector<uint32_t> own;
  uint32_t* lv = level;
  if (!lv && refs) {
    own.resize(n_abs);
    lv = own.data();
  }
  uint64_t at = 0, top = 0;
  for (size_t i = 0; i < n_abs; i++) {
    uint32_t l = 0;
    if (refs)
      for (uint64_t c = at; c < at + abs[i].n_blocks; c++)
        for (int h = 0; h < 2; h++) {
          const int64_t r = refs[2 * c + h];
          if (r >= 0 && lv[r] + 1 > l) l = lv[r] + 1;
        }
    if (lv) lv[i] = l;
    if (start) start[i] = at;
    if (l > top) top = l;
    at += abs[i].n_blocks;
  }
  info->n_levels = n_abs ? top + 1 : 0;
  return MH_OK;
}
