// Host memory safety of the Poseidon2 chiplet's planner (mh_poseidon2_chiplet_plan, csrc/poseidon2_chiplet_plan.cpp): a stand-alone
// program, built with -fsanitize=address,undefined (make -C tools asan_poseidon2_chiplet_plan_run), no GPU, no Python.
// It feeds the planner  (1) random well-formed ledgers, whose starts and levels must equal a restatement written here,  (2) the same
// ledgers with one defect of every kind, which must be refused with that kind and index, and  (3) hostile lists: counts that wrap,
// n_cycles far from the sum, references of any 64-bit value -- in heap blocks of exactly the stated sizes, so that a read past a list
// is an error of the sanitizer.  Exit code 0 and "clean" only if all of that holds.
#include "asan_common.hpp"
#include "../include/midenhip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(4242);
// heap copies of exactly the stated sizes
static int plan(const std::vector<mh_p2c_absorption>& abs, const std::vector<int64_t>* refs, size_t n_cycles, std::vector<uint64_t>& start,
                std::vector<uint32_t>& level, mh_p2c_info& info) {
  Exact<mh_p2c_absorption> a(abs);
  std::vector<int64_t> none;
  Exact<int64_t> r(refs ? *refs : none);
  start.assign(abs.size(), 0);
  level.assign(abs.size(), 0);
  Exact<uint64_t> s(start);
  Exact<uint32_t> l(level);
  const int rc = mh_poseidon2_chiplet_plan(a.p, abs.size(), refs ? r.p : nullptr, n_cycles, s.p, l.p, &info);
  if (s.p) memcpy(start.data(), s.p, start.size() * 8);
  if (l.p) memcpy(level.data(), l.p, level.size() * 4);
  return rc;
}

int main() {
  for (int trial = 0; trial < 2000; trial++) {
    const size_t n_abs = rng() % 24;
    std::vector<mh_p2c_absorption> abs(n_abs);
    std::vector<uint64_t> exp_start;
    size_t total = 0;
    for (auto& a : abs) {
      a = mh_p2c_absorption{{rng(), rng(), rng(), rng()}, 1 + rng() % 5, rng(), rng()};
      exp_start.push_back(total);
      total += a.n_blocks;
    }
    std::vector<int64_t> refs(2 * total, -1);
    std::vector<uint32_t> exp_level(n_abs, 0);
    for (size_t i = 0; i < n_abs; i++)
      for (size_t c = exp_start[i]; c < exp_start[i] + abs[i].n_blocks; c++)
        for (int h = 0; h < 2; h++)
          if (i && rng() % 3 == 0) {
            const size_t r = rng() % i;
            refs[2 * c + h] = (int64_t)r;
            if (exp_level[r] + 1 > exp_level[i]) exp_level[i] = exp_level[r] + 1;
          }
    std::vector<uint64_t> start;
    std::vector<uint32_t> level;
    mh_p2c_info info;
    EXPECT(plan(abs, &refs, total, start, level, info) == MH_OK && info.defect_kind == 0, "a well-formed ledger is taken");
    EXPECT(start == exp_start && level == exp_level, "starts and levels are the restated ones");
    uint64_t rows = 16;
    while (rows < 16 * (uint64_t)total) rows <<= 1;
    EXPECT(info.rows_needed == rows && ((uint64_t)1 << info.log_n) == rows && info.n_cycles == total && info.n_absorptions == n_abs, "sizes");
    if (!n_abs) continue;
    // one defect of each kind
    {
      auto bad = abs;
      const size_t at = rng() % n_abs;
      bad[at].n_blocks = 0;
      EXPECT(plan(bad, &refs, total, start, level, info) == MH_ERR_INVALID && info.defect_kind == 2 && info.defect_index == at, "kind 2");
    }
    {
      const size_t cut = rng() % total;  // fewer cycles than the sum: the first absorption that runs past
      size_t at = 0;
      while (exp_start[at] + abs[at].n_blocks <= cut) at++;
      std::vector<int64_t> shorter(refs.begin(), refs.begin() + 2 * cut);
      EXPECT(plan(abs, &shorter, cut, start, level, info) == MH_ERR_INVALID && info.defect_kind == 3 && info.defect_index == at, "kind 3, past");
      std::vector<int64_t> longer(refs);
      longer.resize(2 * (total + 3), -1);
      EXPECT(plan(abs, &longer, total + 3, start, level, info) == MH_ERR_INVALID && info.defect_kind == 3 && info.defect_index == n_abs, "kind 3, short");
    }
    {
      auto bad = refs;
      const size_t at = rng() % bad.size();
      size_t owner = 0;
      while (exp_start[owner] + abs[owner].n_blocks <= at / 2) owner++;
      const int64_t hostile[] = {(int64_t)owner, (int64_t)owner + 1 + (int64_t)(rng() % 1000), -2, INT64_MIN, INT64_MAX, (int64_t)rng() | INT64_MIN,
                                 (int64_t)(rng() >> 1) | ((int64_t)1 << 40)};
      bad[at] = hostile[rng() % 7];
      size_t first = at;  // an earlier reference of the ledger stays well-formed: the defect is the lowest index
      EXPECT(plan(abs, &bad, total, start, level, info) == MH_ERR_INVALID && info.defect_kind == 4 && info.defect_index == first, "kind 4");
    }
    {
      auto bad = abs;  // counts whose sum wraps 64 bits
      bad[rng() % n_abs].n_blocks = ~(uint64_t)0 - rng() % 3;
      bad.push_back(mh_p2c_absorption{{0, 0, 0, 0}, ~(uint64_t)0, 0, 0});
      EXPECT(plan(bad, &refs, total, start, level, info) == MH_ERR_INVALID && info.defect_kind == 3, "wrapping counts are kind 3");
    }
    {
      std::vector<int64_t> wild(refs.size());  // references of any value
      for (auto& r : wild) r = (int64_t)rng();
      const int rc = plan(abs, &wild, total, start, level, info);
      EXPECT(rc == MH_ERR_INVALID && info.defect_kind == 4, "wild references are refused");
    }
  }
  {
    std::vector<mh_p2c_absorption> big{mh_p2c_absorption{{0, 0, 0, 0}, ((uint64_t)1 << 20) + 1, 0, 0}};
    std::vector<uint64_t> start;
    std::vector<uint32_t> level;
    mh_p2c_info info;
    EXPECT(plan(big, nullptr, ((size_t)1 << 20) + 1, start, level, info) == MH_ERR_INVALID && info.defect_kind == 5, "kind 5");
    EXPECT(mh_poseidon2_chiplet_plan(nullptr, 2, nullptr, 2, nullptr, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1, "kind 1");
    EXPECT(mh_poseidon2_chiplet_plan(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) == MH_ERR_INVALID, "no info");
    EXPECT(mh_poseidon2_chiplet_plan(nullptr, 0, nullptr, 0, nullptr, nullptr, &info) == MH_OK && info.rows_needed == 16 && info.n_levels == 0, "empty");
  }
  return verdict("asan_poseidon2_chiplet_plan");
}
