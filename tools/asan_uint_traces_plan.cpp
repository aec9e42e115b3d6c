// Host memory safety of the uint traces' planner (mh_uint_traces_plan, csrc/uint_traces_plan.cpp): a stand-alone program, built with
// -fsanitize=address,undefined (make -C tools asan_uint_traces_plan_run), no GPU, no Python.
// It feeds the planner  (1) random well-formed stores, whose heights and bound indices must equal a restatement written here,  (2) the
// same stores with one defect of every kind 1..7, which must be refused with that kind and index, and  (3) hostile lists: pointers of any
// 32-bit value in any order, bounds that point anywhere, counts above the row limit with no list behind them, every log from -3 to 40 --
// in heap blocks of exactly the stated sizes, so that a read past a list is an error of the sanitizer.  Exit code 0 and "clean" only if
// all of that holds.
#include "asan_common.hpp"
#include "../include/midenhip.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(777);
static int plan(const std::vector<mh_uint_row>& rows, size_t n_mul, size_t n_add, int log_usm, int log_add, std::vector<uint32_t>* bound_index,
                mh_uint_traces_info& info) {
  Exact<mh_uint_row> r(rows);
  const std::vector<mh_uint_mul_op> muls(n_mul);
  const std::vector<mh_uint_add_op> adds(n_add);
  Exact<mh_uint_mul_op> m(muls);
  Exact<mh_uint_add_op> a(adds);
  std::vector<uint32_t> bi(rows.size(), 0xdeadbeefu);
  Exact<uint32_t> b(bi);
  const int rc = mh_uint_traces_plan(r.p, rows.size(), m.p, n_mul, a.p, n_add, log_usm, log_add, bound_index ? b.p : nullptr, &info);
  if (bound_index) {
    if (b.p) memcpy(bi.data(), b.p, bi.size() * 4);
    *bound_index = bi;
  }
  return rc;
}

// a well-formed store: a few modulus rows (their own bound), values under them, ascending pointers with gaps below 2^16
static std::vector<mh_uint_row> good_store(size_t n) {
  std::vector<mh_uint_row> rows(n);
  std::vector<size_t> moduli;
  uint32_t ptr = 0;
  for (size_t i = 0; i < n; i++) {
    ptr += 1 + (uint32_t)(rng() % (i % 7 == 0 ? 65536 : 3));
    mh_uint_row& r = rows[i];
    r = mh_uint_row{};
    r.ptr = ptr;
    r.val_reads = (uint32_t)rng();
    r.limb_reads = (uint32_t)rng();
    if (moduli.empty() || rng() % 9 == 0) {
      r.bound_ptr = ptr;
      for (int j = 0; j < 8; j++) r.value[j] = (uint32_t)rng() | (j == 7 ? 0x80000000u : 0);
      moduli.push_back(i);
    } else {
      const mh_uint_row& b = rows[moduli[rng() % moduli.size()]];
      r.bound_ptr = b.ptr;
      const int top = (int)(rng() % 8);  // equal above limb `top`, smaller there: value <= bound
      for (int j = 0; j < 8; j++) r.value[j] = j > top ? b.value[j] : j == top ? (uint32_t)(rng() % ((uint64_t)b.value[j] + 1)) : (uint32_t)rng();
      if (r.value[top] == b.value[top])
        for (int j = 0; j < top; j++) r.value[j] = b.value[j];
    }
  }
  return rows;
}

int main() {
  for (int trial = 0; trial < 1500; trial++) {
    const size_t n = rng() % 60, n_mul = rng() % 40, n_add = rng() % 40;
    std::vector<mh_uint_row> rows = good_store(n);
    // a bound that comes AFTER the rows under it is as good as one before
    if (n > 2 && trial % 3 == 0) {
      mh_uint_row& last = rows[n - 1];
      last.bound_ptr = last.ptr;
      for (int j = 0; j < 8; j++) last.value[j] = 0xffffffffu;
      rows[0].bound_ptr = last.ptr;
    }
    mh_uint_traces_info info;
    std::vector<uint32_t> bi;
    const uint64_t mul_rows = pow2(8 * (n_mul ? n_mul : 1)), usm = 4 * std::max<uint64_t>(pow2(n), mul_rows / 4), add = pow2(2 * (n_add ? n_add : 1));
    EXPECT(plan(rows, n_mul, n_add, -1, -1, &bi, info) == MH_OK, "a well-formed store is taken");
    EXPECT(info.n_store == n && info.n_mul == n_mul && info.n_add == n_add && info.usm_rows_needed == usm && info.usm_rows == usm &&
               info.add_rows_needed == add && info.add_rows == add && info.defect_kind == 0,
           "heights and counts");
    for (size_t i = 0; i < n; i++) EXPECT(bi[i] < n && rows[bi[i]].ptr == rows[i].bound_ptr, "bound index");
    EXPECT(plan(rows, n_mul, n_add, -1, -1, nullptr, info) == MH_OK, "the bound indices may be left out");
    int lu = 0;
    while (((uint64_t)1 << lu) < usm) lu++;
    EXPECT(plan(rows, n_mul, n_add, lu + 2, 20, nullptr, info) == MH_OK && info.usm_rows == 4 * usm && info.add_rows == ((uint64_t)1 << 20), "larger heights pad");
    if (lu > 0) {
      EXPECT(plan(rows, n_mul, n_add, lu - 1, -1, nullptr, info) == MH_ERR_INVALID && info.defect_kind == 3 && info.defect_section == 0 && info.defect_index == usm,
             "kind 3, the 44-column trace");
    }
    EXPECT(plan(rows, n_mul, n_add, -1, 0, nullptr, info) == (add > 1 ? MH_ERR_INVALID : MH_OK) && (add == 1 || (info.defect_kind == 3 && info.defect_section == 2 && info.defect_index == add)),
           "kind 3, the adder");
    if (n < 3) continue;
    // one defect of every store kind, and a later kind behind it that must not come first
    const size_t at = 1 + rng() % (n - 1);
    std::vector<mh_uint_row> bad = rows;
    bad[at].ptr = bad[at - 1].ptr;  // 4: not above the one before
    bad[n - 1].bound_ptr = 0xfffffff0u;
    EXPECT(plan(bad, n_mul, n_add, -1, -1, &bi, info) == MH_ERR_INVALID && info.defect_kind == 4 && info.defect_index == at, "kind 4");
    bad = rows;
    bad[0].ptr = 0;
    EXPECT(plan(bad, n_mul, n_add, -1, -1, &bi, info) == MH_ERR_INVALID && info.defect_kind == 4 && info.defect_index == 0, "kind 4: ptr 0");
    bad = rows;
    for (size_t i = at; i < n; i++) bad[i].ptr += 70000;  // 5: a gap; the bounds still resolve or not -- kind 5 comes first
    if (bad[n - 1].ptr > rows[n - 1].ptr) {
      for (size_t i = 0; i < n; i++)
        for (size_t j = at; j < n; j++)
          if (rows[i].bound_ptr == rows[j].ptr) bad[i].bound_ptr = bad[j].ptr;
      EXPECT(plan(bad, n_mul, n_add, -1, -1, &bi, info) == MH_ERR_INVALID && info.defect_kind == 5 && info.defect_index == at - 1, "kind 5");
    }
    bad = rows;
    size_t victim = n;
    for (size_t i = 0; i < n && victim == n; i++)
      if (rows[i].bound_ptr != rows[i].ptr) victim = i;
    if (victim < n) {
      bad[victim].bound_ptr = rows[n - 1].ptr + 1;  // 6: not a stored pointer
      EXPECT(plan(bad, n_mul, n_add, -1, -1, &bi, info) == MH_ERR_INVALID && info.defect_kind == 6 && info.defect_index == victim, "kind 6");
      bad = rows;
      const mh_uint_row* b = nullptr;
      for (size_t j = 0; j < n; j++)
        if (rows[j].ptr == rows[victim].bound_ptr) b = &rows[j];
      bool all_ones = true;
      for (int j = 0; j < 8; j++) all_ones = all_ones && b->value[j] == 0xffffffffu;
      if (!all_ones) {
        int j = 0;
        for (int k = 0; k < 8; k++) bad[victim].value[k] = b->value[k];
        while (bad[victim].value[j] == 0xffffffffu) bad[victim].value[j++] = 0;
        bad[victim].value[j]++;  // 7: the bound's value + 1
        EXPECT(plan(bad, n_mul, n_add, -1, -1, &bi, info) == MH_ERR_INVALID && info.defect_kind == 7 && info.defect_index == victim, "kind 7");
      }
    }
  }
  // hostile lists: nothing but the stated bytes may be read, whatever they hold
  for (int trial = 0; trial < 3000; trial++) {
    const size_t n = rng() % 40;
    std::vector<mh_uint_row> rows(n);
    for (auto& r : rows) {
      uint32_t w[12];
      for (auto& x : w) x = (rng() % 4 == 0) ? (uint32_t)(rng() % 8) : (uint32_t)rng();
      memcpy(&r, w, sizeof r);
    }
    if (trial % 2) std::sort(rows.begin(), rows.end(), [](const mh_uint_row& x, const mh_uint_row& y) { return x.ptr < y.ptr; });
    mh_uint_traces_info info;
    std::vector<uint32_t> bi;
    const int rc = plan(rows, rng() % 5, rng() % 5, (int)(rng() % 44) - 3, (int)(rng() % 44) - 3, trial % 3 ? &bi : nullptr, info);
    EXPECT(rc == MH_OK || (rc == MH_ERR_INVALID && info.defect_kind >= 1 && info.defect_kind <= 7), "a hostile store is taken or refused by kind");
    EXPECT(info.n_store == n, "the counts are filled either way");
  }
  {
    mh_uint_traces_info info;
    mh_uint_row one{};
    one.ptr = one.bound_ptr = 1;
    EXPECT(mh_uint_traces_plan(nullptr, 3, nullptr, 0, nullptr, 0, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_section == 0, "kind 1: rows");
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 2, nullptr, 0, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_section == 1, "kind 1: muls");
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, nullptr, 2, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_section == 2, "kind 1: adds");
    EXPECT(mh_uint_traces_plan(nullptr, 0, nullptr, 0, nullptr, 0, -1, -1, nullptr, nullptr) == MH_ERR_INVALID, "no info");
    EXPECT(mh_uint_traces_plan(nullptr, 0, nullptr, 0, nullptr, 0, -1, -1, nullptr, &info) == MH_OK && info.usm_rows_needed == 8 && info.add_rows_needed == 2, "empty");
    // counts above the row limit are refused before a list is read: the pointers are one-element blocks
    mh_uint_mul_op mo{};
    mh_uint_add_op ao{};
    EXPECT(mh_uint_traces_plan(&one, ((size_t)1 << 22) + 1, nullptr, 0, nullptr, 0, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2 && info.defect_section == 0, "kind 2: store");
    EXPECT(mh_uint_traces_plan(&one, 1, &mo, ((size_t)1 << 21) + 1, nullptr, 0, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2 && info.defect_section == 1, "kind 2: muls");
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, &ao, ((size_t)1 << 23) + 1, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2 && info.defect_section == 2, "kind 2: adds");
    EXPECT(mh_uint_traces_plan(&one, 1, &mo, (size_t)1 << 21, &ao, (size_t)1 << 23, -1, -1, nullptr, &info) == MH_OK && info.usm_rows_needed == ((uint64_t)1 << 24) &&
               info.add_rows_needed == ((uint64_t)1 << 24),
           "the largest lists are taken");
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, nullptr, 0, 25, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2, "kind 2: log_usm above 24");
    one.ptr = one.bound_ptr = 0xffffffffu;  // one padding block would take pointer 2^32
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, nullptr, 0, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2 && info.defect_section == 0, "kind 2: padding pointers");
    one.ptr = one.bound_ptr = 0xfffffffeu;
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, nullptr, 0, -1, -1, nullptr, &info) == MH_OK, "the last padding pointer may be 2^32 - 1");
    EXPECT(mh_uint_traces_plan(&one, 1, nullptr, 0, nullptr, 0, 4, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 2, "kind 2: padding pointers of a larger height");
  }
  return verdict("asan_uint_traces_plan");
}
