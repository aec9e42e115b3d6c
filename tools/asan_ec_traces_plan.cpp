// Host memory safety of the EC traces' planner (mh_ec_traces_plan, csrc/ec_traces_plan.cpp): a stand-alone program, built with
// -fsanitize=address,undefined (make -C tools asan_ec_traces_plan_run), no GPU, no Python.
// It feeds the planner  (1) random well-formed lists, whose heights and first rows must equal a restatement written here,  (2) the same
// lists with one defect of every kind 1..7, which must be refused with that kind, section, index and operand, and  (3) hostile lists:
// every field any 32-bit value, n_rows that sum to anything, counts above the row limit with no list behind them, every log from -3 to
// 40 -- in heap blocks of exactly the stated sizes, so that a read past a list is an error of the sanitizer.  Exit code 0 and "clean"
// only if all of that holds.
#include "asan_common.hpp"
#include "../include/midenhip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(4242);
struct Lists {
  std::vector<mh_ec_group> groups;
  std::vector<mh_ec_point> points;
  std::vector<mh_ec_add_op> adds;
  std::vector<mh_msm_expr> exprs;
  std::vector<mh_msm_term> terms;
};

static int plan(const Lists& l, const int (&logs)[4], std::vector<uint32_t>* row_start, mh_ec_traces_info& info) {
  Exact<mh_ec_group> g(l.groups);
  Exact<mh_ec_point> p(l.points);
  Exact<mh_ec_add_op> a(l.adds);
  Exact<mh_msm_expr> e(l.exprs);
  Exact<mh_msm_term> t(l.terms);
  std::vector<uint32_t> rs(l.exprs.size(), 0xdeadbeefu);
  Exact<uint32_t> r(rs);
  const int rc = mh_ec_traces_plan(g.p, l.groups.size(), p.p, l.points.size(), a.p, l.adds.size(), e.p, l.exprs.size(), t.p, l.terms.size(), logs[0], logs[1],
                                   logs[2], logs[3], row_start ? r.p : nullptr, &info);
  if (row_start) {
    if (r.p) memcpy(rs.data(), r.p, rs.size() * 4);
    *row_start = rs;
  }
  return rc;
}

static const int LEAST[4] = {-1, -1, -1, -1};

// lists the planner accepts: groups, points of the three kinds, additions of any content (theirs is the device's to judge), expressions
// whose operands are earlier ones and whose n_rows sum to the terms
static Lists good_lists(size_t n_groups, size_t n_points, size_t n_add, size_t n_exprs) {
  Lists l;
  l.groups.resize(n_groups);
  for (auto& g : l.groups) g = mh_ec_group{(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), rng()};
  l.points.resize(n_groups ? n_points : 0);
  for (auto& p : l.points) {
    const uint32_t kind = (uint32_t)(rng() % 3);
    p = mh_ec_point{1 + (uint32_t)(rng() % n_groups), 0, 0, 0, 0, kind, rng()};
    if (kind != 1) { p.x_ptr = (uint32_t)rng(); p.y_ptr = (uint32_t)rng(); }
    if (kind == 0) { p.u_ptr = (uint32_t)rng(); p.w_ptr = (uint32_t)rng(); }
  }
  l.adds.resize(n_add);
  for (auto& a : l.adds) {
    a = mh_ec_add_op{};
    a.group = (uint32_t)rng(); a.p = (uint32_t)rng(); a.q = (uint32_t)rng(); a.r = (uint32_t)rng(); a.kind = (uint32_t)rng(); a.mints = (uint32_t)rng();
    a.mult = rng();
  }
  l.exprs.resize(n_exprs);
  for (size_t k = 0; k < n_exprs; k++) {
    mh_msm_expr& e = l.exprs[k];
    e = mh_msm_expr{};
    e.kind = k == 0 ? 0 : (uint32_t)(rng() % 3);
    e.group = (uint32_t)rng(); e.val = (uint32_t)rng(); e.neg_minted = (uint32_t)rng(); e.ext_mult = rng(); e.claim_mult = rng();
    e.n_rows = e.kind == 0 ? 1 : 1 + (uint32_t)(rng() % 5);
    if (e.kind != 0) e.a_expr = 1 + (uint32_t)(rng() % k);
    if (e.kind == 1) e.b_expr = 1 + (uint32_t)(rng() % k);
    for (uint32_t r = 0; r < e.n_rows; r++) l.terms.push_back(mh_msm_term{(uint32_t)rng(), (uint32_t)rng()});
  }
  return l;
}

static void expect_refused(const Lists& l, const int (&logs)[4], int section, int kind, uint64_t index, int operand, const char* what) {
  mh_ec_traces_info info;
  std::vector<uint32_t> rs;
  const int rc = plan(l, logs, &rs, info);
  const bool ok = rc == MH_ERR_INVALID && info.defect_section == section && info.defect_kind == kind && info.defect_index == index && info.defect_operand == operand;
  if (!ok)
    fprintf(stderr, "  got rc %d section %d kind %d index %llu operand %d\n", rc, info.defect_section, info.defect_kind, (unsigned long long)info.defect_index,
            info.defect_operand);
  EXPECT(ok, what);
}

int main() {
  // (1) well-formed lists
  for (int round = 0; round < 200; round++) {
    const Lists l = good_lists(1 + rng() % 5, rng() % 300, rng() % 70, rng() % 120);
    mh_ec_traces_info info;
    std::vector<uint32_t> rs;
    EXPECT(plan(l, LEAST, &rs, info) == MH_OK, "a well-formed ledger is accepted");
    EXPECT(info.groups_rows_needed == pow2(l.groups.size(), 2) && info.points_rows_needed == pow2(l.points.size(), 2) &&
               info.add_rows_needed == pow2(4 * (l.adds.empty() ? 1 : l.adds.size()), 4) && info.msm_rows_needed == pow2(l.terms.size(), 2),
           "the heights");
    EXPECT(info.groups_rows == info.groups_rows_needed && info.points_rows == info.points_rows_needed && info.add_rows == info.add_rows_needed &&
               info.msm_rows == info.msm_rows_needed,
           "log -1 takes the least heights");
    uint32_t at = 0;
    bool starts = true;
    for (size_t k = 0; k < l.exprs.size(); k++) {
      starts &= rs[k] == at;
      at += l.exprs[k].n_rows;
    }
    EXPECT(starts && at == l.terms.size(), "the first rows are the prefix sums");
    const int padded[4] = {10, 11, 12, 13};
    EXPECT(plan(l, padded, nullptr, info) == MH_OK && info.groups_rows == 1024 && info.points_rows == 2048 && info.add_rows == 4096 && info.msm_rows == 8192,
           "larger logs pad, row_start may be NULL");
  }
  {
    const Lists none;
    mh_ec_traces_info info;
    EXPECT(plan(none, LEAST, nullptr, info) == MH_OK && info.groups_rows == 2 && info.points_rows == 2 && info.add_rows == 4 && info.msm_rows == 2, "empty lists");
    EXPECT(mh_ec_traces_plan(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, -1, -1, -1, -1, nullptr, nullptr) == MH_ERR_INVALID, "no info");
  }
  // (2) one defect of every kind
  for (int round = 0; round < 50; round++) {
    const Lists l = good_lists(2, 40 + rng() % 40, 9, 30 + rng() % 30);
    mh_ec_traces_info info;
    {  // 1: a NULL list where a count is nonzero (the counts are read, the lists are not)
      Exact<mh_ec_group> g(l.groups);
      EXPECT(mh_ec_traces_plan(g.p, 2, nullptr, 7, nullptr, 0, nullptr, 0, nullptr, 0, -1, -1, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1 &&
                 info.defect_section == 1,
             "kind 1, points");
      EXPECT(mh_ec_traces_plan(g.p, 2, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 5, -1, -1, -1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 1 &&
                 info.defect_section == 3 && info.defect_operand == 1,
             "kind 1, terms");
    }
    {  // 2: counts above the limit are refused before anything behind them is read; a log above 24
      Exact<mh_ec_add_op> a(l.adds);
      EXPECT(mh_ec_traces_plan(nullptr, 0, nullptr, 0, a.p, ((size_t)1 << 22) + 1, nullptr, 0, nullptr, 0, -1, -1, -1, -1, nullptr, &info) == MH_ERR_INVALID &&
                 info.defect_kind == 2 && info.defect_section == 2,
             "kind 2, additions");
      const int big[4] = {-1, 25, -1, -1};
      expect_refused(l, big, 1, 2, 25, 0, "kind 2, a log of 25");
    }
    {
      const int small[4] = {-1, -1, -1, 2};
      expect_refused(l, small, 3, 3, pow2(l.terms.size(), 2), 0, "kind 3, log_msm below the need");
      const int negative[4] = {-2, -1, -1, -1};
      expect_refused(l, negative, 0, 3, 2, 0, "kind 3, a log below -1");
    }
    const size_t pi = rng() % l.points.size();
    { Lists d = l; d.points[pi].group = rng() % 2 ? 0 : 3; expect_refused(d, LEAST, 1, 4, pi, 0, "kind 4"); }
    { Lists d = l; d.points[pi].kind = 3 + (uint32_t)(rng() % 100); expect_refused(d, LEAST, 1, 5, pi, 0, "kind 5, the kind"); }
    { Lists d = l; d.points[pi] = mh_ec_point{1, 0, 5, 0, 0, 1, 0}; expect_refused(d, LEAST, 1, 5, pi, 2, "kind 5, a point at infinity with a y"); }
    { Lists d = l; d.points[pi] = mh_ec_point{1, 4, 5, 0, 6, 2, 0}; expect_refused(d, LEAST, 1, 5, pi, 4, "kind 5, a certified point with a w"); }
    const size_t ek = 1 + rng() % (l.exprs.size() - 1);
    { Lists d = l; d.exprs[ek].kind = 3; expect_refused(d, LEAST, 3, 6, ek, 0, "kind 6, the kind"); }
    { Lists d = l; d.exprs[ek].n_rows = 0; expect_refused(d, LEAST, 3, 6, ek, 1, "kind 6, no rows"); }
    { Lists d = l; d.exprs[0].n_rows = 2; expect_refused(d, LEAST, 3, 6, 0, 1, "kind 6, an intro of two rows"); }
    { Lists d = l; d.terms.pop_back(); expect_refused(d, LEAST, 3, 6, d.exprs.size(), 2, "kind 6, the sum"); }
    {
      Lists d = l;
      mh_msm_expr& e = d.exprs[ek];
      const int form = (int)(rng() % 3);
      int operand = 0;
      if (e.kind == 0) { (form ? e.a_expr : e.b_expr) = 1; operand = form ? 0 : 1; }
      else if (form == 0) { e.a_expr = 0; }
      else if (form == 1) { e.a_expr = (uint32_t)ek + 1; }  // itself
      else { e.b_expr = e.kind == 1 ? (uint32_t)ek + 1 + (uint32_t)(rng() % 1000) : 1; operand = 1; }
      expect_refused(d, LEAST, 3, 7, ek, operand, "kind 7");
    }
    {  // two defects: the lower kind
      Lists d = l;
      d.exprs[ek].kind = 7;
      d.points[pi].group = 0;
      expect_refused(d, LEAST, 1, 4, pi, 0, "kind 4 before kind 6");
    }
  }
  // (3) hostile lists: whatever the planner answers, it reads nothing outside the blocks and writes row_start only when it accepts
  for (int round = 0; round < 400; round++) {
    Lists l;
    l.groups.resize(rng() % 4);
    l.points.resize(rng() % 50);
    l.adds.resize(rng() % 20);
    l.exprs.resize(rng() % 40);
    l.terms.resize(rng() % 90);
    for (auto& g : l.groups) g = mh_ec_group{(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), rng()};
    for (auto& p : l.points) p = mh_ec_point{(uint32_t)(rng() % 6), (uint32_t)(rng() % 2), (uint32_t)(rng() % 2), (uint32_t)(rng() % 2), (uint32_t)(rng() % 2), (uint32_t)(rng() % 4), rng()};
    for (auto& a : l.adds) { a = mh_ec_add_op{}; a.p = (uint32_t)rng(); a.kind = (uint32_t)rng(); }
    for (auto& e : l.exprs) {
      e = mh_msm_expr{};
      e.kind = (uint32_t)(rng() % 4); e.a_expr = (uint32_t)(rng() % 50); e.b_expr = (uint32_t)(rng() % 50);
      e.n_rows = rng() % 8 ? (uint32_t)(rng() % 4) : (uint32_t)rng();
    }
    for (auto& t : l.terms) t = mh_msm_term{(uint32_t)rng(), (uint32_t)rng()};
    const int logs[4] = {(int)(rng() % 44) - 3, (int)(rng() % 44) - 3, (int)(rng() % 44) - 3, (int)(rng() % 44) - 3};
    mh_ec_traces_info info;
    std::vector<uint32_t> rs;
    const int rc = plan(l, logs, &rs, info);
    EXPECT(rc == MH_OK || (rc == MH_ERR_INVALID && info.defect_kind >= 1 && info.defect_kind <= 7), "a hostile ledger is accepted or refused with a planner kind");
    if (rc != MH_OK)
      for (uint32_t v : rs) EXPECT(v == 0xdeadbeefu, "a refusal writes no first row");
  }
  return verdict("asan_ec_traces_plan");
}
