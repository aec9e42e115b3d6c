// Host memory safety of the ChunkNode and TranscriptEval traces' planners (mh_chunk_node_plan, mh_transcript_eval_plan,
// csrc/transcript_traces_plan.cpp): a stand-alone program, built with -fsanitize=address,undefined
// (make -C tools asan_transcript_traces_plan_run), no GPU, no Python.
// It feeds the planners  (1) random well-formed lists, whose heights and first rows must equal a restatement written here,  (2) the same
// lists with one defect of every kind 1..7, which must be refused with that kind, index and operand, and  (3) hostile lists: every field
// any 64-bit value (or one near the limits the planners compare with), kinds and ops anything, spans that wrap, every log from -3 to 40 --
// in heap blocks of exactly the stated sizes, so that a read past a list is an error of the sanitizer.  Neither planner reads through
// `bytes`, `digests` or `limbs`: those are dangling non-null pointers here.  Exit code 0 and "clean" only if all of that holds.
#include "asan_common.hpp"
#include "../include/midenhip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(777);
static const uint8_t* const DANGLING8 = (const uint8_t*)(uintptr_t)0x10;    // never read through
static const uint32_t* const DANGLING32 = (const uint32_t*)(uintptr_t)0x10;

// ---------------------------------------------------------------- ChunkNode ----------------------------------------------------------------
struct Cn {
  std::vector<mh_kn_record> rec;
  uint64_t n_bytes = 0, cycles = 0;
};

static int cn_plan(const Cn& l, int log_n, mh_chunk_node_info& info) {
  Exact<mh_kn_record> r(l.rec);
  return mh_chunk_node_plan(l.n_bytes ? DANGLING8 : nullptr, l.n_bytes, l.rec.empty() ? nullptr : DANGLING8, r.p, l.rec.size(), l.cycles, log_n, &info);
}

static uint64_t chunks_of(uint64_t len) { return len ? (len + 31) / 32 : 1; }

static Cn cn_good(size_t n) {
  Cn l;
  uint64_t head = 0, perm = 0, sponge = 0;
  for (size_t i = 0; i < n; i++) {
    const uint64_t len = rng() % 300;
    mh_kn_record r{l.n_bytes, len, head, sponge, perm, perm + chunks_of(len), perm + chunks_of(len) + 1, 1 + rng() % 3};
    l.rec.push_back(r);
    l.n_bytes += len;
    head += chunks_of(len);
    perm += chunks_of(len) + 2;
    sponge += 32 * (len / 136 + 1);
  }
  l.cycles = perm + rng() % 3;
  return l;
}

static void cn_expect(const Cn& l, int log_n, int kind, uint64_t index, int operand, const char* what) {
  mh_chunk_node_info info;
  const int rc = cn_plan(l, log_n, info);
  EXPECT(rc == MH_ERR_INVALID && info.defect_kind == kind && info.defect_index == index && info.defect_operand == operand, what);
}

static void cn_tests() {
  for (int round = 0; round < 200; round++) {
    const size_t n = round < 3 ? (size_t)round : 1 + rng() % 40;
    const Cn l = cn_good(n);
    uint64_t total = 0;
    for (const mh_kn_record& r : l.rec) total += chunks_of(r.len);
    mh_chunk_node_info info;
    EXPECT(cn_plan(l, -1, info) == MH_OK && info.defect_kind == 0, "a well-formed list is accepted");
    EXPECT(info.rows == pow2(total > n ? total : n, 2) && info.rows_needed == info.rows && info.n_chunks == total && info.n_records == n, "heights");
    EXPECT(cn_plan(l, 24, info) == MH_OK && info.rows == (uint64_t)1 << 24, "a larger log pads");
    if (n == 0) continue;
    const size_t i = rng() % n;
    Cn d = l;
    d.rec[i].len = l.n_bytes - d.rec[i].offset + 1;
    cn_expect(d, -1, 2, i, 0, "len past the bytes");
    d = l;
    d.rec[i].offset = ~0ull - rng() % 4;
    d.rec[i].len = 1 + rng() % 8;
    cn_expect(d, -1, 2, i, 0, "offset + len wraps");
    d = l;
    d.rec[i].chunk_head += 1;
    cn_expect(d, -1, 3, i, 0, "chunk_head");
    d = l;
    d.rec[i].sponge_head += 1 + rng() % 31;
    cn_expect(d, -1, 4, i, 0, "sponge_head");
    d = l;
    d.rec[i].perm_chunks = l.cycles - chunks_of(d.rec[i].len) + 1;
    cn_expect(d, -1, 5, i, 0, "the chain runs past the cycles");
    d = l;
    d.rec[i].perm_chunks = ~0ull;
    cn_expect(d, -1, 5, i, 0, "the chain's span wraps");
    d = l;
    d.rec[i].perm_digest_chunks = l.cycles;
    cn_expect(d, -1, 5, i, 1, "perm_digest_chunks");
    d = l;
    d.rec[i].perm_keccak = l.cycles + rng();
    if (d.rec[i].perm_keccak >= l.cycles) cn_expect(d, -1, 5, i, 2, "perm_keccak");
    const int high = 25 + (int)(rng() % 10);
    cn_expect(l, high, 6, (uint64_t)high, 0, "a log above 24");
    mh_chunk_node_info need;
    cn_plan(l, -1, need);
    int least = 0;
    while (((uint64_t)1 << least) < need.rows) least++;
    cn_expect(l, least - 1, 7, need.rows, 0, "a log below the need");
    cn_expect(l, -2 - (int)(rng() % 3), 7, need.rows, 0, "a log below -1");
  }
  {  // NULL pointers
    Cn l = cn_good(3);
    Exact<mh_kn_record> r(l.rec);
    mh_chunk_node_info info;
    EXPECT(mh_chunk_node_plan(nullptr, l.n_bytes, DANGLING8, r.p, 3, l.cycles, -1, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_operand == 0, "bytes");
    EXPECT(mh_chunk_node_plan(DANGLING8, l.n_bytes, nullptr, r.p, 3, l.cycles, -1, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_operand == 1, "digests");
    EXPECT(mh_chunk_node_plan(DANGLING8, l.n_bytes, DANGLING8, nullptr, 3, l.cycles, -1, &info) == MH_ERR_INVALID && info.defect_kind == 1 && info.defect_operand == 2, "records");
    EXPECT(mh_chunk_node_plan(DANGLING8, l.n_bytes, DANGLING8, r.p, 3, l.cycles, -1, nullptr) == MH_ERR_INVALID, "info");
  }
  {  // more than 2^24 rows through one record: a message of 32 (2^24 + 1) bytes (the bytes are not read)
    Cn l;
    const uint64_t len = 32 * (((uint64_t)1 << 24) + 1);
    l.rec.push_back(mh_kn_record{0, len, 0, 0, 0, 1, 2, 1});
    l.n_bytes = len;
    l.cycles = ~0ull;
    cn_expect(l, -1, 6, ((uint64_t)1 << 24) + 1, 0, "too many rows");
  }
  const uint64_t edges[] = {0, 1, 31, 32, 33, 135, 136, 137, (uint64_t)1 << 24, ((uint64_t)1 << 24) + 1, (uint64_t)1 << 32, (uint64_t)1 << 62, (uint64_t)1 << 63,
                            ~0ull - 32, ~0ull - 1, ~0ull};
  auto word = [&]() { return rng() % 3 ? edges[rng() % (sizeof edges / sizeof *edges)] : rng(); };
  for (int round = 0; round < 3000; round++) {  // hostile: whatever comes back, no read leaves the list
    Cn l;
    const size_t n = rng() % 12;
    for (size_t i = 0; i < n; i++) l.rec.push_back(mh_kn_record{word(), word(), rng() % 4 ? (uint64_t)i : word(), word(), word(), word(), word(), word()});
    l.n_bytes = word();
    l.cycles = word();
    mh_chunk_node_info info;
    const int rc = cn_plan(l, (int)(rng() % 44) - 3, info);
    EXPECT((rc == MH_OK) == (info.defect_kind == 0) && (rc == MH_OK || rc == MH_ERR_INVALID), "an answer");
    if (rc == MH_OK) EXPECT(info.rows <= (uint64_t)1 << 24 && info.rows >= info.rows_needed && info.n_chunks <= info.rows, "an accepted hostile list fits");
  }
}

// ---------------------------------------------------------------- TranscriptEval ----------------------------------------------------------------
struct Te {
  std::vector<mh_te_node> nodes;
  std::vector<mh_te_term> terms;
  uint64_t n_lit = 0, root = 0, cycles = 0;
};

static int te_plan(const Te& l, int log_n, std::vector<uint32_t>* row_start, mh_transcript_eval_info& info) {
  Exact<mh_te_node> n(l.nodes);
  Exact<mh_te_term> t(l.terms);
  std::vector<uint32_t> rs(l.nodes.size(), 0xdeadbeefu);
  Exact<uint32_t> r(rs);
  const int rc = mh_transcript_eval_plan(n.p, l.nodes.size(), t.p, l.terms.size(), l.n_lit ? DANGLING32 : nullptr, l.n_lit, l.root, l.cycles, log_n,
                                         row_start ? r.p : nullptr, &info);
  if (row_start) {
    if (r.p) memcpy(rs.data(), r.p, rs.size() * 4);
    *row_start = rs;
  }
  return rc;
}

// nodes the planner accepts: leaves, ops over earlier nodes of any class (the class is the device's to judge), MSM claims, ZEROs and a
// fold of ANDs whose last is the root
static Te te_good(size_t n_values) {
  Te l;
  uint64_t perm = 0;
  l.n_lit = 1 + rng() % 5;
  auto push = [&](uint32_t kind, uint32_t op, int64_t lhs, int64_t rhs, uint64_t span) {
    l.nodes.push_back(mh_te_node{kind, op, lhs, rhs, perm, rng() % 1000, rng() % 10, rng() % 3, rng() % 7});
    perm += span;
  };
  push(2, 0, (int64_t)(rng() % l.n_lit), 0, 1);
  for (size_t i = 0; i < n_values; i++) {
    const size_t own = l.nodes.size();
    const int64_t a = (int64_t)(rng() % own), b = (int64_t)(rng() % own);
    switch (rng() % 7) {
      case 0: push(2, 0, (int64_t)(rng() % l.n_lit), 0, 1); break;
      case 1: push(3, 0, (int64_t)(rng() % l.n_lit), 0, 1); break;
      case 2: push(4, 1 + (uint32_t)(rng() % 4), a, b, 1); break;
      case 3: push(5, 0, a, b, 1); break;
      case 4: push(6, 0, 0, 0, 1); break;
      case 5: push(7, 1 + (uint32_t)(rng() % 3), a, b, 1); break;
      default: {
        const uint64_t k = 1 + rng() % 5;
        const int64_t start = (int64_t)l.terms.size();
        for (uint64_t t = 0; t < k; t++) l.terms.push_back(mh_te_term{(uint32_t)(rng() % own), (uint32_t)(rng() % own)});
        push(8, 0, start, (int64_t)k, k);
      }
    }
  }
  const size_t zeros = rng() % 4;
  for (size_t z = 0; z < zeros; z++) push(0, 0, 0, 0, 0);
  const size_t ands = 1 + rng() % 4;
  l.cycles = perm + ands + 1 + rng() % 3;
  for (size_t a = 0; a < ands; a++) push(1, 0, (int64_t)(rng() % l.nodes.size()), -1 - (int64_t)(rng() % l.cycles), 1);
  l.root = l.nodes.size() - 1;
  return l;
}

static void te_expect(const Te& l, int log_n, int kind, uint64_t index, int operand, const char* what) {
  mh_transcript_eval_info info;
  const int rc = te_plan(l, log_n, nullptr, info);
  EXPECT(rc == MH_ERR_INVALID && info.defect_kind == kind && info.defect_index == index && info.defect_operand == operand, what);
}

static size_t find_kind(const Te& l, uint32_t kind) {
  for (size_t i = 0; i < l.nodes.size(); i++)
    if (l.nodes[i].kind == kind) return i;
  return l.nodes.size();
}

static void te_tests() {
  for (int round = 0; round < 300; round++) {
    const Te l = te_good(rng() % 60);
    const size_t n = l.nodes.size();
    std::vector<uint32_t> start;
    mh_transcript_eval_info info;
    EXPECT(te_plan(l, -1, &start, info) == MH_OK && info.defect_kind == 0, "a well-formed transcript is accepted");
    uint64_t at = 1, zeros = 0;
    bool starts_ok = true;
    for (size_t i = 0; i < n; i++) {
      starts_ok &= start[i] == at;
      if (i == l.root) continue;
      if (l.nodes[i].kind == 0) zeros++;
      else at += l.nodes[i].kind == 8 ? (uint64_t)l.nodes[i].rhs : 1;
    }
    const uint64_t active = at + (zeros ? 1 : 0);
    EXPECT(starts_ok && info.active_rows == active && info.n_zero == zeros && info.rows == pow2(active, 2) && info.rows == info.rows_needed, "rows");
    EXPECT(te_plan(l, -1, nullptr, info) == MH_OK, "no row_start asked for");
    Te d = l;
    const size_t i = rng() % n;
    d.nodes[i].kind = 9 + (uint32_t)(rng() % 5);
    te_expect(d, -1, 2, i, 0, "an unknown kind");
    size_t k;
    if ((k = find_kind(l, 4)) < n) {
      d = l;
      d.nodes[k].op = rng() % 2 ? 0 : 5;
      te_expect(d, -1, 2, k, 1, "a uint op outside 1..4");
      d = l;
      d.nodes[k].lhs = (int64_t)k + (int64_t)(rng() % 3);
      te_expect(d, -1, 3, k, 0, "an operand that is not below the own index");
      d = l;
      d.nodes[k].rhs = -1 - (int64_t)(rng() % 5);
      te_expect(d, -1, 3, k, 1, "an external source under a uint op");
    }
    if ((k = find_kind(l, 7)) < n) {
      d = l;
      d.nodes[k].op = 4;
      te_expect(d, -1, 2, k, 1, "an EC op outside 1..3");
    }
    if ((k = find_kind(l, 3)) < n) {
      d = l;
      d.nodes[k].lhs = (int64_t)l.n_lit;
      te_expect(d, -1, 3, k, 0, "a literal past the pool");
    }
    if ((k = find_kind(l, 8)) < n) {
      d = l;
      d.nodes[k].rhs = 0;
      te_expect(d, -1, 3, k, 1, "an MSM of no term");
      d = l;
      d.nodes[k].rhs = (int64_t)l.terms.size() - d.nodes[k].lhs + 1;
      te_expect(d, -1, 3, k, 0, "a term span past the rows");
      d = l;
      d.nodes[k].lhs = INT64_MAX;
      te_expect(d, -1, 3, k, 0, "a term span that wraps");
      d = l;
      const uint64_t t = (uint64_t)l.nodes[k].lhs + rng() % (uint64_t)l.nodes[k].rhs;
      const bool base = rng() % 2;
      (base ? d.terms[t].base_node : d.terms[t].scalar_node) = (uint32_t)k;
      // an earlier term of the span, or an earlier MSM over shared rows, may fall first: only the kind is certain
      mh_transcript_eval_info bad;
      EXPECT(te_plan(d, -1, nullptr, bad) == MH_ERR_INVALID && bad.defect_kind == 3 && bad.defect_index <= t, "a term node that is not below the own index");
      d = l;
      d.nodes[k].perm = l.cycles - (uint64_t)l.nodes[k].rhs + 1;
      te_expect(d, -1, 5, k, 0, "an MSM whose last cycle is past the trace");
    }
    d = l;
    d.root = n + rng() % 3;
    te_expect(d, -1, 4, d.root, 0, "a root out of range");
    d = l;
    d.root = 0;
    te_expect(d, -1, 4, 0, 0, "a root that is a value node");
    d = l;
    d.nodes[l.root].rhs = -1 - (int64_t)l.cycles;
    te_expect(d, -1, 5, l.root, 2, "an external cycle past the trace");
    d = l;
    d.nodes[l.root].rhs = INT64_MIN;
    te_expect(d, -1, 5, l.root, 2, "the most negative source");
    d = l;
    d.nodes[0].perm = l.cycles + rng() % 2;
    te_expect(d, -1, 5, 0, 0, "an own cycle past the trace");
    te_expect(l, 25, 6, 25, 0, "a log above 24");
    int least = 0;
    while (((uint64_t)1 << least) < info.rows) least++;
    te_expect(l, least - 1, 7, info.rows, 0, "a log below the need");
    te_expect(l, -2, 7, info.rows, 0, "a log below -1");
  }
  {  // NULL pointers
    const Te l = te_good(30);
    Exact<mh_te_node> n(l.nodes);
    Exact<mh_te_term> t(l.terms);
    mh_transcript_eval_info info;
    EXPECT(mh_transcript_eval_plan(nullptr, l.nodes.size(), t.p, l.terms.size(), DANGLING32, l.n_lit, l.root, l.cycles, -1, nullptr, &info) == MH_ERR_INVALID &&
               info.defect_kind == 1 && info.defect_operand == 0, "nodes");
    if (!l.terms.empty())
      EXPECT(mh_transcript_eval_plan(n.p, l.nodes.size(), nullptr, l.terms.size(), DANGLING32, l.n_lit, l.root, l.cycles, -1, nullptr, &info) == MH_ERR_INVALID &&
                 info.defect_kind == 1 && info.defect_operand == 1, "terms");
    EXPECT(mh_transcript_eval_plan(n.p, l.nodes.size(), t.p, l.terms.size(), nullptr, l.n_lit, l.root, l.cycles, -1, nullptr, &info) == MH_ERR_INVALID &&
               info.defect_kind == 1 && info.defect_operand == 2, "limbs");
    EXPECT(mh_transcript_eval_plan(n.p, l.nodes.size(), t.p, l.terms.size(), DANGLING32, l.n_lit, l.root, l.cycles, -1, nullptr, nullptr) == MH_ERR_INVALID, "info");
    EXPECT(mh_transcript_eval_plan(nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, -1, nullptr, &info) == MH_ERR_INVALID && info.defect_kind == 4, "no node: no root");
  }
  {  // more than 2^24 rows: many MSM claims over the same few term rows
    Te l;
    l.n_lit = 1;
    l.nodes.push_back(mh_te_node{2, 0, 0, 0, 0, 0, 0, 0, 0});
    l.nodes.push_back(mh_te_node{6, 0, 0, 0, 0, 0, 0, 0, 0});
    for (int t = 0; t < 4096; t++) l.terms.push_back(mh_te_term{1, 0});
    for (int k = 0; k < 4100; k++) l.nodes.push_back(mh_te_node{8, 0, 0, 4096, 0, 0, 0, 0, 0});
    l.nodes.push_back(mh_te_node{0, 0, 0, 0, 0, 0, 0, 0, 0});
    l.root = l.nodes.size() - 1;
    l.cycles = 4096;
    mh_transcript_eval_info info;
    std::vector<uint32_t> start;
    EXPECT(te_plan(l, -1, &start, info) == MH_ERR_INVALID && info.defect_kind == 6 && info.defect_index > (uint64_t)1 << 24, "too many rows");
  }
  const int64_t edges[] = {0, 1, -1, -2, 2, 63, 64, 1 << 24, (1 << 24) + 1, (int64_t)1 << 32, INT64_MAX, INT64_MAX - 1, INT64_MIN, INT64_MIN + 1};
  auto word = [&]() { return rng() % 3 ? edges[rng() % (sizeof edges / sizeof *edges)] : (int64_t)rng(); };
  for (int round = 0; round < 4000; round++) {  // hostile: whatever comes back, no read leaves a list
    Te l;
    const size_t n = rng() % 14, nt = rng() % 6;
    for (size_t i = 0; i < n; i++) {
      const uint32_t kind = rng() % 8 ? (uint32_t)(rng() % 9) : (uint32_t)rng();
      const int64_t lhs = rng() % 2 ? word() : (int64_t)(rng() % (n + 2)), rhs = rng() % 2 ? word() : (int64_t)(rng() % (n + 2));
      l.nodes.push_back(mh_te_node{kind, rng() % 4 ? (uint32_t)(rng() % 6) : (uint32_t)rng(), lhs, rhs, rng() % 2 ? (uint64_t)word() : rng() % 16, rng(), rng(), rng(), rng()});
    }
    for (size_t t = 0; t < nt; t++) l.terms.push_back(mh_te_term{rng() % 2 ? (uint32_t)(rng() % (n + 1)) : (uint32_t)rng(), rng() % 2 ? (uint32_t)(rng() % (n + 1)) : (uint32_t)rng()});
    l.n_lit = rng() % 3 ? rng() % 4 : (uint64_t)word();
    l.root = rng() % 4 ? rng() % (n + 1) : (uint64_t)word();
    l.cycles = rng() % 2 ? rng() % 32 : (uint64_t)word();
    mh_transcript_eval_info info;
    std::vector<uint32_t> start;
    const int rc = te_plan(l, (int)(rng() % 44) - 3, rng() % 2 ? &start : nullptr, info);
    EXPECT((rc == MH_OK) == (info.defect_kind == 0) && (rc == MH_OK || rc == MH_ERR_INVALID), "an answer");
    if (rc == MH_OK) EXPECT(info.rows <= (uint64_t)1 << 24 && info.rows >= info.rows_needed && info.active_rows <= info.rows, "an accepted hostile list fits");
  }
}

int main() {
  cn_tests();
  te_tests();
  return verdict("asan_transcript_traces_plan");
}
