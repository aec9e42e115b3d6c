// Host memory safety of the opening plan, the checks in front of it and mh_lmcs_verify (csrc/lmcs_plan.hpp, csrc/lmcs_verify.cpp):
// a stand-alone program, built with -fsanitize=address,undefined (make -C tools asan_lmcs_verify_run), no GPU, no Python.
// It builds small trees itself with the host hashers (lmcs_host.hpp) under all five configurations, opens them by the reference's
// rule written out independently here (per level: the opened nodes whose sibling is not opened stream it, left to right), and feeds
// mh_lmcs_verify  (1) the openings, which must be accepted,  (2) every damage class of tests/test_lmcs_verify.py, which must be
// refused,  (3) random lengths, counts, heights, widths, alignments and indices around them, which must neither be accepted when
// they differ from the opening nor touch memory they do not own.  Exit code 0 and "clean" only if all of that holds.
#include "asan_common.hpp"
#include <string>
#include "../include/midenhip.h"
#include "../miden-vm_amd/csrc/gl.cuh"
#include "../miden-vm_amd/csrc/lmcs_host.hpp"
#include "../miden-vm_amd/csrc/lmcs_plan.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

static std::mt19937_64 rng(12345);
static u64 felt() { return rng() % GL_P; }
struct Made {
  int lmcs, salt, depth;
  size_t alignment;
  std::vector<size_t> widths;
  std::vector<u64> idx, fields, commits;
  u64 root[4];
};

static size_t own_alignment(int lmcs) { return lmcs == MH_LMCS_BLAKE3 ? 1 : (lmcs == MH_LMCS_KECCAK ? 17 : 8); }

// a tree of 2^depth leaves over matrices of the given widths (all of tree height), salted or not, opened at idx
static Made make(int lmcs, int salt, int depth, std::vector<size_t> widths, std::vector<u64> idx) {
  Made m;
  m.lmcs = lmcs; m.salt = salt; m.depth = depth; m.alignment = own_alignment(lmcs); m.widths = widths; m.idx = idx;
  const size_t n = (size_t)1 << depth;
  size_t row_len = (size_t)salt;
  for (size_t w : widths) row_len += lmcs_plan::aligned_width(w, m.alignment);
  std::vector<std::vector<u64>> rows(n, std::vector<u64>(row_len, 0));
  std::vector<std::vector<Digest4>> layers(depth + 1);
  layers[0].resize(n);
  for (size_t i = 0; i < n; i++) {
    u64 st[lmcs_host::MAX_STATE_WORDS] = {0};
    size_t off = 0;
    for (size_t w : widths) {
      const size_t aw = lmcs_plan::aligned_width(w, m.alignment);
      for (size_t k = 0; k < w; k++) rows[i][off + k] = felt();
      lmcs_host::leaf_absorb(lmcs, st, rows[i].data() + off, aw);
      off += aw;
    }
    if (salt) {
      for (int k = 0; k < salt; k++) rows[i][off + k] = felt();
      lmcs_host::leaf_absorb(lmcs, st, rows[i].data() + off, (size_t)salt);
    }
    layers[0][i] = Digest4{st[0], st[1], st[2], st[3]};
  }
  for (int l = 0; l < depth; l++) {
    layers[l + 1].resize(layers[l].size() / 2);
    for (size_t p = 0; p < layers[l + 1].size(); p++) layers[l + 1][p] = lmcs_host::compress2(lmcs, layers[l][2 * p], layers[l][2 * p + 1]);
  }
  for (int k = 0; k < 4; k++) m.root[k] = layers[depth][0][k];
  std::set<u64> level(idx.begin(), idx.end());
  for (u64 i : level) m.fields.insert(m.fields.end(), rows[i].begin(), rows[i].end());
  for (int l = 0; l < depth; l++) {
    std::set<u64> up;
    for (u64 x : level) {
      if (!level.count(x ^ 1)) m.commits.insert(m.commits.end(), layers[l][x ^ 1].begin(), layers[l][x ^ 1].end());
      up.insert(x >> 1);
    }
    level.swap(up);
  }
  return m;
}

// the call under test, with every array copied into a heap block of exactly its length so that any read past an end is caught
static int verify(const Made& m, char* err, size_t cap) {
  std::vector<size_t> w(m.widths);
  std::vector<u64> idx(m.idx), f(m.fields), c(m.commits);
  mh_lmcs_opening o;
  for (int k = 0; k < 4; k++) o.root[k] = m.root[k];
  o.log_height = m.depth;
  o.n_mats = (int)w.size();
  o.widths = w.data();
  o.alignment = m.alignment;
  o.indices = idx.data(); o.n_indices = idx.size();
  o.fields = f.data(); o.n_fields = f.size();
  o.commitments = c.data(); o.n_commit_felts = c.size();
  return mh_lmcs_verify(m.lmcs, m.salt, &o, err, cap);
}

int main() {
  char err[160];
  size_t n_calls = 0;
  for (int lmcs = MH_LMCS_POSEIDON2; lmcs <= MH_LMCS_RPX; lmcs++)
    for (int salt : {0, 1, 8}) {
      const std::vector<std::vector<u64>> sets = {{5}, {6, 7}, {1, 12}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {9, 2, 9, 15, 2, 3}};
      for (const auto& idx : sets) {
        const Made good = make(lmcs, salt, 4, {3, 9, 17}, idx);
        EXPECT(verify(good, err, sizeof err) == MH_OK, err);
        n_calls++;
        std::vector<Made> bad;
        auto put = [&](auto change) {
          Made b = good;
          change(b);
          bad.push_back(b);
        };
        put([](Made& b) { b.fields[b.fields.size() / 2] = (b.fields[b.fields.size() / 2] + 1) % GL_P; });
        if (!good.commits.empty()) {
          put([](Made& b) { b.commits[1] ^= 1; });
          put([](Made& b) { b.commits.resize(b.commits.size() - 4); });
          put([](Made& b) { b.commits.resize(b.commits.size() - 1); });
        }
        put([](Made& b) { b.root[2] = (b.root[2] + 1) % GL_P; });
        put([](Made& b) { b.fields.pop_back(); });
        put([](Made& b) { b.fields.push_back(0); });
        put([](Made& b) { b.commits.insert(b.commits.end(), 4, 1); });
        put([](Made& b) { b.fields[0] = GL_P; });
        put([](Made& b) { b.fields[0] = ~(u64)0; });
        put([](Made& b) { b.idx.push_back((u64)1 << b.depth); });
        put([](Made& b) { b.idx.push_back(~(u64)0); });
        put([](Made& b) { b.idx.clear(); });
        put([](Made& b) { b.depth = 3; });
        put([](Made& b) { b.depth = 5; });
        put([](Made& b) { b.depth = 33; });
        put([](Made& b) { b.depth = -1; });
        put([](Made& b) { b.depth = 0; });
        put([](Made& b) { b.alignment = 0; });
        put([](Made& b) { b.alignment = 3; });
        put([](Made& b) { b.alignment = ~(size_t)0; });
        put([](Made& b) { b.widths[0] = ~(size_t)0; });
        put([](Made& b) { b.widths[1] = (size_t)1 << 40; });
        put([](Made& b) { b.widths.clear(); });
        put([](Made& b) { b.widths.push_back(1); });
        put([](Made& b) { b.salt = b.salt == 8 ? 7 : b.salt + 1; });
        put([](Made& b) { b.salt = 9; });
        put([](Made& b) { b.lmcs = 5; });
        put([](Made& b) { b.fields.clear(); });
        put([](Made& b) { b.commits.clear(); b.fields.clear(); b.idx.assign(1, 0); });
        for (const Made& b : bad) {
          const bool same = b.fields == good.fields && b.commits == good.commits;  // (commits.clear() of an opening without siblings)
          if (b.widths.empty()) {  // n_mats = 0 with a dangling pointer: refused before it is read
            EXPECT(verify(b, err, sizeof err) == MH_ERR_INVALID, "no matrix");
          } else if (!(same && b.depth == good.depth && b.idx == good.idx && b.alignment == good.alignment && b.widths == good.widths &&
                       b.salt == good.salt && b.lmcs == good.lmcs && std::equal(b.root, b.root + 4, good.root))) {
            EXPECT(verify(b, err, sizeof err) == MH_ERR_INVALID, "a damaged opening was accepted");
            EXPECT(err[0] != 0, "no reason given");
          }
          n_calls++;
        }
        // random shapes around the opening: lengths cut or grown, indices and heights drawn freely
        for (int it = 0; it < 60; it++) {
          Made b = good;
          b.fields.resize(rng() % (good.fields.size() + 20));
          for (size_t k = good.fields.size(); k < b.fields.size(); k++) b.fields[k] = rng();
          b.commits.resize(rng() % (good.commits.size() + 12));
          for (size_t k = good.commits.size(); k < b.commits.size(); k++) b.commits[k] = rng();
          if (it % 3 == 0) b.depth = (int)(rng() % 40) - 3;
          if (it % 4 == 0) {
            b.idx.resize(rng() % 40);
            for (u64& x : b.idx) x = (it % 8) ? rng() % 64 : rng();
          }
          if (it % 5 == 0) b.alignment = rng() % 40;
          if (it % 7 == 0) b.widths.assign(1 + rng() % 5, rng() % 30);
          const int rc = verify(b, err, it % 2 ? sizeof err : (size_t)(rng() % 8));
          const bool untouched = b.fields == good.fields && b.commits == good.commits && b.depth == good.depth && b.idx == good.idx &&
                                 b.alignment == good.alignment && b.widths == good.widths;
          // (other widths can add up to the same aligned stream, which is the same leaf: those calls are checked for memory safety only)
          if (it % 7 != 0) EXPECT(rc == (untouched ? MH_OK : MH_ERR_INVALID), "a random variation was accepted");
          n_calls++;
        }
      }
    }
  // the plan alone on large and degenerate index sets
  for (int depth : {0, 1, 20, 32}) {
    std::vector<u64> idx;
    const u64 top = depth ? (((u64)1 << depth) - 1) : 0;
    for (int k = 0; k < 500; k++) idx.push_back(depth ? rng() & top : 0);
    idx.push_back(0);
    idx.push_back(top);
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    lmcs_plan::Plan p;
    std::string why;
    EXPECT(lmcs_plan::build(depth, idx.data(), idx.size(), p, why), why.c_str());
    EXPECT(p.level_off.size() == (size_t)depth + 1 && p.pairs.size() == 2 * (size_t)p.level_off.back(), "plan shape");
    size_t below = idx.size();
    for (int l = 0; l < depth; l++) {  // every source points into the level below or into the stream
      for (size_t e = 2 * (size_t)p.level_off[l]; e < 2 * (size_t)p.level_off[l + 1]; e++) {
        const uint32_t s = p.pairs[e];
        EXPECT((s & lmcs_plan::SIBLING) ? (s & ~lmcs_plan::SIBLING) < p.n_siblings : s < below, "source out of range");
      }
      below = p.n_parents(l);
    }
    EXPECT(below == 1 || depth == 0, "the plan ends in one node");
  }
  return verdict((std::to_string(n_calls) + " calls of mh_lmcs_verify").c_str());
}
