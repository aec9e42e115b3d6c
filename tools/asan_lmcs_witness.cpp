// Host memory safety of mh_lmcs_witness_size and mh_lmcs_witness (csrc/lmcs_plan.hpp PathTable, csrc/lmcs_verify.cpp): a stand-alone
// program, built with -fsanitize=address,undefined (make -C tools asan_lmcs_witness_run), no GPU, no Python; the companion of
// asan_lmcs_verify.cpp.  It builds small trees itself with the host hashers (lmcs_host.hpp), keeps ALL their layers, opens them by the
// reference's rule, and calls mh_lmcs_witness with output blocks of exactly the size mh_lmcs_witness_size states, so that a write past
// an end is caught:  (1) accepted openings, whose three arrays must equal the tree's own layers (path(i)[l] = node (i >> l) ^ 1 of
// level l);  (2) damaged openings and (3) random lengths, depths, indices and undersized streams around them, which must be refused
// exactly when mh_lmcs_verify refuses them, with its reason, and must leave the (sentinel-filled) blocks as they were.
#include "asan_common.hpp"
#include <string>
#include "../include/midenhip.h"
#include "../miden-vm_amd/csrc/gl.cuh"
#include "../miden-vm_amd/csrc/lmcs_host.hpp"
#include "../miden-vm_amd/csrc/lmcs_plan.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

static std::mt19937_64 rng(4321);
static u64 felt() { return rng() % GL_P; }
static const u64 SENTINEL = 0xA5A5A5A5A5A5A5A5ULL;

struct Made {
  int lmcs, salt, depth;
  size_t alignment;
  std::vector<size_t> widths;
  std::vector<u64> idx, fields, commits;
  u64 root[4];
  std::vector<std::vector<Digest4>> layers;
};

static size_t own_alignment(int lmcs) { return lmcs == MH_LMCS_BLAKE3 ? 1 : (lmcs == MH_LMCS_KECCAK ? 17 : 8); }

static Made make(int lmcs, int salt, int depth, std::vector<size_t> widths, std::vector<u64> idx) {
  Made m;
  m.lmcs = lmcs; m.salt = salt; m.depth = depth; m.alignment = own_alignment(lmcs); m.widths = widths; m.idx = idx;
  const size_t n = (size_t)1 << depth;
  size_t row_len = (size_t)salt;
  for (size_t w : widths) row_len += lmcs_plan::aligned_width(w, m.alignment);
  std::vector<std::vector<u64>> rows(n, std::vector<u64>(row_len, 0));
  m.layers.resize(depth + 1);
  m.layers[0].resize(n);
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
    m.layers[0][i] = Digest4{st[0], st[1], st[2], st[3]};
  }
  for (int l = 0; l < depth; l++) {
    m.layers[l + 1].resize(m.layers[l].size() / 2);
    for (size_t p = 0; p < m.layers[l + 1].size(); p++) m.layers[l + 1][p] = lmcs_host::compress2(lmcs, m.layers[l][2 * p], m.layers[l][2 * p + 1]);
  }
  for (int k = 0; k < 4; k++) m.root[k] = m.layers[depth][0][k];
  std::set<u64> level(idx.begin(), idx.end());
  for (u64 i : level) m.fields.insert(m.fields.end(), rows[i].begin(), rows[i].end());
  for (int l = 0; l < depth; l++) {
    std::set<u64> up;
    for (u64 x : level) {
      if (!level.count(x ^ 1)) m.commits.insert(m.commits.end(), m.layers[l][x ^ 1].begin(), m.layers[l][x ^ 1].end());
      up.insert(x >> 1);
    }
    level.swap(up);
  }
  return m;
}

struct Call {
  int rc_size, rc_verify, rc;
  size_t k = 0, n_nodes = 0;
  std::vector<u64> leaf, paths, nodes;
  char err_verify[160], err[160];
};

// both calls under test on heap blocks of exactly their lengths; `with_nodes` = 0 passes nodes = NULL
static Call witness(const Made& m, bool with_nodes = true) {
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
  Call r;
  r.rc_size = mh_lmcs_witness_size(&o, &r.k, &r.n_nodes, r.err, sizeof r.err);
  if (r.rc_size != MH_OK) r.k = r.n_nodes = 0;
  // a refused shape gets blocks of one word: whatever were written would fall outside or show
  const size_t depth = r.rc_size == MH_OK ? (size_t)m.depth : 0;
  r.leaf.assign(std::max<size_t>(1, 4 * r.k), SENTINEL);
  r.paths.assign(std::max<size_t>(1, 4 * r.k * depth), SENTINEL);
  r.nodes.assign(std::max<size_t>(1, 4 * r.n_nodes), SENTINEL);
  r.rc_verify = mh_lmcs_verify(m.lmcs, m.salt, &o, r.err_verify, sizeof r.err_verify);
  r.rc = mh_lmcs_witness(m.lmcs, m.salt, &o, r.leaf.data(), r.paths.data(), with_nodes ? r.nodes.data() : nullptr, r.err, sizeof r.err);
  return r;
}

static bool untouched(const Call& r) {
  auto all = [](const std::vector<u64>& v) { return std::all_of(v.begin(), v.end(), [](u64 x) { return x == SENTINEL; }); };
  return all(r.leaf) && all(r.paths) && all(r.nodes);
}

// the arrays of an accepted opening against the tree's own layers
static void check_against_layers(const Made& m, const Call& r) {
  std::set<u64> level(m.idx.begin(), m.idx.end());
  const std::vector<u64> uniq(level.begin(), level.end());
  EXPECT(r.k == uniq.size(), "n_leaves");
  if (r.k != uniq.size()) return;
  for (size_t q = 0; q < uniq.size(); q++) {
    EXPECT(std::equal(m.layers[0][uniq[q]].begin(), m.layers[0][uniq[q]].end(), r.leaf.begin() + 4 * q), "leaf digest");
    for (int l = 0; l < m.depth; l++) {
      const Digest4& d = m.layers[l][(uniq[q] >> l) ^ 1];
      EXPECT(std::equal(d.begin(), d.end(), r.paths.begin() + 4 * (q * (size_t)m.depth + l)), "path element");
    }
  }
  size_t at = 0;
  for (int l = 1; l <= m.depth; l++) {
    std::set<u64> up;
    for (u64 x : level) up.insert(x >> 1);
    level.swap(up);
    for (u64 x : level) {
      EXPECT(at < r.n_nodes && std::equal(m.layers[l][x].begin(), m.layers[l][x].end(), r.nodes.begin() + 4 * at), "node");
      at++;
    }
  }
  EXPECT(at == r.n_nodes, "n_nodes");
}

int main() {
  size_t n_calls = 0;
  for (int lmcs = MH_LMCS_POSEIDON2; lmcs <= MH_LMCS_RPX; lmcs++)
    for (int salt : {0, 8}) {
      const std::vector<std::pair<int, std::vector<u64>>> sets = {{4, {5}}, {4, {6, 7}}, {4, {1, 12}},
                                                                  {4, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}},
                                                                  {4, {9, 2, 9, 15, 2, 3}}, {0, {0}}, {1, {1}}, {1, {0, 1}}, {6, {63, 0, 31, 32, 33}}};
      for (const auto& s : sets) {
        const Made good = make(lmcs, salt, s.first, {3, 9, 17}, s.second);
        {
          const Call r = witness(good);
          EXPECT(r.rc_size == MH_OK && r.rc == MH_OK && r.rc_verify == MH_OK, r.err);
          check_against_layers(good, r);
          const Call r2 = witness(good, false);
          EXPECT(r2.rc == MH_OK && r2.leaf == r.leaf && r2.paths == r.paths, "nodes = NULL changes the other arrays");
          EXPECT(std::all_of(r2.nodes.begin(), r2.nodes.end(), [](u64 x) { return x == SENTINEL; }), "nodes = NULL was written");
          n_calls += 2;
        }
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
        put([](Made& b) { b.idx.push_back((u64)1 << b.depth); });
        put([](Made& b) { b.idx.push_back(~(u64)0); });
        put([](Made& b) { b.idx.clear(); });
        put([](Made& b) { b.depth += 1; });
        put([](Made& b) { b.depth = 33; });
        put([](Made& b) { b.depth = -1; });
        put([](Made& b) { b.alignment = 0; });
        put([](Made& b) { b.alignment = ~(size_t)0; });
        put([](Made& b) { b.widths[0] = ~(size_t)0; });
        put([](Made& b) { b.widths.push_back(1); });
        put([](Made& b) { b.salt = 9; });
        put([](Made& b) { b.lmcs = 5; });
        put([](Made& b) { b.fields.clear(); });
        put([](Made& b) { b.commits.clear(); b.fields.clear(); b.idx.assign(1, 0); });
        for (const Made& b : bad) {
          const Call r = witness(b);
          EXPECT(r.rc == MH_ERR_INVALID && r.rc_verify == MH_ERR_INVALID, "a damaged opening was accepted");
          EXPECT(!strcmp(r.err, r.err_verify), "another reason than mh_lmcs_verify's");
          EXPECT(untouched(r), "a refused opening wrote to the buffers");
          n_calls++;
        }
        // random shapes around the opening: streams cut or grown, indices and heights drawn freely
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
          const Call r = witness(b);
          EXPECT(r.rc == r.rc_verify, "verdict differs from mh_lmcs_verify's");
          EXPECT(!strcmp(r.err, r.err_verify), "another reason than mh_lmcs_verify's");
          if (r.rc != MH_OK) EXPECT(untouched(r), "a refused opening wrote to the buffers");
          n_calls++;
        }
      }
    }
  // the shape call and the path table alone on large and degenerate index sets
  for (int depth : {0, 1, 20, 32}) {
    std::vector<u64> idx;
    const u64 top = depth ? (((u64)1 << depth) - 1) : 0;
    for (int k = 0; k < 500; k++) idx.push_back(depth ? rng() & top : 0);
    idx.push_back(0);
    idx.push_back(top);
    mh_lmcs_opening o;
    memset(&o, 0, sizeof o);
    o.log_height = depth;
    o.indices = idx.data();
    o.n_indices = idx.size();
    size_t k = 0, n_nodes = 0;
    char err[64];
    EXPECT(mh_lmcs_witness_size(&o, &k, &n_nodes, err, sizeof err) == MH_OK, err);
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    lmcs_plan::Plan p;
    std::string why;
    EXPECT(lmcs_plan::build(depth, idx.data(), idx.size(), p, why), why.c_str());
    EXPECT(k == idx.size() && n_nodes == p.n_nodes(), "shape");
    lmcs_plan::PathTable pt;
    lmcs_plan::build_paths(p, pt);
    EXPECT(pt.parent_of.size() == (depth ? k + n_nodes - 1 : 0), "path table size");
    for (int l = 0; l < depth; l++) {  // every slot's parent exists and names the slot as one of its sources
      const size_t slots = l ? p.n_parents(l - 1) : p.n_leaves;
      for (size_t s = 0; s < slots; s++) {
        const uint32_t par = pt.parent_of[lmcs_plan::slot_off(p, l) + s];
        EXPECT(par < p.n_parents(l), "parent out of range");
        if (par >= p.n_parents(l)) continue;
        const size_t e = 2 * ((size_t)p.level_off[l] + par);
        EXPECT(p.pairs[e] == s || p.pairs[e + 1] == s, "parent does not consume its slot");
      }
    }
    n_calls++;
  }
  return verdict((std::to_string(n_calls) + " calls of mh_lmcs_witness").c_str());
}
