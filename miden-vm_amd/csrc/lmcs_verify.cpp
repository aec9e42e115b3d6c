// mh_lmcs_verify: the counterpart of mh_tree_open (the reference's Lmcs::open_batch, lmcs/config.rs:172-211) -- HOST ONLY, no context.
// An opening is checked in two steps: prepare() refuses everything that can be told from the lengths, the indices and the felts
// alone and builds the plan (lmcs_plan.hpp); execute_host() hashes it with the hashers of lmcs_host.hpp and compares with the root.
// The batch entries (verify_batch.hip) share prepare() and run the same plan on the device.
#include "lmcs_verify.hpp"
#include "gl.cuh"
#include "lmcs_host.hpp"
#include <algorithm>
#include <cstdio>
#include <exception>

namespace lmcs_verify {

bool prepare(int lmcs, int salt_elems, const mh_lmcs_opening& o, lmcs_plan::Opening& out, std::string& why) {
  if (lmcs < MH_LMCS_POSEIDON2 || lmcs > MH_LMCS_RPX) return why = "unknown LMCS hasher id", false;
  if (salt_elems < 0 || salt_elems > MH_MAX_SALT_ELEMS) return why = "salt_elems must be in 0..MH_MAX_SALT_ELEMS", false;
  if (!o.widths || (!o.indices && o.n_indices) || (!o.fields && o.n_fields) || (!o.commitments && o.n_commit_felts))
    return why = "null array", false;
  if (o.n_mats < 1) return why = "a tree holds between 1 and 4096 matrices", false;
  if (o.log_height < 0 || o.log_height > lmcs_plan::MAX_DEPTH) return why = "tree height out of range (0..32)", false;
  if (o.n_indices < 1) return why = "an opening needs at least one index", false;
  if (o.n_indices > lmcs_plan::MAX_LEAVES) return why = "too many opened leaves", false;
  for (size_t i = 0; i < o.n_indices; i++)
    if (o.indices[i] >> o.log_height) return why = "index " + std::to_string(i) + " outside the tree", false;
  std::vector<uint64_t> idx(o.indices, o.indices + o.n_indices);
  std::sort(idx.begin(), idx.end());
  idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
  size_t total = 0;
  if (!lmcs_plan::field_count(o.widths, (size_t)o.n_mats, o.alignment, (size_t)salt_elems, idx.size(), out.row_len, total, why)) return false;
  if (o.n_fields != total)
    return why = std::string(o.n_fields < total ? "field stream too short" : "trailing data in the field stream") + ": " +
                 std::to_string(o.n_fields) + " felts, the opening carries " + std::to_string(total),
           false;
  if (!lmcs_plan::build(o.log_height, idx.data(), idx.size(), out.plan, why)) return false;
  if (o.n_commit_felts != 4 * out.plan.n_siblings)
    return why = std::string(o.n_commit_felts < 4 * out.plan.n_siblings ? "commitment stream too short" : "trailing data in the commitment stream") +
                 ": " + std::to_string(o.n_commit_felts) + " words, the opening carries " + std::to_string(out.plan.n_siblings) + " digests",
           false;
  for (size_t i = 0; i < o.n_fields; i++)
    if (o.fields[i] >= GL_P) return why = "non-canonical field element", false;
  if (!byte_digests(lmcs)) {  // a byte digest's words are not felts
    for (size_t i = 0; i < o.n_commit_felts; i++)
      if (o.commitments[i] >= GL_P) return why = "non-canonical digest element", false;
    for (int i = 0; i < 4; i++)
      if (o.root[i] >= GL_P) return why = "non-canonical digest element in the root", false;
  }
  out.hashed.clear();
  for (int m = 0; m < o.n_mats; m++) out.hashed.push_back((uint32_t)lmcs_plan::aligned_width(o.widths[m], o.alignment));
  if (salt_elems) out.hashed.push_back((uint32_t)salt_elems);
  for (int i = 0; i < 4; i++) out.root[i] = o.root[i];
  out.rows = o.fields;
  out.sibs = o.commitments;
  return true;
}

bool execute_host(int lmcs, const lmcs_plan::Opening& op) {
  const lmcs_plan::Plan& pl = op.plan;
  std::vector<Digest4> cur(pl.n_leaves), next;
  for (size_t q = 0; q < pl.n_leaves; q++) {
    u64 st[lmcs_host::MAX_STATE_WORDS] = {0};
    const u64* row = op.rows + q * op.row_len;
    for (uint32_t w : op.hashed) {
      lmcs_host::leaf_absorb(lmcs, st, row, w);
      row += w;
    }
    cur[q] = Digest4{st[0], st[1], st[2], st[3]};
  }
  auto source = [&](uint32_t s) {
    if (!(s & lmcs_plan::SIBLING)) return cur[s];
    const u64* d = op.sibs + 4 * (size_t)(s & ~lmcs_plan::SIBLING);
    return Digest4{d[0], d[1], d[2], d[3]};
  };
  for (int l = 0; l < pl.depth; l++) {
    const size_t np = pl.n_parents(l);
    next.resize(np);
    for (size_t p = 0; p < np; p++) {
      const size_t e = 2 * ((size_t)pl.level_off[l] + p);
      next[p] = lmcs_host::compress2(lmcs, source(pl.pairs[e]), source(pl.pairs[e + 1]));
    }
    cur.swap(next);
  }
  return cur.size() == 1 && cur[0] == Digest4{op.root[0], op.root[1], op.root[2], op.root[3]};
}

bool execute_host_witness(int lmcs, const lmcs_plan::Opening& op, std::vector<u64>& leaf_digests, std::vector<u64>& paths, std::vector<u64>& nodes) {
  const lmcs_plan::Plan& pl = op.plan;
  lmcs_plan::PathTable pt;
  lmcs_plan::build_paths(pl, pt);
  leaf_digests.resize(4 * pl.n_leaves);
  paths.resize(4 * pl.n_leaves * (size_t)pl.depth);
  nodes.resize(4 * pl.n_nodes());
  for (size_t q = 0; q < pl.n_leaves; q++) {
    u64 st[lmcs_host::MAX_STATE_WORDS] = {0};
    const u64* row = op.rows + q * op.row_len;
    for (uint32_t w : op.hashed) {
      lmcs_host::leaf_absorb(lmcs, st, row, w);
      row += w;
    }
    for (int i = 0; i < 4; i++) leaf_digests[4 * q + i] = st[i];
  }
  std::vector<uint32_t> anc(pl.n_leaves);  // the slot of every leaf's ancestor on the current level
  for (size_t q = 0; q < pl.n_leaves; q++) anc[q] = (uint32_t)q;
  const u64* cur = leaf_digests.data();  // the level below: the leaves, then the nodes of the level before
  for (int l = 0; l < pl.depth; l++) {
    auto source = [&](uint32_t s) { return (s & lmcs_plan::SIBLING) ? op.sibs + 4 * (size_t)(s & ~lmcs_plan::SIBLING) : cur + 4 * (size_t)s; };
    const size_t p0 = pl.level_off[l], s0 = lmcs_plan::slot_off(pl, l);
    for (size_t p = 0; p < pl.n_parents(l); p++) {
      const u64 *a = source(pl.pairs[2 * (p0 + p)]), *b = source(pl.pairs[2 * (p0 + p) + 1]);
      const Digest4 d = lmcs_host::compress2(lmcs, Digest4{a[0], a[1], a[2], a[3]}, Digest4{b[0], b[1], b[2], b[3]});
      for (int i = 0; i < 4; i++) nodes[4 * (p0 + p) + i] = d[i];
    }
    for (size_t q = 0; q < pl.n_leaves; q++) {
      const uint32_t p = pt.parent_of[s0 + anc[q]];
      const uint32_t ls = pl.pairs[2 * (p0 + p)], rs = pl.pairs[2 * (p0 + p) + 1];
      const u64* other = source(ls == anc[q] ? rs : ls);
      for (int i = 0; i < 4; i++) paths[4 * (q * (size_t)pl.depth + l) + i] = other[i];
      anc[q] = p;
    }
    cur = nodes.data() + 4 * p0;
  }
  const u64* top = pl.depth ? nodes.data() + 4 * (pl.n_nodes() - 1) : leaf_digests.data();
  return top[0] == op.root[0] && top[1] == op.root[1] && top[2] == op.root[2] && top[3] == op.root[3];
}

bool witness_shape(const mh_lmcs_opening& o, lmcs_plan::Plan& plan, std::string& why) {
  if (!o.indices && o.n_indices) return why = "null array", false;
  if (o.log_height < 0 || o.log_height > lmcs_plan::MAX_DEPTH) return why = "tree height out of range (0..32)", false;
  if (o.n_indices < 1) return why = "an opening needs at least one index", false;
  if (o.n_indices > lmcs_plan::MAX_LEAVES) return why = "too many opened leaves", false;
  for (size_t i = 0; i < o.n_indices; i++)
    if (o.indices[i] >> o.log_height) return why = "index " + std::to_string(i) + " outside the tree", false;
  std::vector<uint64_t> idx(o.indices, o.indices + o.n_indices);
  std::sort(idx.begin(), idx.end());
  idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
  return lmcs_plan::build(o.log_height, idx.data(), idx.size(), plan, why);
}

}  // namespace lmcs_verify

namespace {
int reject(char* err, size_t err_cap, int code, const std::string& msg) {
  if (err && err_cap) snprintf(err, err_cap, "opening rejected: %s", msg.c_str());
  return code;
}
}  // namespace

extern "C" int mh_lmcs_witness_size(const mh_lmcs_opening* o, size_t* n_leaves, size_t* n_nodes, char* err, size_t err_cap) {
  try {
    if (!o || !n_leaves || !n_nodes) return reject(err, err_cap, MH_ERR_INVALID, "null argument");
    lmcs_plan::Plan plan;
    std::string why;
    if (!lmcs_verify::witness_shape(*o, plan, why)) return reject(err, err_cap, MH_ERR_INVALID, why);
    *n_leaves = plan.n_leaves;
    *n_nodes = plan.n_nodes();
    if (err && err_cap) err[0] = 0;
    return MH_OK;
  } catch (const std::exception& e) {
    return reject(err, err_cap, MH_ERR_INTERNAL, e.what());
  }
}

extern "C" int mh_lmcs_witness(int lmcs, int salt_elems, const mh_lmcs_opening* o, uint64_t* leaf_digests, uint64_t* paths, uint64_t* nodes,
                               char* err, size_t err_cap) {
  try {
    if (!o) return reject(err, err_cap, MH_ERR_INVALID, "null argument");
    lmcs_plan::Opening op;
    std::string why;
    if (!lmcs_verify::prepare(lmcs, salt_elems, *o, op, why)) return reject(err, err_cap, MH_ERR_INVALID, why);
    if (!leaf_digests || (!paths && op.plan.depth)) return reject(err, err_cap, MH_ERR_INVALID, "null output buffer");
    std::vector<u64> ld, pa, nd;
    if (!lmcs_verify::execute_host_witness(lmcs, op, ld, pa, nd)) return reject(err, err_cap, MH_ERR_INVALID, "Merkle root mismatch");
    std::copy(ld.begin(), ld.end(), leaf_digests);
    std::copy(pa.begin(), pa.end(), paths);
    if (nodes) std::copy(nd.begin(), nd.end(), nodes);
    if (err && err_cap) err[0] = 0;
    return MH_OK;
  } catch (const std::exception& e) {
    return reject(err, err_cap, MH_ERR_INTERNAL, e.what());
  }
}

extern "C" int mh_lmcs_verify(int lmcs, int salt_elems, const mh_lmcs_opening* o, char* err, size_t err_cap) {
  auto fail = [&](int code, const std::string& msg) {
    if (err && err_cap) snprintf(err, err_cap, "opening rejected: %s", msg.c_str());
    return code;
  };
  try {
    if (!o) return fail(MH_ERR_INVALID, "null argument");
    lmcs_plan::Opening op;
    std::string why;
    if (!lmcs_verify::prepare(lmcs, salt_elems, *o, op, why)) return fail(MH_ERR_INVALID, why);
    if (!lmcs_verify::execute_host(lmcs, op)) return fail(MH_ERR_INVALID, "Merkle root mismatch");
    if (err && err_cap) err[0] = 0;
    return MH_OK;
  } catch (const std::exception& e) {
    return fail(MH_ERR_INTERNAL, e.what());
  }
}
