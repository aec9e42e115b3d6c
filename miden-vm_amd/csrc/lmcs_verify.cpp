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

}  // namespace lmcs_verify

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
