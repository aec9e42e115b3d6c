// The SHAPE of an LMCS batch opening (lmcs/config.rs:172-211), separated from its hashing.
//
// Which nodes of the tree a verifier derives, which siblings it takes from the commitment stream, and in which order, depends on
// (depth, sorted unique indices) alone.  The plan lists, level by level from the leaves up, one (left source, right source) pair per
// parent; a source is slot i of the level below (slot i of level 0 = the i-th opened leaf) or sibling s of the stream.  The rule is
// the verifier's (verifier.cpp open_batch): going left to right, node n pairs with n ^ 1 when that is the next opened node,
// otherwise it consumes one streamed digest.  Whoever executes the plan -- the host (lmcs_verify.cpp) or the device
// (verify_batch.hip) -- hashes the leaves, walks the levels and compares slot 0 of the last one with the root.
//
// No hashing here and nothing of the configuration beyond the row alignment (8, 17 for Keccak, 1 for Blake3).  Host only, no HIP.
// Every length is checked before anything is sized by it: the inputs are hostile (mh_lmcs_verify, the sanitizer driver under tools/).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace lmcs_plan {

constexpr uint32_t SIBLING = 0x80000000u;  // source = SIBLING | s: sibling s of the stream; otherwise slot i of the level below
constexpr int MAX_DEPTH = 32;              // the field's two-adicity: no domain is taller
constexpr size_t MAX_WIDTH = (size_t)1 << 20, MAX_MATS = 4096, MAX_ALIGNMENT = (size_t)1 << 20;
constexpr size_t MAX_LEAVES = (size_t)1 << 24;  // opened leaves of one opening (sources are 31-bit)

struct Plan {
  int depth = 0;
  size_t n_leaves = 0;
  size_t n_siblings = 0;            // digests the commitment stream must carry, exactly
  std::vector<uint32_t> level_off;  // depth + 1 entries: the parents of level l are pairs [level_off[l], level_off[l + 1])
  std::vector<uint32_t> pairs;      // 2 per parent: left source, right source
  std::vector<uint64_t> indices;    // the opened indices as build() took them: slot q of level 0 is leaf indices[q]
  size_t n_parents(int l) const { return level_off[l + 1] - level_off[l]; }
  size_t n_nodes() const { return pairs.size() / 2; }  // derived parents of all levels; level_off[l] places level l's among them
};

// What reading the opening back as a Merkle witness (mh_lmcs_witness*) needs beside the plan: for every slot of the level below, the
// parent that consumes it.  The slots of level 0 (the leaves) come first, then level after level the parents of the plan, the root
// excluded: slot_off(plan, l) + i is slot i of level l, and parent_of[..] is a slot of level l + 1 = a parent of pairs level l.
// The authentication path of leaf q is then: a = q; per level l: p = parent_of[slot_off(l) + a], the path element is the source of
// pair level_off[l] + p that is not slot a, a = p.  The node set in `nodes` order is the plan's own: parent level_off[l] + p.
struct PathTable {
  std::vector<uint32_t> parent_of;  // n_leaves + n_nodes - 1 entries (depth 0: none)
};
inline size_t slot_off(const Plan& pl, int l) { return l == 0 ? 0 : pl.n_leaves + pl.level_off[l - 1]; }
inline void build_paths(const Plan& pl, PathTable& out) {
  out.parent_of.assign(pl.depth ? pl.n_leaves + pl.n_nodes() - 1 : 0, 0);
  for (int l = 0; l < pl.depth; l++) {
    const size_t s0 = slot_off(pl, l);
    for (size_t p = 0; p < pl.n_parents(l); p++)
      for (int side = 0; side < 2; side++) {
        const uint32_t s = pl.pairs[2 * ((size_t)pl.level_off[l] + p) + side];
        if (!(s & SIBLING)) out.parent_of[s0 + s] = (uint32_t)p;
      }
  }
}

inline size_t aligned_width(size_t w, size_t alignment) { return (w + alignment - 1) / alignment * alignment; }

// idx: ascending, without duplicates, every index < 2^depth.  false + a reason otherwise (the plan is then unusable).
inline bool build(int depth, const uint64_t* idx, size_t n, Plan& out, std::string& why) {
  out = Plan();
  if (depth < 0 || depth > MAX_DEPTH) return why = "tree height out of range (0..32)", false;
  if (n < 1) return why = "an opening needs at least one index", false;
  if (n > MAX_LEAVES) return why = "too many opened leaves", false;
  for (size_t i = 0; i < n; i++) {
    if (idx[i] >> depth) return why = "index outside the tree", false;
    if (i && idx[i] <= idx[i - 1]) return why = "indices not sorted and unique", false;
  }
  out.depth = depth;
  out.n_leaves = n;
  out.indices.assign(idx, idx + n);
  out.level_off.reserve((size_t)depth + 1);
  out.level_off.push_back(0);
  std::vector<uint64_t> level(idx, idx + n), up;
  for (int d = depth; d > 0; d--) {
    up.clear();
    for (size_t i = 0; i < level.size();) {
      const uint64_t node = level[i];
      uint32_t self = (uint32_t)i, other;
      if (i + 1 < level.size() && level[i + 1] == (node ^ 1)) {
        other = (uint32_t)(i + 1);
        i += 2;
      } else {
        other = SIBLING | (uint32_t)out.n_siblings++;
        i += 1;
      }
      out.pairs.push_back((node & 1) ? other : self);
      out.pairs.push_back((node & 1) ? self : other);
      up.push_back(node >> 1);
    }
    level.swap(up);
    out.level_off.push_back((uint32_t)(out.pairs.size() / 2));
  }
  // distinct indices below 2^depth meet in one node after depth levels
  if (level.size() != 1) return why = "internal: the plan does not end in one node", false;
  return true;
}

// felts the opening's field stream must carry, exactly: per opened leaf the aligned rows of every matrix, then the raw salt.
// false: a width, the alignment or the product is out of range.
inline bool field_count(const size_t* widths, size_t n_mats, size_t alignment, size_t salt_elems, size_t n_leaves, size_t& row_len,
                        size_t& total, std::string& why) {
  if (alignment < 1 || alignment > MAX_ALIGNMENT) return why = "alignment out of range", false;
  if (n_mats < 1 || n_mats > MAX_MATS) return why = "a tree holds between 1 and 4096 matrices", false;
  row_len = salt_elems;
  for (size_t m = 0; m < n_mats; m++) {
    if (widths[m] > MAX_WIDTH) return why = "matrix width out of range", false;
    row_len += aligned_width(widths[m], alignment);  // <= 4096 * 2^21 + 8: no overflow
  }
  if (n_leaves > MAX_LEAVES) return why = "too many opened leaves", false;
  total = row_len * n_leaves;  // < 2^34 * 2^24
  return true;
}

// A validated opening, ready to be hashed: the streams are known to have the plan's lengths and to hold canonical felts.
struct Opening {
  uint64_t root[4] = {0, 0, 0, 0};
  std::vector<uint32_t> hashed;  // what a leaf absorbs, in order: the aligned width of every matrix, then the salt width if any
  size_t row_len = 0;            // their sum
  Plan plan;
  const uint64_t* rows = nullptr;  // plan.n_leaves x row_len felts (the caller's field stream)
  const uint64_t* sibs = nullptr;  // plan.n_siblings x 4 words (the caller's commitment stream)
};

}  // namespace lmcs_plan
