// Internal: an mh_lmcs_opening checked and turned into a plan (lmcs_plan.hpp), and the plan executed with the host hashers.
// Shared by mh_lmcs_verify (lmcs_verify.cpp), the batch entries (verify_batch.hip) and the recording verifier (verifier.cpp).
#pragma once
#include "../../include/midenhip.h"
#include "lmcs_plan.hpp"
#include <memory>
#include <string>
#include <vector>

namespace lmcs_verify {

inline size_t config_alignment(int lmcs) { return lmcs == MH_LMCS_BLAKE3 ? 1 : (lmcs == MH_LMCS_KECCAK ? 17 : 8); }
inline bool byte_digests(int lmcs) { return lmcs == MH_LMCS_BLAKE3 || lmcs == MH_LMCS_KECCAK; }

// Everything mh_lmcs_verify refuses except the root mismatch: false + the reason.  The indices are sorted and de-duplicated here.
// `out` points into o's streams: they must outlive it.
bool prepare(int lmcs, int salt_elems, const mh_lmcs_opening& o, lmcs_plan::Opening& out, std::string& why);
// leaves -> root with lmcs_host's hashers; true: the derived root is the opening's
bool execute_host(int lmcs, const lmcs_plan::Opening& op);
// the same walk kept: the three arrays of mh_lmcs_witness (4 words per digest), filled whatever the verdict
bool execute_host_witness(int lmcs, const lmcs_plan::Opening& op, std::vector<uint64_t>& leaf_digests, std::vector<uint64_t>& paths,
                          std::vector<uint64_t>& nodes);
// mh_lmcs_witness_size: mh_lmcs_verify's checks of the height and the indices alone, and the plan of the sorted unique indices
bool witness_shape(const mh_lmcs_opening& o, lmcs_plan::Plan& plan, std::string& why);

}  // namespace lmcs_verify

// mh_verify_batch_witness's result (verify_batch.hip; miden.cpp renumbers its items): per item the witnesses of its openings.  The
// three digest arrays of a tree are NOT copies: they point into the read-back block of the device pass that made them, which the set
// keeps whole (the device wrote the final layout).
struct mh_witness_set {
  struct Tree {
    int kind = 0, which = 0, depth = 0;
    size_t row_len = 0, n_nodes = 0;
    uint64_t root[4] = {0, 0, 0, 0};
    std::vector<uint64_t> indices, rows;
    const uint64_t *leaf_digests = nullptr, *paths = nullptr, *nodes = nullptr;  // into `blocks`
  };
  std::vector<std::vector<Tree>> items;
  std::vector<std::unique_ptr<uint64_t[]>> blocks;
};

// verifier.cpp: the host replay of one item of mh_verify_batch.  Everything mh_verify_hiding checks except the digests of the
// openings, which are recorded (with the name of their tree) for the device pass.  MH_OK, or a code and the reason.
struct DagIR;
int verify_replay_recording(int lmcs, int salt_elems, const mh_pcs_params& params, const std::vector<DagIR>& airs, const uint64_t challenger_state[12],
                            mh_external_assertions external, const mh_verify_item& it, std::vector<lmcs_plan::Opening>& openings,
                            std::vector<std::string>& labels, uint64_t digest[4], std::string& reason);
