/* Merkle witnesses from a verified proof through the C ABI of libmidenhip, from plain C: prove one small statement (the
 * DummyMidenAir of prove_c_abi.c), put it through mh_verify_batch_witness, and read back what the verifier derived -- per tree of
 * the proof a leaf hash and an authentication path per query, and the inner nodes.  Every path is then checked on its own: the rows
 * of one leaf and its path are a single-index opening, and mh_lmcs_verify must accept it against the tree's root.  This is the data a
 * recursive verifier loads into its Merkle store.
 *
 *   gcc -O2 -Iinclude examples/witness_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o witness_c_abi
 *   ./witness_c_abi [lmcs=0]
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "midenhip.h"

#define GL_P 0xFFFFFFFF00000001ULL
enum { OP_CONST = 0, OP_MAIN = 1, OP_MUL = 12 };
enum { WIDTH = 11, AUX = 2, LOG_N = 5 };

static uint64_t node(uint64_t op, uint64_t a, uint64_t b) { return op | (a << 8) | (b << 36); }

#define CHECK(call)                                                                  \
  do {                                                                               \
    int rc_ = (call);                                                                \
    if (rc_ != MH_OK) {                                                              \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ctx ? mh_last_error(ctx) : "no ctx"); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

int main(int argc, char** argv) {
  const int lmcs = argc > 1 ? atoi(argv[1]) : MH_LMCS_POSEIDON2;
  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  CHECK(mh_ctx_set_lmcs(ctx, lmcs));

  uint64_t blob[12 + 2 * 19 + 1];
  size_t w = 0;
  const uint64_t header[12] = {0x4d48444147303031ULL, WIDTH, AUX, 2, AUX, 0, 0, 3, 19, 1, 0, 0};
  for (int i = 0; i < 12; i++) blob[w++] = header[i];
  blob[w++] = node(OP_CONST, 0, 0); blob[w++] = 1;
  uint64_t prod = 0, next_id = 1;
  for (uint64_t j = 0; j < 9; j++) {
    blob[w++] = node(OP_MAIN, j, 0); blob[w++] = 0;
    const uint64_t leaf = next_id++;
    blob[w++] = node(OP_MUL, prod, leaf); blob[w++] = 0;
    prod = next_id++;
  }
  blob[w++] = prod;
  mh_air* air = NULL;
  CHECK(mh_air_load(ctx, blob, w, &air));

  const mh_pcs_params params = {3, 2, 2, 1, 2, 6, 3};
  const uint64_t state[12] = {0};
  const uint64_t pre[11] = {6, 3, 2, 1, 3, 2, 4, 0, /*n publics*/ 0, 0, /*n aux inputs*/ 0}; /* observe_protocol_params + an empty statement */
  const size_t n = (size_t)1 << LOG_N;
  uint64_t* rows = (uint64_t*)malloc(n * WIDTH * 8);
  if (!rows) return 1;
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (size_t r = 0; r < n; r++)
    for (size_t c = 0; c < WIDTH; c++) {
      x = x * 6364136223846793005ULL + 1442695040888963407ULL;
      rows[r * WIDTH + c] = c == 0 ? 0 : x % GL_P;
    }
  mh_air* airs[1] = {air};
  const uint64_t* host_traces[1] = {rows};
  const int log_heights[1] = {LOG_N};
  mh_proof* proof = NULL;
  CHECK(mh_prove_host(ctx, &params, 1, airs, host_traces, log_heights, NULL, 0, state, pre, 11, NULL, NULL, &proof));
  free(rows);

  const uint8_t height = LOG_N;
  mh_verify_item item;
  memset(&item, 0, sizeof item);
  item.log_trace_heights = &height;
  item.pre_observe = pre;
  item.n_pre_observe = 11;
  item.fields = mh_proof_fields(proof);
  item.n_fields = mh_proof_num_fields(proof);
  item.commitments = mh_proof_commitments(proof);
  item.n_commitments = mh_proof_num_commitments(proof);
  const uint64_t* blobs[1] = {blob};
  const size_t blob_words[1] = {w};
  mh_verify_result result;
  mh_witness_set* set = NULL;
  CHECK(mh_verify_batch_witness(ctx, lmcs, 0, &params, 1, blobs, blob_words, state, NULL, 1, &item, &result, &set));
  if (result.code != MH_OK) {
    fprintf(stderr, "the proof was rejected: %s\n", result.reason);
    return 1;
  }
  const size_t n_trees = mh_witness_set_trees(set, 0);
  size_t n_paths = 0;
  int bad = 0;
  for (size_t t = 0; t < n_trees; t++) {
    mh_witness_tree tr;
    CHECK(mh_witness_set_tree(set, 0, t, &tr));
    /* the last node is the root the proof committed to */
    if (tr.depth > 0 && memcmp(tr.nodes + 4 * (tr.n_nodes - 1), tr.root, sizeof tr.root)) bad = 1;
    for (size_t q = 0; q < tr.n_leaves; q++) {
      /* every tree of this statement holds one matrix, so a leaf absorbs its row in one piece: one matrix of row_len cells, alignment 1 */
      mh_lmcs_opening o;
      memset(&o, 0, sizeof o);
      memcpy(o.root, tr.root, sizeof o.root);
      o.log_height = tr.depth;
      o.n_mats = 1;
      o.widths = &tr.row_len;
      o.alignment = 1;
      o.indices = tr.indices + q;
      o.n_indices = 1;
      o.fields = tr.rows + q * tr.row_len;
      o.n_fields = tr.row_len;
      o.commitments = tr.paths + 4 * q * (size_t)tr.depth;
      o.n_commit_felts = 4 * (size_t)tr.depth;
      char why[256];
      if (mh_lmcs_verify(lmcs, 0, &o, why, sizeof why) != MH_OK) {
        fprintf(stderr, "tree %zu, leaf %" PRIu64 ": %s\n", t, tr.indices[q], why);
        bad = 1;
      }
      n_paths++;
    }
    printf("%s tree %d: depth %d, %zu leaves, %zu nodes, root %016" PRIx64 "\n", tr.kind ? "FRI round" : "committed", tr.which, tr.depth,
           tr.n_leaves, tr.n_nodes, tr.root[0]);
  }
  mh_witness_set_free(set);
  mh_proof_free(proof);
  mh_air_free(air);
  mh_ctx_destroy(ctx);
  if (bad || !n_trees) {
    fprintf(stderr, "a path did not verify on its own\n");
    return 1;
  }
  printf("%zu trees, %zu paths: each verified on its own\n", n_trees, n_paths);
  return 0;
}
