/* The batch verifier through the C ABI of libmidenhip, from plain C: prove a few small statements (the DummyMidenAir of
 * prove_c_abi.c at several heights), damage one proof, and put the whole batch through mh_verify_batch -- every item is replayed on
 * the host, the LMCS openings of all of them are hashed on the device in one pass.  Each verdict is compared with mh_verify_lmcs on
 * the same item.
 *
 *   gcc -O2 -Iinclude examples/verify_batch_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o verify_batch_c_abi
 *   ./verify_batch_c_abi [lmcs=0] [n_proofs=4]
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "midenhip.h"

#define GL_P 0xFFFFFFFF00000001ULL
#define MAX_PROOFS 16
enum { OP_CONST = 0, OP_MAIN = 1, OP_MUL = 12 };
enum { WIDTH = 11, AUX = 2 };

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
  int n_proofs = argc > 2 ? atoi(argv[2]) : 4;
  if (n_proofs < 2 || n_proofs > MAX_PROOFS) n_proofs = 4;
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
  mh_proof* proofs[MAX_PROOFS];
  uint8_t heights[MAX_PROOFS];
  uint64_t* damaged = NULL;
  mh_verify_item items[MAX_PROOFS];
  memset(items, 0, sizeof items);
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int p = 0; p < n_proofs; p++) { /* heights 2^4 .. 2^7, a fresh trace each */
    const int log_n = 4 + p % 4;
    const size_t n = (size_t)1 << log_n;
    uint64_t* rows = (uint64_t*)malloc(n * WIDTH * 8);
    if (!rows) return 1;
    for (size_t r = 0; r < n; r++)
      for (size_t c = 0; c < WIDTH; c++) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        rows[r * WIDTH + c] = c == 0 ? 0 : x % GL_P;
      }
    mh_air* airs[1] = {air};
    const uint64_t* host_traces[1] = {rows};
    const int log_heights[1] = {log_n};
    CHECK(mh_prove_host(ctx, &params, 1, airs, host_traces, log_heights, NULL, 0, state, pre, 11, NULL, NULL, &proofs[p]));
    free(rows);
    heights[p] = (uint8_t)log_n;
    items[p].log_trace_heights = &heights[p];
    items[p].pre_observe = pre;
    items[p].n_pre_observe = 11;
    items[p].fields = mh_proof_fields(proofs[p]);
    items[p].n_fields = mh_proof_num_fields(proofs[p]);
    items[p].commitments = mh_proof_commitments(proofs[p]);
    items[p].n_commitments = mh_proof_num_commitments(proofs[p]);
  }
  /* damage proof 1: the last felt of its field stream lies in an opened row of the last FRI round tree */
  {
    const size_t nf = items[1].n_fields;
    damaged = (uint64_t*)malloc(nf * 8);
    if (!damaged) return 1;
    memcpy(damaged, items[1].fields, nf * 8);
    damaged[nf - 1] = (damaged[nf - 1] + 1) % GL_P;
    items[1].fields = damaged;
  }
  const uint64_t* blobs[1] = {blob};
  const size_t blob_words[1] = {w};
  mh_verify_result results[MAX_PROOFS];
  CHECK(mh_verify_batch(ctx, lmcs, 0, &params, 1, blobs, blob_words, state, NULL, (size_t)n_proofs, items, results));
  int bad = 0;
  for (int p = 0; p < n_proofs; p++) {
    uint64_t vdigest[4];
    char why[256];
    const int rc = mh_verify_lmcs(lmcs, &params, 1, blobs, blob_words, items[p].log_trace_heights, NULL, 0, state, pre, 11, items[p].fields,
                                  items[p].n_fields, items[p].commitments, items[p].n_commitments, NULL, NULL, NULL, vdigest, why, sizeof why);
    printf("proof %d (2^%d rows): %s%s%s\n", p, heights[p], results[p].code == MH_OK ? "accepted" : "rejected: ",
           results[p].code == MH_OK ? "" : results[p].reason, (rc == MH_OK) == (results[p].code == MH_OK) ? "" : "  != mh_verify_lmcs");
    if ((rc == MH_OK) != (results[p].code == MH_OK)) bad = 1;
    if (rc == MH_OK && memcmp(vdigest, results[p].digest, sizeof vdigest)) bad = 1;
    if ((p == 1) == (results[p].code == MH_OK)) bad = 1; /* exactly the damaged one is rejected */
  }
  free(damaged);
  for (int p = 0; p < n_proofs; p++) mh_proof_free(proofs[p]);
  mh_air_free(air);
  mh_ctx_destroy(ctx);
  if (bad) {
    fprintf(stderr, "verdicts differ from the expected ones\n");
    return 1;
  }
  printf("batch of %d verified: 1 rejected, %d accepted\n", n_proofs, n_proofs - 1);
  return 0;
}
