/* The polynomial commitment scheme on its own, from plain C: commit two matrices of different heights as two LMCS trees, open both at
 * three out-of-domain points (mh_pcs_open = pcs::open_with_channel, crates/lifted-stark/src/pcs/prover.rs:34-101), verify the
 * opening on the host (mh_pcs_verify = pcs::verify_aligned, pcs/verifier.rs:72-174), then change one claimed evaluation and watch the
 * verifier refuse.  The roots are bound by the caller, as in pcs/tests.rs:69-72: their words go into pre_observe on both sides.
 *
 *   gcc -O2 -Wall -Werror -Iinclude examples/pcs_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,miden-vm_amd/lib -o pcs_c_abi
 *   ./pcs_c_abi [lmcs = 0 (Poseidon2) | 1 (Blake3) | 2 (Keccak) | 3 (RPO) | 4 (RPX)] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "midenhip.h"

#define P 0xFFFFFFFF00000001ULL
#define CHECK(call)                                                                        \
  do {                                                                                     \
    int rc_ = (call);                                                                      \
    if (rc_ != MH_OK) {                                                                    \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ctx ? mh_last_error(ctx) : ""); \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

static uint64_t lcg = 0x9E3779B97F4A7C15ULL;
static uint64_t next_felt(void) {
  lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
  return lcg % P;
}

int main(int argc, char** argv) {
  const int lmcs = argc > 1 ? atoi(argv[1]) : MH_LMCS_POSEIDON2;
  const mh_pcs_params params = {3, 2, 2, 1, 2, 5, 3}; /* toy parameters: blowup 8, arity 4, final degree 4, five queries */
  enum { LOG_A = 4, W_A = 9, LOG_B = 6, W_B = 17, N_POINTS = 3 };
  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  CHECK(mh_ctx_set_lmcs(ctx, lmcs));

  static uint64_t a[(1 << LOG_A) * W_A], b[(1 << LOG_B) * W_B];
  for (size_t i = 0; i < sizeof a / sizeof a[0]; i++) a[i] = next_felt();
  for (size_t i = 0; i < sizeof b / sizeof b[0]; i++) b[i] = next_felt();
  mh_trace *ta = NULL, *tb = NULL;
  mh_tree* trees[2] = {NULL, NULL};
  uint64_t roots[8];
  CHECK(mh_trace_upload(ctx, a, LOG_A, W_A, &ta));
  CHECK(mh_trace_upload(ctx, b, LOG_B, W_B, &tb));
  CHECK(mh_commit_traces(ctx, 1, &ta, params.log_blowup, &trees[0], roots));
  CHECK(mh_commit_traces(ctx, 1, &tb, params.log_blowup, &trees[1], roots + 4));

  /* three points outside the trace domain and the LDE coset of the TALLER matrix */
  uint64_t points[2 * N_POINTS];
  for (int k = 0; k < N_POINTS; k++) do {
      points[2 * k] = next_felt();
      points[2 * k + 1] = next_felt();
    } while (!mh_pcs_point_ok(LOG_B, params.log_blowup, points + 2 * k));

  uint64_t state[12] = {0};
  mh_proof* proof = NULL;
  CHECK(mh_pcs_open(ctx, &params, 2, (const mh_tree* const*)trees, N_POINTS, points, state, roots, 8, &proof));
  const size_t n_fields = mh_proof_num_fields(proof), n_commitments = mh_proof_num_commitments(proof);
  const uint64_t* digest = mh_proof_digest(proof);
  printf("opened 2 trees at %d points: %zu fields, %zu commitments, digest %016llx %016llx %016llx %016llx\n", N_POINTS, n_fields,
         n_commitments, (unsigned long long)digest[0], (unsigned long long)digest[1], (unsigned long long)digest[2],
         (unsigned long long)digest[3]);

  /* the verifier's side: roots, shapes, points and the two streams -- no context */
  const uint8_t heights[2] = {LOG_A, LOG_B};
  const int n_mats[2] = {1, 1};
  const size_t widths[2] = {W_A, W_B};
  static uint64_t evals[N_POINTS * (W_A + W_B) * 2];
  uint64_t vdigest[4];
  char err[512];
  int rc = mh_pcs_verify(lmcs, 0, &params, 2, roots, heights, n_mats, widths, N_POINTS, points, state, roots, 8, mh_proof_fields(proof),
                         n_fields, mh_proof_commitments(proof), n_commitments, evals, vdigest, err, sizeof err);
  if (rc != MH_OK || memcmp(vdigest, digest, sizeof vdigest) != 0) {
    fprintf(stderr, "verification failed (%d): %s\n", rc, err);
    return 1;
  }
  printf("verified: f_0(z_0^4) of the short matrix = (%llu, %llu), f_0(z_0) of the tall one = (%llu, %llu)\n", (unsigned long long)evals[0],
         (unsigned long long)evals[1], (unsigned long long)evals[2 * W_A], (unsigned long long)evals[2 * W_A + 1]);

  /* one claimed evaluation changed: the first transcript field is c0 of the first evaluation */
  uint64_t* forged = (uint64_t*)malloc(n_fields * sizeof(uint64_t));
  if (!forged) return 1;
  memcpy(forged, mh_proof_fields(proof), n_fields * sizeof(uint64_t));
  forged[0] = (forged[0] + 1) % P;
  rc = mh_pcs_verify(lmcs, 0, &params, 2, roots, heights, n_mats, widths, N_POINTS, points, state, roots, 8, forged, n_fields,
                     mh_proof_commitments(proof), n_commitments, NULL, vdigest, err, sizeof err);
  if (rc != MH_ERR_INVALID || !err[0]) {
    fprintf(stderr, "a forged evaluation was not refused (%d)\n", rc);
    return 1;
  }
  printf("tampered evaluation refused: %s\n", err);

  free(forged);
  mh_proof_free(proof);
  mh_tree_free(trees[0]);
  mh_tree_free(trees[1]);
  mh_trace_free(ta);
  mh_trace_free(tb);
  mh_ctx_destroy(ctx);
  return 0;
}
