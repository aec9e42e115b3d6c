/* The hasher controller's rows and the Poseidon2 permutation trace from plain C without a permutation on the host: a small mixed list of
 * hash operations goes to the device (mh_miden_hasher_section), which computes the permutations, writes the controller rows in place into
 * a device-resident chiplets trace and numbers the distinct pre-states; mh_miden_poseidon2_trace then derives the statement's third
 * main trace from those rows -- what a Rust shim does instead of running Hasher::permute / hash_basic_block / build_merkle_root /
 * update_merkle_root (processor/src/trace/chiplets/hasher/mod.rs) and uploading rows x 20 cells.
 *
 *   gcc -O2 -Iinclude examples/hasher_section_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o hasher_section
 *   ./hasher_section
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "midenhip.h"

#define CHECK(call)                                                                              \
  do {                                                                                           \
    int rc_ = (call);                                                                            \
    if (rc_ != MH_OK) {                                                                          \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ctx ? mh_last_error(ctx) : "no ctx"); \
      return 1;                                                                                  \
    }                                                                                            \
  } while (0)

enum { LOG_N = 7, N = 1 << LOG_N, WIDTH = 22, DEPTH = 3, N_OPS = 7 };

int main(void) {
  if (sizeof(mh_hash_op) != 24 || sizeof(mh_hash_result) != 136 || sizeof(mh_hasher_section_info) != 48) return 3;
  /* operands: a 12-felt state | h1, h2 | three batches | old value, new value, three siblings */
  uint64_t felts[12 + 8 + 24 + 8 + 4 * DEPTH];
  const size_t n_felts = sizeof felts / sizeof felts[0];
  for (size_t i = 0; i < n_felts; i++) felts[i] = 0x9E3779B97F4A7C15ULL * (i + 1);   /* any uint64_t: reduced mod p on the device */
  const uint64_t state = 0, h12 = 12, batches = 20, old_value = 44;   /* the new value follows at 48, the siblings at 52 */
  const mh_hash_op ops[N_OPS] = {
      {0, 0, 0, state},                  /* HPERM */
      {1, 0, 5, h12},                    /* a control block, domain 5 */
      {2, 3, 0, batches},                /* a basic block of three batches */
      {3, DEPTH, 5, old_value},          /* MPVERIFY: value | siblings = the four words from old_value on */
      {4, DEPTH, 5, old_value},          /* MRUPDATE old -> new at node 5 */
      {0, 0, 0, state},                  /* the first state again: the same perm_id, no new request */
      {2, 3, 0, batches},                /* a memoised replay of the block: the operation listed again */
  };
  /* a chiplets trace whose every row is a padding row (s0..s4 = 1) with its clock: the hasher section is written over its first rows */
  uint64_t* host = (uint64_t*)calloc((size_t)N * WIDTH, sizeof(uint64_t));
  if (!host) return 3;
  for (size_t r = 0; r < N; r++) {
    for (int c = 0; c < 5; c++) host[r * WIDTH + c] = 1;
    host[r * WIDTH + WIDTH - 1] = r + 1;
  }

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  mh_trace* chiplets = NULL;
  CHECK(mh_trace_upload(ctx, host, LOG_N, WIDTH, &chiplets));

  /* a defective list is refused by index and kind, nothing is written, and the context goes on */
  mh_hash_op bad_ops[N_OPS];
  memcpy(bad_ops, ops, sizeof ops);
  bad_ops[4].index = 8;                  /* 8 >> 3 != 0: invalid index for the path */
  mh_hasher_section_info bad;
  if (mh_miden_hasher_section(ctx, chiplets, bad_ops, N_OPS, felts, n_felts, NULL, &bad) != MH_ERR_INVALID || bad.defect != 3 || bad.defect_index != 4) {
    fprintf(stderr, "the defective list was not refused as defect 3 at op 4\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  mh_hash_result results[N_OPS];
  mh_hasher_section_info info;
  CHECK(mh_miden_hasher_section(ctx, chiplets, ops, N_OPS, felts, n_felts, results, &info));
  printf("hasher section: n_rows %" PRIu64 ", n_permutations %" PRIu64 ", n_requests %" PRIu64 ", mrupdate_id %" PRIu64 "\n", info.n_rows,
         info.n_permutations, info.n_requests, info.mrupdate_id);
  const uint64_t want_perms = 1 + 1 + 3 + DEPTH + 2 * DEPTH + 1 + 3;
  if (info.n_permutations != want_perms || info.n_rows != ((2 * want_perms + 7) & ~(uint64_t)7) || info.mrupdate_id != 1 ||
      info.n_requests != want_perms - 4 /* the repeated permute and the replayed block's three */) {
    fprintf(stderr, "unexpected counts\n");
    return 5;
  }
  if (results[0].addr != 1 || results[1].addr != 3 || results[5].addr != 2 * (1 + 1 + 3 + 3 * DEPTH) + 1 ||
      memcmp(results[0].state, results[5].state, sizeof results[0].state) != 0 || memcmp(results[2].state, results[6].state, 4 * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "unexpected results\n");
    return 5;
  }
  printf("block digest %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " at addr %" PRIu64 "\n", results[2].state[0], results[2].state[1],
         results[2].state[2], results[2].state[3], results[2].addr);

  /* the rows on the host: column 0 is the hasher's selector, the rows below the section and the clock column were not touched */
  uint64_t* got = (uint64_t*)malloc((size_t)N * WIDTH * sizeof(uint64_t));
  if (!got) return 3;
  CHECK(mh_trace_download(ctx, chiplets, got));
  for (size_t r = 0; r < N; r++) {
    const int inside = r < info.n_rows;
    if (got[r * WIDTH] != (inside ? 0u : 1u) || got[r * WIDTH + WIDTH - 1] != r + 1 ||
        (!inside && memcmp(got + r * WIDTH, host + r * WIDTH, WIDTH * sizeof(uint64_t)) != 0)) {
      fprintf(stderr, "row %zu is not what it should be\n", r);
      return 6;
    }
  }

  /* the third main trace from the rows just written: its request count is the section's */
  mh_trace* third = NULL;
  mh_p2_trace_info p2;
  CHECK(mh_miden_poseidon2_trace(ctx, chiplets, -1, &third, &p2));
  printf("poseidon2 trace: %" PRIu64 " requests from %" PRIu64 " controller input rows, 2^%d rows\n", p2.n_requests, p2.n_input_rows, (int)p2.log_n);
  if (p2.n_requests != info.n_requests || p2.n_input_rows != info.n_permutations) {
    fprintf(stderr, "the permutation trace counts other requests than the section\n");
    return 7;
  }
  printf("n_requests agree\n");

  mh_trace_free(third);
  mh_trace_free(chiplets);
  mh_ctx_destroy(ctx);
  free(got);
  free(host);
  return 0;
}
