/* The precompile prover's Poseidon2 chiplet trace from plain C without a permutation on the host: a chain of two blocks, a one-shot and
 * an absorption of both their digests (the Keccak node's triple) go to the device as a ledger whose third absorption REFERS to the first
 * two (mh_poseidon2_chiplet_trace_build); the device hashes level by level and lays the 32 columns of Poseidon2Air -- what a Rust shim
 * does instead of running Poseidon2Requires' generate_trace (transcript/poseidon2/trace.rs) and uploading the matrix.  The trace is the
 * one mh_prove_precompile_traces takes at index 1.
 *
 *   gcc -O2 -Iinclude examples/poseidon2_chiplet_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o poseidon2_chiplet
 *   ./poseidon2_chiplet
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

enum { WIDTH = 32, N_ABS = 3, N_CYCLES = 4, ROWS = 64 };
#define POISON 0xDEAD0000BEEF0001ULL

int main(void) {
  if (sizeof(mh_p2c_absorption) != 56 || sizeof(mh_p2c_info) != 48) return 3;
  /* cycles 0 1: the chain; 2: the one-shot; 3: (digest of absorption 0, digest of absorption 1), the literals poisoned */
  const mh_p2c_absorption abs[N_ABS] = {{{1, 2, 3, 4}, 2, 1, 1}, {{5, 6, 7, 8}, 1, 2, 1}, {{9, 10, 11, 12}, 1, 1, 3}};
  uint64_t blocks[N_CYCLES][8];
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 8; i++) blocks[c][i] = 100 * (uint64_t)(c + 1) + (uint64_t)i;
  for (int i = 0; i < 8; i++) blocks[3][i] = POISON;
  const int64_t refs[N_CYCLES][2] = {{-1, -1}, {-1, -1}, {-1, -1}, {0, 1}};

  /* the planner alone: host only, no context */
  uint64_t start[N_ABS];
  uint32_t level[N_ABS];
  mh_p2c_info plan;
  if (mh_poseidon2_chiplet_plan(abs, N_ABS, &refs[0][0], N_CYCLES, start, level, &plan) != MH_OK) return 3;
  printf("plan: %" PRIu64 " absorptions, %" PRIu64 " cycles, %" PRIu64 " levels, %" PRIu64 " rows; starts %" PRIu64 " %" PRIu64 " %" PRIu64 ", levels %u %u %u\n",
         plan.n_absorptions, plan.n_cycles, plan.n_levels, plan.rows_needed, start[0], start[1], start[2], level[0], level[1], level[2]);
  if (plan.n_levels != 2 || plan.rows_needed != ROWS || start[2] != 3 || level[2] != 1) return 4;

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));

  /* a reference to the absorption itself is refused by kind and index; the out-pointer stays as it was */
  const int64_t bad_refs[N_CYCLES][2] = {{-1, -1}, {-1, -1}, {-1, -1}, {0, 2}};
  mh_trace* trace = NULL;
  mh_p2c_info bad;
  if (mh_poseidon2_chiplet_trace_build(ctx, abs, N_ABS, &blocks[0][0], &bad_refs[0][0], N_CYCLES, -1, &trace, NULL, NULL, &bad) != MH_ERR_INVALID || trace ||
      bad.defect_kind != 4 || bad.defect_index != 7) {
    fprintf(stderr, "the self-reference was not refused as kind 4 at index 7\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  uint64_t digests[N_ABS][4], outputs[N_CYCLES][12];
  mh_p2c_info info;
  CHECK(mh_poseidon2_chiplet_trace_build(ctx, abs, N_ABS, &blocks[0][0], &refs[0][0], N_CYCLES, -1, &trace, &digests[0][0], &outputs[0][0], &info));
  printf("poseidon2 chiplet: %" PRIu64 " cycles in %" PRIu64 " levels, 2^%d rows\n", info.n_cycles, info.n_levels, info.log_n);
  for (int a = 0; a < N_ABS; a++)
    printf("digest %d = %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", a, digests[a][0], digests[a][1], digests[a][2], digests[a][3]);

  /* the literal form from the digests that came back: the same bytes */
  uint64_t lit[N_CYCLES][8];
  memcpy(lit, blocks, sizeof lit);
  memcpy(&lit[3][0], digests[0], 32);
  memcpy(&lit[3][4], digests[1], 32);
  mh_trace* literal = NULL;
  CHECK(mh_poseidon2_chiplet_trace_build(ctx, abs, N_ABS, &lit[0][0], NULL, N_CYCLES, -1, &literal, NULL, NULL, NULL));
  uint64_t* a = (uint64_t*)malloc((size_t)ROWS * WIDTH * sizeof(uint64_t));
  uint64_t* b = (uint64_t*)malloc((size_t)ROWS * WIDTH * sizeof(uint64_t));
  if (!a || !b) return 3;
  CHECK(mh_trace_download(ctx, trace, a));
  CHECK(mh_trace_download(ctx, literal, b));
  if (memcmp(a, b, (size_t)ROWS * WIDTH * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "the reference form and the literal form differ\n");
    return 5;
  }
  printf("reference form == literal form\n");

  /* a few cells: row 48 is the first row of cycle 3 -- its state starts with the two digests; the chain's second cycle absorbs */
  const uint64_t* r48 = a + 48 * WIDTH;
  printf("row 48: seq %" PRIu64 ", in_mult %" PRIu64 ", out_mult %" PRIu64 ", is_absorb %" PRIu64 ", state[0] %016" PRIx64 ", state[4] %016" PRIx64 ", cube[0] %016" PRIx64
         "; row 16: is_absorb %" PRIu64 "; row 63: state[0] %016" PRIx64 "\n",
         r48[0], r48[1], r48[2], r48[3], r48[4], r48[8], r48[19], a[16 * WIDTH + 3], a[63 * WIDTH + 4]);
  if (r48[0] != 3 || r48[1] != 1 || r48[2] != 3 || r48[3] != 0 || r48[4] != digests[0][0] || r48[8] != digests[1][0] || a[16 * WIDTH + 3] != 1 ||
      a[63 * WIDTH + 4] != digests[2][0] || outputs[3][0] != digests[2][0] || outputs[1][3] != digests[0][3]) {
    fprintf(stderr, "unexpected cells\n");
    return 6;
  }

  mh_trace_free(literal);
  mh_trace_free(trace);
  mh_ctx_destroy(ctx);
  free(b);
  free(a);
  return 0;
}
