/* The precompile prover's Keccak round and sponge traces from plain C without a trace cell on the host: the messages "" and "abc" go
 * to the device (mh_keccak_traces_build), which absorbs and permutes them and lays the 68 columns of KeccakRoundAir and the 67 of
 * KeccakSpongeAir -- what a Rust shim does instead of running generate_trace_from_states_inner (hash/keccak/round/mod.rs) and the
 * sponge's generate_trace (hash/keccak/sponge/trace.rs) and uploading both.  The traces are the ones mh_prove_precompile_traces takes at
 * indices 2 and 4.
 *
 *   gcc -O2 -Iinclude examples/keccak_traces_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o keccak_traces
 *   ./keccak_traces
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

enum { ROUND_WIDTH = 68, SPONGE_WIDTH = 67 };

int main(void) {
  if (sizeof(mh_keccak_msg) != 24 || sizeof(mh_keccak_traces_info) != 48) return 3;
  /* the empty message owns one chunk of the tape (chunks 0), "abc" the next (chunk 1) */
  const uint8_t bytes[3] = {'a', 'b', 'c'};
  const mh_keccak_msg msgs[2] = {{0, 0, 0}, {0, 3, 1}};

  /* the library's round programme: 106 operating slots in 10 levels */
  int32_t program[128 * 5], levels[128];
  if (mh_keccak_round_program(program) != MH_OK || mh_keccak_round_levels(levels) != MH_OK) return 3;
  int operating = 0, top = 0;
  for (int i = 0; i < 128; i++) {
    operating += program[5 * i] != 0;
    if (levels[i] > top) top = levels[i];
  }
  printf("round programme: %d operating slots, %d levels\n", operating, top + 1);

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));

  /* a message that runs past the bytes is refused by kind and index; the out-pointers stay as they were */
  const mh_keccak_msg bad_msgs[2] = {{0, 0, 0}, {1, 3, 1}};
  mh_trace *round = NULL, *sponge = NULL;
  mh_keccak_traces_info bad;
  if (mh_keccak_traces_build(ctx, bytes, sizeof bytes, bad_msgs, 2, -1, -1, &round, &sponge, NULL, &bad) != MH_ERR_INVALID || round || sponge ||
      bad.defect_kind != 1 || bad.defect_index != 1) {
    fprintf(stderr, "the defective message was not refused as kind 1 at message 1\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  uint8_t digests[2][32];
  mh_keccak_traces_info info;
  CHECK(mh_keccak_traces_build(ctx, bytes, sizeof bytes, msgs, 2, -1, -1, &round, &sponge, &digests[0][0], &info));
  printf("keccak traces: %" PRIu64 " permutations, round %" PRIu64 " rows, sponge %" PRIu64 " rows (%" PRIu64 " active)\n", info.n_perms,
         info.round_rows_needed, info.sponge_rows_needed, info.sponge_rows);
  for (int m = 0; m < 2; m++) {
    printf("keccak256(\"%s\") = ", m ? "abc" : "");
    for (int i = 0; i < 32; i++) printf("%02x", digests[m][i]);
    printf("\n");
  }
  if (info.n_perms != 2 || info.round_rows_needed != 4096 || info.sponge_rows_needed != 64 || info.sponge_rows != 64) {
    fprintf(stderr, "unexpected sizes\n");
    return 5;
  }

  /* a few cells read back: ip starts at 25 in the first lane and at 25 + 3200 in the second; both lanes are active on row 0 and not in
   * the dead round; the sponge's rows are numbered and the first row of "abc" has 3 bytes left */
  uint64_t* rt = (uint64_t*)malloc((size_t)4096 * ROUND_WIDTH * sizeof(uint64_t));
  uint64_t* st = (uint64_t*)malloc((size_t)64 * SPONGE_WIDTH * sizeof(uint64_t));
  if (!rt || !st) return 3;
  CHECK(mh_trace_download(ctx, round, rt));
  CHECK(mh_trace_download(ctx, sponge, st));
  printf("round row 0: ip %" PRIu64 " %" PRIu64 ", active %" PRIu64 " %" PRIu64 "; row 3072: active %" PRIu64 "; sponge row 32: seq %" PRIu64 ", bytes left %" PRIu64 ", chunk_ptr %" PRIu64 "\n",
         rt[0], rt[34], rt[33], rt[67], rt[3072 * ROUND_WIDTH + 33], st[32 * SPONGE_WIDTH], st[32 * SPONGE_WIDTH + 2], st[32 * SPONGE_WIDTH + 4]);
  if (rt[0] != 25 || rt[34] != 25 + 3200 || rt[33] != 1 || rt[67] != 1 || rt[3072 * ROUND_WIDTH + 33] != 0 || st[32 * SPONGE_WIDTH] != 32 ||
      st[32 * SPONGE_WIDTH + 2] != 3 || st[32 * SPONGE_WIDTH + 4] != 4) {
    fprintf(stderr, "unexpected cells\n");
    return 6;
  }

  /* the stand-alone form: the zero state through Keccak-f[1600] */
  uint64_t zero[25], outputs[25];
  memset(zero, 0, sizeof zero);
  mh_trace* alone = NULL;
  CHECK(mh_keccak_round_trace_build(ctx, zero, 1, -1, &alone, outputs));
  printf("keccak-f(0)[0] = %016" PRIx64 "\n", outputs[0]);
  if (outputs[0] != 0xF1258F7940E1DDE7ULL) return 7;

  mh_trace_free(alone);
  mh_trace_free(sponge);
  mh_trace_free(round);
  mh_ctx_destroy(ctx);
  free(st);
  free(rt);
  return 0;
}
