/* The precompile prover's ChunkNode and TranscriptEval traces from plain C without a permutation on the host: two Keccak claims folded
 * under a zero leaf.  The messages go to mh_keccak_traces_build (round and sponge traces, and the two Keccak digests); the Poseidon2
 * ledger -- per message the chunk chain, the digest's one chunk and the node's absorption of both their digests, then the two ANDs --
 * goes to mh_poseidon2_chiplet_trace_build with every digest a REFERENCE; mh_chunk_node_trace_build and mh_transcript_eval_trace_build
 * then read the digests their rows hold from that device-resident trace.  What comes back is the transcript root, the statement's public
 * input -- what a Rust shim does instead of running the reference's generate_trace of the chunk, node and eval chips and uploading the
 * matrices.  The traces are the ones mh_prove_precompile_traces takes at indices 0, 1, 2, 4 and 5.
 *
 *   gcc -O2 -Iinclude examples/transcript_traces_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o transcript_traces
 *   ./transcript_traces
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

enum { N_MSG = 2, LEN0 = 3, LEN1 = 40, N_BYTES = LEN0 + LEN1, N_ABS = 8, N_CYCLES = 9, N_NODES = 3 };
#define POISON 0xDEAD0000BEEF0001ULL
#define KECCAK256_PRECOMPILE_ID 1416710563871706399ULL /* precompile_id("keccak256") */

static uint64_t le32(const uint8_t* b, size_t at, size_t end) {
  uint64_t v = 0;
  for (int k = 0; k < 4; k++)
    if (at + (size_t)k < end) v |= (uint64_t)b[at + (size_t)k] << (8 * k);
  return v;
}

int main(void) {
  if (sizeof(mh_kn_record) != 64 || sizeof(mh_te_node) != 64 || sizeof(mh_te_term) != 8 || sizeof(mh_chunk_node_info) != 56 ||
      sizeof(mh_transcript_eval_info) != 80)
    return 3;
  uint8_t bytes[N_BYTES];
  memcpy(bytes, "abc", LEN0);
  for (int i = 0; i < LEN1; i++) bytes[LEN0 + i] = (uint8_t)(16 + i);
  /* message 0: one chunk, chunk row 0, sponge rows 0..31; message 1: two chunks, rows 1 2, sponge rows 32..63 */
  const mh_keccak_msg msgs[N_MSG] = {{0, LEN0, 0}, {LEN0, LEN1, 1}};

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  mh_trace *round = NULL, *sponge = NULL, *p2 = NULL, *chunk_node = NULL, *eval = NULL;
  uint8_t digests[N_MSG][32];
  CHECK(mh_keccak_traces_build(ctx, bytes, N_BYTES, msgs, N_MSG, -1, -1, &round, &sponge, &digests[0][0], NULL));

  /* the Poseidon2 ledger, absorptions 0..7 on cycles 0 | 1 | 2 | 3 4 | 5 | 6 | 7 | 8:
   *   0 chunks of message 0   1 its digest as one chunk   2 the node: (digest of 0, digest of 1) under [keccak256, 0, len, 0]
   *   3 chunks of message 1   4 its digest                5 its node: (digest of 3, digest of 4)
   *   6 AND(ZERO, node 0)     7 AND(6, node 1): the root */
  const mh_p2c_absorption abs[N_ABS] = {{{2, 0, 0, 0}, 1, 1, 1}, {{2, 0, 0, 0}, 1, 1, 1}, {{KECCAK256_PRECOMPILE_ID, 0, LEN0, 0}, 1, 1, 1},
                                        {{2, 0, 0, 0}, 2, 1, 1}, {{2, 0, 0, 0}, 1, 1, 1}, {{KECCAK256_PRECOMPILE_ID, 0, LEN1, 0}, 1, 1, 1},
                                        {{1, 0, 0, 0}, 1, 1, 1}, {{1, 0, 0, 0}, 1, 1, 1}};
  uint64_t blocks[N_CYCLES][8];
  int64_t refs[N_CYCLES][2];
  for (int c = 0; c < N_CYCLES; c++) {
    refs[c][0] = refs[c][1] = -1;
    for (int i = 0; i < 8; i++) blocks[c][i] = 0;
  }
  for (int i = 0; i < 8; i++) {
    blocks[0][i] = le32(bytes, (size_t)(4 * i), LEN0);
    blocks[1][i] = le32(digests[0], (size_t)(4 * i), 32);
    blocks[3][i] = le32(bytes, (size_t)(LEN0 + 4 * i), N_BYTES);
    blocks[4][i] = le32(bytes, (size_t)(LEN0 + 32 + 4 * i), N_BYTES);
    blocks[5][i] = le32(digests[1], (size_t)(4 * i), 32);
    blocks[2][i] = blocks[6][i] = blocks[8][i] = POISON; /* both halves are references */
  }
  for (int i = 4; i < 8; i++) blocks[7][i] = POISON;     /* AND(ZERO, .): the first half is the literal zero hash */
  refs[2][0] = 0, refs[2][1] = 1;                          /* absorption indices, not cycles */
  refs[6][0] = 3, refs[6][1] = 4;
  refs[7][1] = 2;
  refs[8][0] = 6, refs[8][1] = 5;
  CHECK(mh_poseidon2_chiplet_trace_build(ctx, abs, N_ABS, &blocks[0][0], &refs[0][0], N_CYCLES, -1, &p2, NULL, NULL, NULL));

  /* the node records: offset, len, chunk_head, sponge_head, perm_chunks, perm_digest_chunks, perm_keccak, out_mult */
  const mh_kn_record records[N_MSG] = {{0, LEN0, 0, 0, 0, 1, 2, 1}, {LEN0, LEN1, 1, 32, 3, 5, 6, 1}};
  mh_chunk_node_info cn;
  /* a node cycle that lies inside message 1's chain is refused by kind, index and operand; the out pointer stays as it was */
  mh_kn_record bad[N_MSG];
  memcpy(bad, records, sizeof bad);
  bad[0].perm_keccak = 3;
  if (mh_chunk_node_trace_build(ctx, p2, bytes, N_BYTES, &digests[0][0], bad, N_MSG, -1, &chunk_node, &cn) != MH_ERR_INVALID || chunk_node ||
      cn.defect_kind != 9 || cn.defect_index != 0 || cn.defect_operand != 2) {
    fprintf(stderr, "the node cycle inside a chain was not refused as kind 9, index 0, operand 2\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));
  CHECK(mh_chunk_node_trace_build(ctx, p2, bytes, N_BYTES, &digests[0][0], records, N_MSG, -1, &chunk_node, &cn));

  /* the transcript: a ZERO leaf, AND(ZERO, claim 0), AND(that, claim 1); a claim is the digest on its node's cycle: -1 - cycle */
  const mh_te_node nodes[N_NODES] = {{0, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, -1 - 2, 7, 0, 0, 0, 0}, {1, 0, 1, -1 - 6, 8, 0, 0, 0, 0}};
  mh_transcript_eval_info te;
  uint64_t root[4];
  CHECK(mh_transcript_eval_trace_build(ctx, p2, nodes, N_NODES, NULL, 0, NULL, 0, 2, -1, &eval, root, &te));
  printf("chunk/node: %" PRIu64 " x 42 (%" PRIu64 " chunk rows, %" PRIu64 " records); eval: %" PRIu64 " x 39 (%" PRIu64 " active rows)\n", cn.rows,
         cn.n_chunks, cn.n_records, te.rows, te.active_rows);
  printf("root: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", root[0], root[1], root[2], root[3]);

  /* row 1 of the node side holds message 1's three digests; its last is the claim the second AND absorbs */
  uint64_t* m = (uint64_t*)malloc(sizeof(uint64_t) * 42 * (size_t)cn.rows);
  uint64_t* e = (uint64_t*)malloc(sizeof(uint64_t) * 39 * (size_t)te.rows);
  if (!m || !e) return 2;
  CHECK(mh_trace_download(ctx, chunk_node, m));
  CHECK(mh_trace_download(ctx, eval, e));
  printf("h_keccak of message 1: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "; the root row's rhs: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
         m[42 + 12 + 25], m[42 + 12 + 26], m[42 + 12 + 27], m[42 + 12 + 28], e[6], e[7], e[8], e[9]);
  int ok = 1;
  for (int j = 0; j < 4; j++) ok &= m[42 + 12 + 25 + j] == e[6 + j] && e[10 + j] == root[j];
  free(m);
  free(e);
  mh_trace_free(eval);
  mh_trace_free(chunk_node);
  mh_trace_free(p2);
  mh_trace_free(sponge);
  mh_trace_free(round);
  mh_ctx_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "the rows disagree about a digest\n");
    return 4;
  }
  return 0;
}
