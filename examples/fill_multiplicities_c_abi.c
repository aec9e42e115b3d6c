/* The multiplicity column of a table lookup, counted on the device, from plain C through libmidenhip: upload a trace whose
 * multiplicity column was never computed, let mh_fill_multiplicities write it from the bus messages of the AIR's lookup program, prove
 * the filled trace where it lies and verify the proof with the library's LogUp balance assertion.
 *
 * Input: one file of little-endian u64 words --
 *     log_n, width, lookup_column, fraction, main_column        the one slot: which fraction's multiplicity is affine in which column
 *     n_air_words, n_lookup_words, n_pre_observe
 *     pcs params[7]                                             mh_pcs_params in declaration order
 *     challenger_state[12], pre_observe[n_pre_observe]
 *     air blob ("MHDAG001"), lookup blob ("MHLKP001")
 *     trace[2^log_n][width]                                     row-major
 * Exit 0: filled, balanced, proved, verified.  Exit 1: the buses do not close (a looked-up value no table row carries); the unmatched
 * denominators are printed.  tests/test_gpu_fill_multiplicities.py runs it on a one-bus table AIR.
 *
 *   gcc -O2 -Wall -Werror -Iinclude examples/fill_multiplicities_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o fill
 *   ./fill statement.bin
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include "midenhip.h"

static uint64_t* read_words(FILE* f, size_t n) {
  uint64_t* p = (uint64_t*)malloc((n ? n : 1) * sizeof(uint64_t));
  if (!p || fread(p, sizeof(uint64_t), n, f) != n) {
    fprintf(stderr, "short statement file\n");
    exit(2);
  }
  return p;
}

#define CHECK(call)                                                               \
  do {                                                                            \
    int rc_ = (call);                                                             \
    if (rc_ != MH_OK) {                                                           \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, mh_last_error(ctx));    \
      return 3;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s statement.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  uint64_t* head = read_words(f, 8);
  const int log_n = (int)head[0];
  const size_t width = (size_t)head[1], n_air = (size_t)head[5], n_lookup = (size_t)head[6], n_pre = (size_t)head[7];
  if (log_n < 1 || log_n > 24 || width < 1 || width > 1024 || head[4] >= width) {
    fprintf(stderr, "log height outside 1..24 or a column outside the trace\n");
    return 2;
  }
  const mh_mult_slot slot = {0, (uint32_t)head[2], (uint32_t)head[3], (uint32_t)head[4]};
  uint64_t* pw = read_words(f, 7);
  const mh_pcs_params params = {(int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3], (int)pw[4], (int)pw[5], (int)pw[6]};
  uint64_t* state = read_words(f, 12);
  uint64_t* pre = read_words(f, n_pre);
  uint64_t* air_blob = read_words(f, n_air);
  uint64_t* lookup_blob = read_words(f, n_lookup);
  uint64_t* rows = read_words(f, width << log_n);
  fclose(f);

  mh_ctx* ctx = NULL;
  if (mh_ctx_create(0, &ctx) != MH_OK) {
    fprintf(stderr, "mh_ctx_create failed\n");
    return 3;
  }
  mh_air* air = NULL;
  mh_lookup* lookup = NULL;
  mh_trace* trace = NULL;
  CHECK(mh_air_load(ctx, air_blob, n_air, &air));
  CHECK(mh_lookup_load(ctx, lookup_blob, n_lookup, &lookup));
  CHECK(mh_air_attach_lookup(air, lookup)); /* the aux trace is built on the device from the same program */
  CHECK(mh_trace_upload(ctx, rows, log_n, width, &trace));

  /* ---- fill: any challenges do (a cell does not depend on them); the report is the exact balance check of the filled trace ---- */
  const uint64_t challenges[4] = {3, 5, 7, 11};
  const mh_lookup* lookups[1] = {lookup};
  mh_trace* traces[1] = {trace};
  enum { ENTRY_CAP = 8 };
  mh_balance_entry entries[ENTRY_CAP];
  uint64_t written = 0;
  size_t n_entries = 0, n_pushes = 0;
  int rc = mh_fill_multiplicities(ctx, 1, lookups, traces, NULL, challenges, 2, NULL, NULL, 0, &slot, 1, &written, entries, ENTRY_CAP, &n_entries,
                                  NULL, 0, &n_pushes);
  if (rc != MH_OK && rc != MH_ERR_UNSATISFIED) {
    fprintf(stderr, "mh_fill_multiplicities failed (%d): %s\n", rc, mh_last_error(ctx));
    return 3;
  }
  CHECK(mh_trace_download(ctx, trace, rows));
  uint64_t total = 0;
  for (size_t r = 0; r < ((size_t)1 << log_n); r++) total += rows[r * width + slot.main_column];
  printf("written %" PRIu64 " cells of column %u, their sum %" PRIu64 "\n", written, slot.main_column, total);
  if (rc == MH_ERR_UNSATISFIED) {
    for (size_t i = 0; i < n_entries && i < ENTRY_CAP; i++)
      printf("unmatched denominator (%" PRIu64 ", %" PRIu64 "): net (%" PRIu64 ", %" PRIu64 ") over %" PRIu64 " pushes\n", entries[i].denom[0],
             entries[i].denom[1], entries[i].net[0], entries[i].net[1], entries[i].pushes);
    printf("%zu unmatched denominators; first: %s\n", n_entries, mh_last_error(ctx));
    return 1;
  }
  printf("balanced\n");

  /* ---- prove the filled trace where it lies, verify on the host ---- */
  mh_air* airs[1] = {air};
  mh_proof* proof = NULL;
  CHECK(mh_prove(ctx, &params, 1, airs, traces, NULL, 0, state, pre, n_pre, NULL, NULL, &proof));
  const uint64_t* blobs[1] = {air_blob};
  const size_t blob_words[1] = {n_air};
  const uint8_t heights[1] = {(uint8_t)log_n};
  uint64_t digest[4];
  char why[256];
  rc = mh_verify_ex(&params, 1, blobs, blob_words, heights, NULL, 0, state, pre, n_pre, mh_proof_fields(proof), mh_proof_num_fields(proof),
                    mh_proof_commitments(proof), mh_proof_num_commitments(proof), NULL, mh_external_logup_balance, NULL, digest, why, sizeof why);
  if (rc != MH_OK) {
    fprintf(stderr, "mh_verify_ex: %s\n", why);
    return 1;
  }
  printf("proved %zu bytes, verified, digest %016" PRIx64 "\n", mh_proof_serialize(proof, NULL, 0), digest[0]);
  mh_proof_free(proof);
  mh_trace_free(trace);
  mh_air_attach_lookup(air, NULL);
  mh_lookup_free(lookup);
  mh_air_free(air);
  mh_ctx_destroy(ctx);
  free(head); free(pw); free(state); free(pre); free(air_blob); free(lookup_blob); free(rows);
  return 0;
}
