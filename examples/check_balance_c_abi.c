/* check_trace_balance (air/src/lookup/debug/trace/mod.rs:44-95) of a whole Miden statement from plain C through libmidenhip: which bus
 * messages are unmatched, and which rows pushed them, when every constraint holds but the LogUp buses do not balance.
 *
 * Input: the statement file of examples/prove_miden_c_abi.c --
 *     u64 log_core, log_chiplets, log_poseidon2, n_aux_inputs
 *     u64 public_values[32], aux_inputs[n_aux_inputs]
 *     u64 core[2^log_core][51], chiplets[2^log_chiplets][22], poseidon2[2^log_poseidon2][16]     row-major, little endian
 * Prints one line per unmatched denominator and one per push on it (instance -1: a boundary push of the statement) and exits 1 when the
 * buses do not balance, 0 when they do.  tests/test_gpu_check_balance.py runs it on a reference snapshot and on a copy with a wrong
 * program hash.
 *
 *   gcc -O2 -Wall -Werror -Iinclude examples/check_balance_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o check_balance
 *   ./check_balance statement.bin [exact = 0 | 1]
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

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s statement.bin [exact]\n", argv[0]);
    return 2;
  }
  const int flags = argc > 2 && atoi(argv[2]) ? MH_CHECK_EXACT : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  uint64_t* head = read_words(f, 4);
  const int log_core = (int)head[0], log_chip = (int)head[1], log_p2 = (int)head[2];
  const size_t n_aux = (size_t)head[3];
  if (log_core < 1 || log_core > 30 || log_chip < 1 || log_chip > 30 || log_p2 < 1 || log_p2 > 30) {
    fprintf(stderr, "log heights outside 1..30\n");
    return 2;
  }
  uint64_t* public_values = read_words(f, MH_MIDEN_NUM_PUBLIC_VALUES);
  uint64_t* aux_inputs = read_words(f, n_aux);
  uint64_t* core = read_words(f, ((size_t)51) << log_core);
  uint64_t* chiplets = read_words(f, ((size_t)22) << log_chip);
  uint64_t* poseidon2 = read_words(f, ((size_t)16) << log_p2);
  fclose(f);

  mh_ctx* ctx = NULL;
  int rc = mh_ctx_create(0, &ctx);
  if (rc != MH_OK) {
    fprintf(stderr, "mh_ctx_create failed (%d)\n", rc);
    return 3;
  }
  mh_miden* miden = NULL;
  rc = mh_miden_load(ctx, &miden);
  if (rc != MH_OK) {
    fprintf(stderr, "mh_miden_load failed (%d): %s\n", rc, mh_last_error(ctx));
    return 3;
  }
  enum { ENTRY_CAP = 16, PUSH_CAP = 64 };
  mh_balance_entry entries[ENTRY_CAP];
  mh_balance_push pushes[PUSH_CAP];
  size_t n = 0, n_pushes = 0;
  rc = mh_check_balance_miden(ctx, miden, core, log_core, chiplets, log_chip, poseidon2, log_p2, public_values, aux_inputs, n_aux, flags, entries,
                              ENTRY_CAP, &n, pushes, PUSH_CAP, &n_pushes);
  if (rc != MH_OK && rc != MH_ERR_UNSATISFIED) {
    fprintf(stderr, "mh_check_balance_miden failed (%d): %s\n", rc, mh_last_error(ctx));
    return 3;
  }
  for (size_t i = 0; i < n && i < ENTRY_CAP; i++) {
    const mh_balance_entry* e = &entries[i];
    printf("denominator (%" PRIu64 ", %" PRIu64 "): net (%" PRIu64 ", %" PRIu64 ") over %" PRIu64 " pushes\n", e->denom[0], e->denom[1],
           e->net[0], e->net[1], e->pushes);
    if (e->first_push == MH_BALANCE_NO_PUSHES) continue;
    for (uint64_t k = e->first_push; k < e->first_push + e->pushes && k < PUSH_CAP; k++)
      printf("  instance %d row %" PRIu64 " column %u fraction %u multiplicity (%" PRIu64 ", %" PRIu64 ")\n", pushes[k].instance, pushes[k].row,
             pushes[k].column, pushes[k].fraction, pushes[k].multiplicity[0], pushes[k].multiplicity[1]);
  }
  if (rc == MH_OK) printf("balanced\n");
  else printf("%zu unmatched denominators, %zu pushes; first: %s\n", n, n_pushes, mh_last_error(ctx));
  mh_miden_free(miden);
  mh_ctx_destroy(ctx);
  free(head); free(public_values); free(aux_inputs); free(core); free(chiplets); free(poseidon2);
  return rc == MH_OK ? 0 : 1;
}
