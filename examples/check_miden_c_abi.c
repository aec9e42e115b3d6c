/* ExecutionTrace::check_constraints (processor/src/trace/mod.rs:261-278) from plain C through libmidenhip: which constraint of which
 * AIR fails on which row, before any proof is attempted.
 *
 * Input: the statement file of examples/prove_miden_c_abi.c --
 *     u64 log_core, log_chiplets, log_poseidon2, n_aux_inputs
 *     u64 public_values[32], aux_inputs[n_aux_inputs]
 *     u64 core[2^log_core][51], chiplets[2^log_chiplets][22], poseidon2[2^log_poseidon2][16]     row-major, little endian
 * Prints one line per failing constraint (instance -1: an external assertion, the bus balance) and exits 1 when the statement is not
 * satisfied, 0 when it is.  tests/test_gpu_check_constraints.py runs it on the reference processor's snapshot case 13 and a perturbed copy.
 *
 *   gcc -O2 -Wall -Werror -Iinclude examples/check_miden_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o check_miden
 *   ./check_miden statement.bin [exact = 0 | 1]
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
  mh_check_entry entries[64];
  size_t n = 0;
  rc = mh_check_miden(ctx, miden, core, log_core, chiplets, log_chip, poseidon2, log_p2, public_values, aux_inputs, n_aux, flags, entries, 64, &n);
  if (rc != MH_OK && rc != MH_ERR_UNSATISFIED) {
    fprintf(stderr, "mh_check_miden failed (%d): %s\n", rc, mh_last_error(ctx));
    return 3;
  }
  for (size_t i = 0; i < n && i < 64; i++)
    printf("instance %d constraint %u: %" PRIu64 " rows, first %" PRIu64 ", value (%" PRIu64 ", %" PRIu64 ")\n", entries[i].instance,
           entries[i].constraint, entries[i].rows, entries[i].first_row, entries[i].value[0], entries[i].value[1]);
  if (rc == MH_OK) printf("satisfied\n");
  else printf("%zu failing entries; first: %s\n", n, mh_last_error(ctx));
  mh_miden_free(miden);
  mh_ctx_destroy(ctx);
  free(head); free(public_values); free(aux_inputs); free(core); free(chiplets); free(poseidon2);
  return rc == MH_OK ? 0 : 1;
}
