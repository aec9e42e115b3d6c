/* A Miden proof from plain C whose third main trace never exists on the host: the Poseidon2 permutation trace is derived on the device
 * from the hasher controller's rows of the chiplets trace (mh_miden_poseidon2_trace) -- what a Rust shim does instead of calling
 * fill_poseidon2_permutation_trace (processor/src/trace/chiplets/hasher/trace.rs:361-408) and uploading its 16 columns.
 *
 * Input: the statement file of examples/prove_miden_c_abi.c --
 *     u64 log_core, log_chiplets, log_poseidon2, n_aux_inputs
 *     u64 public_values[32], aux_inputs[n_aux_inputs]
 *     u64 core[2^log_core][51], chiplets[2^log_chiplets][22], poseidon2[2^log_poseidon2][16]     row-major, little endian
 * The host-built poseidon2 matrix of the file is only compared with: the derived trace must equal it cell for cell, and the proof
 * from (core, chiplets, derived) must be the proof mh_prove_miden makes from the three host matrices.
 *
 *   gcc -O2 -Iinclude examples/p2_trace_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o p2_trace
 *   ./p2_trace statement.bin [hash_fn = 0 Poseidon2 | 1 Blake3_256]
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
    fprintf(stderr, "usage: %s statement.bin [hash_fn]\n", argv[0]);
    return 2;
  }
  const int hash_fn = argc > 2 ? atoi(argv[2]) : MH_LMCS_POSEIDON2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  uint64_t* head = read_words(f, 4);
  const int log_core = (int)head[0], log_chip = (int)head[1], log_p2 = (int)head[2];
  const size_t n_aux = (size_t)head[3];
  uint64_t* public_values = read_words(f, MH_MIDEN_NUM_PUBLIC_VALUES);
  uint64_t* aux_inputs = read_words(f, n_aux);
  uint64_t* core = read_words(f, ((size_t)51) << log_core);
  uint64_t* chiplets = read_words(f, ((size_t)22) << log_chip);
  uint64_t* poseidon2 = read_words(f, ((size_t)16) << log_p2);
  fclose(f);

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  mh_miden* miden = NULL;
  CHECK(mh_miden_load(ctx, &miden));

  /* the two traces that carry information go up; the third is made where it is used */
  mh_trace* traces[3] = {NULL, NULL, NULL};
  CHECK(mh_trace_upload(ctx, core, log_core, 51, &traces[0]));
  CHECK(mh_trace_upload(ctx, chiplets, log_chip, 22, &traces[1]));
  mh_p2_trace_info info;
  CHECK(mh_miden_poseidon2_trace(ctx, traces[1], log_p2, &traces[2], &info));
  printf("derived: %" PRIu64 " requests from %" PRIu64 " controller input rows, 2^%d rows\n", info.n_requests, info.n_input_rows, (int)info.log_n);

  const size_t p2_words = ((size_t)16) << log_p2;
  uint64_t* derived = (uint64_t*)malloc(p2_words * sizeof(uint64_t));
  if (!derived) return 3;
  CHECK(mh_trace_download(ctx, traces[2], derived));
  if (memcmp(derived, poseidon2, p2_words * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "the derived trace differs from the host-built one\n");
    return 4;
  }
  printf("derived trace equals the host-built one\n");

  /* a height with no padding cycle left is a defect of the request, not a crash: the context stays usable */
  if (info.n_requests >= 4) {
    int small = 6;
    while ((((uint64_t)1 << (small + 1)) >> 4) < info.n_requests + 1) small++;
    mh_trace* none = NULL;
    mh_p2_trace_info bad;
    if (mh_miden_poseidon2_trace(ctx, traces[1], small, &none, &bad) != MH_ERR_INVALID || none || bad.defect != 4) {
      fprintf(stderr, "a trace of 2^%d rows was not refused\n", small);
      return 5;
    }
    printf("refused: %s\n", mh_last_error(ctx));
  }

  mh_proof *proof = NULL, *host_proof = NULL;
  CHECK(mh_prove_miden_traces(ctx, miden, hash_fn, traces, public_values, aux_inputs, n_aux, &proof));
  CHECK(mh_prove_miden(ctx, miden, hash_fn, core, log_core, chiplets, log_chip, poseidon2, log_p2, public_values, aux_inputs, n_aux, &host_proof));
  const uint64_t *d = mh_proof_digest(proof), *hd = mh_proof_digest(host_proof);
  if (memcmp(d, hd, 4 * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "the proof from the derived trace differs from the proof from three host matrices\n");
    return 6;
  }
  const size_t n_bytes = mh_proof_serialize(proof, NULL, 0);
  uint8_t* bytes = (uint8_t*)malloc(n_bytes);
  if (!bytes || mh_proof_serialize(proof, bytes, n_bytes) != n_bytes) return 3;
  printf("proof: %zu bytes\n", n_bytes);
  printf("digest %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", d[0], d[1], d[2], d[3]);

  uint64_t vd[4];
  char err[256] = "";
  if (mh_verify_miden(hash_fn, public_values, aux_inputs, n_aux, bytes, n_bytes, vd, err, sizeof err) != MH_OK || memcmp(vd, d, sizeof vd) != 0) {
    fprintf(stderr, "mh_verify_miden refused the proof: %s\n", err);
    return 7;
  }
  printf("verified\n");

  mh_proof_free(proof);
  mh_proof_free(host_proof);
  for (int i = 0; i < 3; i++) mh_trace_free(traces[i]);
  mh_miden_free(miden);
  mh_ctx_destroy(ctx);
  free(bytes); free(derived); free(head); free(public_values); free(aux_inputs); free(core); free(chiplets); free(poseidon2);
  return 0;
}
