/* A Miden proof from plain C whose memory rows never exist on the host: the memory chiplet's section of the chiplets trace is built on
 * the device from the list of accesses in program order (mh_miden_memory_section) -- what a Rust shim does instead of calling
 * Memory::fill_trace (processor/src/trace/chiplets/memory/mod.rs:308-406) and uploading 17 felts per access: it hands over 48 bytes.
 *
 * Input: the statement file of examples/prove_miden_c_abi.c, followed by the access list --
 *     u64 log_core, log_chiplets, log_poseidon2, n_aux_inputs
 *     u64 public_values[32], aux_inputs[n_aux_inputs]
 *     u64 core[2^log_core][51], chiplets[2^log_chiplets][22], poseidon2[2^log_poseidon2][16]     row-major, little endian
 *     u64 start_row, n_accesses
 *     mh_mem_access accesses[n_accesses]                                                         48 bytes each
 * The memory rows of the file's chiplets matrix are only compared with: they are blanked before the upload, the rebuilt trace must equal
 * the file's cell for cell, and the proof over it must be the proof mh_prove_miden makes from the three host matrices.
 *
 *   gcc -O2 -Iinclude examples/memory_section_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o memory_section
 *   ./memory_section statement.bin [hash_fn = 0 Poseidon2 | 1 Blake3_256]
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

static void* read_bytes(FILE* f, size_t n) {
  void* p = malloc(n ? n : 1);
  if (!p || fread(p, 1, n, f) != n) {
    fprintf(stderr, "short statement file\n");
    exit(2);
  }
  return p;
}
static uint64_t* read_words(FILE* f, size_t n) { return (uint64_t*)read_bytes(f, n * sizeof(uint64_t)); }

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
  uint64_t* where = read_words(f, 2);
  const uint64_t start_row = where[0];
  const size_t n = (size_t)where[1];
  mh_mem_access* accesses = (mh_mem_access*)read_bytes(f, n * sizeof(mh_mem_access));
  fclose(f);
  if (sizeof(mh_mem_access) != 48 || sizeof(mh_mem_section_info) != 40) return 3;

  /* what goes up: the chiplets matrix without its memory rows (columns 0..19 blank; 20 and 21 are not the section's) */
  const size_t chip_words = ((size_t)22) << log_chip;
  uint64_t* blank = (uint64_t*)malloc(chip_words * sizeof(uint64_t));
  if (!blank) return 3;
  memcpy(blank, chiplets, chip_words * sizeof(uint64_t));
  for (size_t r = start_row; r < start_row + n; r++) memset(blank + r * 22, 0, 20 * sizeof(uint64_t));

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));
  mh_miden* miden = NULL;
  CHECK(mh_miden_load(ctx, &miden));
  mh_trace* traces[3] = {NULL, NULL, NULL};
  CHECK(mh_trace_upload(ctx, core, log_core, 51, &traces[0]));
  CHECK(mh_trace_upload(ctx, blank, log_chip, 22, &traces[1]));
  CHECK(mh_trace_upload(ctx, poseidon2, log_p2, 16, &traces[2]));

  /* a list with a defect is refused with its kind and index, and nothing is written: the context stays usable */
  uint64_t* seen = (uint64_t*)malloc(chip_words * sizeof(uint64_t));
  if (!seen) return 3;
  if (n) {
    mh_mem_section_info bad;
    const uint32_t kind = accesses[n - 1].kind;
    accesses[n - 1].kind = 7;
    if (mh_miden_memory_section(ctx, traces[1], start_row, accesses, n, NULL, &bad) != MH_ERR_INVALID || bad.defect != 1 || bad.defect_index != n - 1) {
      fprintf(stderr, "an access of kind 7 was not refused\n");
      return 5;
    }
    printf("refused: %s\n", mh_last_error(ctx));
    accesses[n - 1].kind = kind;
    CHECK(mh_trace_download(ctx, traces[1], seen));
    if (memcmp(seen, blank, chip_words * sizeof(uint64_t)) != 0) {
      fprintf(stderr, "the refused call wrote to the trace\n");
      return 5;
    }
  }

  mh_mem_section_info info;
  uint32_t* row_of = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
  if (!row_of) return 3;
  CHECK(mh_miden_memory_section(ctx, traces[1], start_row, accesses, n, row_of, &info));
  printf("built: %" PRIu64 " rows over %" PRIu64 " words in %" PRIu64 " contexts, into 2^%d rows at row %" PRIu64 "\n", info.n_rows, info.n_words,
         info.n_contexts, (int)info.log_n, start_row);
  CHECK(mh_trace_download(ctx, traces[1], seen));
  if (memcmp(seen, chiplets, chip_words * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "the rebuilt chiplets trace differs from the host-built one\n");
    return 4;
  }
  /* row_of pairs every access with its row: the row carries the access's clock and address */
  for (size_t i = 0; i < n; i++) {
    const uint64_t* row = chiplets + (start_row + row_of[i]) * 22 + 3;
    if (row_of[i] >= n || row[6] != accesses[i].clk || row[3] + row[4] + 2 * row[5] != accesses[i].addr) {
      fprintf(stderr, "row_of[%zu] names a row of another access\n", i);
      return 4;
    }
  }
  printf("rebuilt trace equals the host-built one\n");

  mh_proof *proof = NULL, *host_proof = NULL;
  CHECK(mh_prove_miden_traces(ctx, miden, hash_fn, traces, public_values, aux_inputs, n_aux, &proof));
  CHECK(mh_prove_miden(ctx, miden, hash_fn, core, log_core, chiplets, log_chip, poseidon2, log_p2, public_values, aux_inputs, n_aux, &host_proof));
  const uint64_t *d = mh_proof_digest(proof), *hd = mh_proof_digest(host_proof);
  if (memcmp(d, hd, 4 * sizeof(uint64_t)) != 0) {
    fprintf(stderr, "the proof over the rebuilt trace differs from the proof from three host matrices\n");
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
  free(bytes); free(seen); free(blank); free(row_of); free(accesses); free(where); free(head); free(public_values); free(aux_inputs);
  free(core); free(chiplets); free(poseidon2);
  return 0;
}
