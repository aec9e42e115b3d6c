/* The whole chiplets trace from plain C without a chiplets cell on the host: the five lists of a small program -- hash operations,
 * bitwise operations, memory accesses, one circuit evaluation, the kernel's procedures and the calls made -- go to the device
 * (mh_miden_chiplets_build), which lays the five sections behind their selector prefixes, pads and numbers the rows;
 * mh_miden_poseidon2_trace then derives the statement's third main trace from it -- what a Rust shim does instead of running
 * Chiplets::fill_trace (processor/src/trace/chiplets/mod.rs) and uploading 2^log_n x 22 cells.
 *
 *   gcc -O2 -Iinclude examples/chiplets_build_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o chiplets_build
 *   ./chiplets_build
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

#define INS(l, r, op) ((uint64_t)(l) | ((uint64_t)(r) << 30) | ((uint64_t)(op) << 60)) /* op: 0 sub, 1 mul, 2 add */

enum { WIDTH = 22 };

int main(void) {
  if (sizeof(mh_bitwise_op) != 12 || sizeof(mh_ace_eval) != 32 || sizeof(mh_ace_section_info) != 56) return 3;
  /* hasher: a permutation and a control block */
  uint64_t hash_felts[20];
  for (size_t i = 0; i < 20; i++) hash_felts[i] = 0x9E3779B97F4A7C15ULL * (i + 1);
  const mh_hash_op hash_ops[2] = {{0, 0, 0, 0}, {1, 0, 5, 12}};
  const mh_bitwise_op bitwise_ops[3] = {{0, 0xDEADBEEFu, 0x0F0F1234u}, {1, 0xDEADBEEFu, 0x0F0F1234u}, {0, 0xFFFFFFFFu, 0x80000000u}};
  /* the circuit x (x - 1) - r over the inputs x = 3, r = 6 and the constant -1 (wire ids 7, 6, 5, 4; gates 3, 2, 1, 0): it is zero */
  const uint64_t p = 0xFFFFFFFF00000001ULL;
  const uint64_t ace_felts[12] = {3, 0, 6, 0, p - 1, 0, 0, 0, INS(7, 5, 2), INS(7, 3, 1), INS(2, 6, 0), INS(1, 1, 1)};
  const mh_ace_eval ace_evals[1] = {{0, 1024, 9, 4, 4, 0, 0}};
  /* memory: the circuit's words written, then read as the evaluation reads them (two word reads, four element reads at clk 9) */
  mh_mem_access mem[9];
  memset(mem, 0, sizeof mem);
  for (int w = 0; w < 3; w++) {
    mem[w].addr = 1024 + 4 * w; mem[w].clk = 1 + w; mem[w].kind = 2;
    memcpy(mem[w].value, ace_felts + 4 * w, 32);
  }
  for (int w = 0; w < 2; w++) { mem[3 + w].addr = 1024 + 4 * w; mem[3 + w].clk = 9; mem[3 + w].kind = 3; }
  for (int k = 0; k < 4; k++) { mem[5 + k].addr = 1032 + k; mem[5 + k].clk = 9; mem[5 + k].kind = 1; }
  /* the kernel: 0x0100 sorts before 0x0001 (byte order), the third procedure is declared twice */
  const uint64_t procs[4][4] = {{0x0001, 0, 0, 0}, {0x0100, 0, 0, 0}, {7, 7, 7, 7}, {7, 7, 7, 7}};
  const uint64_t calls[3][4] = {{7, 7, 7, 7}, {0x0001, 0, 0, 0}, {7, 7, 7, 7}};
  mh_chiplets_lists lists = {hash_ops, 2, hash_felts, 20, bitwise_ops, 3, mem, 9, ace_evals, 1, ace_felts, 12, &procs[0][0], 4, &calls[0][0], 3};

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));

  /* a defective list is refused by section, kind and index; no trace exists afterwards and the context goes on */
  mh_bitwise_op bad_ops[3];
  memcpy(bad_ops, bitwise_ops, sizeof bad_ops);
  bad_ops[2].op = 2;
  mh_chiplets_lists bad_lists = lists;
  bad_lists.bitwise_ops = bad_ops;
  mh_trace* none = NULL;
  mh_chiplets_info bad;
  if (mh_miden_chiplets_build(ctx, &bad_lists, -1, &none, &bad) != MH_ERR_INVALID || none || bad.defect_section != 1 || bad.defect != 1 ||
      bad.defect_index != 2) {
    fprintf(stderr, "the defective list was not refused as section 1, defect 1 at op 2\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  mh_trace* chiplets = NULL;
  mh_chiplets_info info;
  CHECK(mh_miden_chiplets_build(ctx, &lists, -1, &chiplets, &info));
  printf("chiplets trace: 2^%d rows, trace_len %" PRIu64 ", starts %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 ", padding from %" PRIu64 "\n",
         (int)info.log_n, info.trace_len, info.start[0], info.start[1], info.start[2], info.start[3], info.start[4], info.padding_start);
  printf("ace: %" PRIu64 " rows, %" PRIu64 " wires, %" PRIu64 " gates, %" PRIu64 " rounds; kernel rom: %" PRIu64 " rows for %" PRIu64 " calls\n",
         info.ace.n_rows, info.ace.n_wires, info.ace.n_gates, info.ace.n_rounds, info.kernel_rom.n_rows, info.kernel_rom.n_calls);
  if (info.start[1] != 8 || info.start[2] != 32 || info.start[3] != 41 || info.start[4] != 47 || info.padding_start != 50 || info.log_n != 6) {
    fprintf(stderr, "unexpected layout\n");
    return 5;
  }

  const size_t n = (size_t)1 << info.log_n;
  uint64_t* got = (uint64_t*)malloc(n * WIDTH * sizeof(uint64_t));
  if (!got) return 3;
  CHECK(mh_trace_download(ctx, chiplets, got));
  const uint64_t* last_and = got + (info.start[1] + 7) * WIDTH;   /* the eighth row of the first bitwise operation: its result */
  const uint64_t* kr = got + info.start[4] * WIDTH;               /* the kernel ROM's first row: 0x0100, never called */
  printf("and result %08" PRIx64 ", first kernel row m %" PRIu64 " h0 %" PRIx64 "\n", last_and[14], kr[5], kr[6]);
  if (last_and[14] != (0xDEADBEEFu & 0x0F0F1234u) || kr[5] != 0 || kr[6] != 0x0100 || kr[WIDTH + 5] != 1 || kr[2 * WIDTH + 5] != 2) {
    fprintf(stderr, "unexpected cells\n");
    return 6;
  }
  for (size_t r = 0; r < n; r++) {
    const uint64_t* row = got + r * WIDTH;
    int ones = 0;
    while (ones < 5 && row[ones] == 1) ones++;
    const int want = r < info.start[1] ? 0 : r < info.start[2] ? 1 : r < info.start[3] ? 2 : r < info.start[4] ? 3 : r < info.padding_start ? 4 : 5;
    if (ones != want || row[WIDTH - 1] != r + 1) {
      fprintf(stderr, "row %zu is not what it should be\n", r);
      return 6;
    }
  }

  /* the third main trace from the controller rows just written */
  mh_trace* third = NULL;
  mh_p2_trace_info p2;
  CHECK(mh_miden_poseidon2_trace(ctx, chiplets, -1, &third, &p2));
  printf("poseidon2 trace: %" PRIu64 " requests\n", p2.n_requests);
  if (p2.n_requests != info.hasher.n_requests) return 7;

  mh_trace_free(third);
  mh_trace_free(chiplets);
  mh_ctx_destroy(ctx);
  free(got);
  return 0;
}
