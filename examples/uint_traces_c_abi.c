/* The precompile prover's UintStoreMul and UintAdd traces from plain C: a store of eight values under the modulus 97, two
 * multiply-accumulates (one subtractive, borrowing a modulus) and two additions (one wrapping) go to the device as three plain lists
 * (mh_uint_traces_build); the device divides, lays the carries, counts the readers of every stored value and writes the 44 and the 30
 * columns -- what a Rust shim does instead of running UintStoreRequires / UintMulRequires / UintAddRequires' generate_trace and
 * uploading the matrices.  The traces are the ones mh_prove_precompile_traces takes at indices 6 and 7.
 *
 *   gcc -O2 -Iinclude examples/uint_traces_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o uint_traces
 *   ./uint_traces
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include "midenhip.h"

#define CHECK(call)                                                                              \
  do {                                                                                           \
    int rc_ = (call);                                                                            \
    if (rc_ != MH_OK) {                                                                          \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ctx ? mh_last_error(ctx) : "no ctx"); \
      return 1;                                                                                  \
    }                                                                                            \
  } while (0)

enum { USM_WIDTH = 44, ADD_WIDTH = 30, N_STORE = 8, N_MUL = 2, N_ADD = 2, USM_ROWS = 32, ADD_ROWS = 4, T = 65536 };

int main(void) {
  if (sizeof(mh_uint_row) != 48 || sizeof(mh_uint_mul_op) != 40 || sizeof(mh_uint_add_op) != 32 || sizeof(mh_uint_traces_info) != 80) return 3;
  /* ptr 1: the bound 96 (modulus 97), its own bound, read once from outside; the transients from 2^16 on */
  const mh_uint_row rows[N_STORE] = {{1, 1, {96}, 1, 0},     {T, 1, {5}, 0, 0},      {T + 1, 1, {7}, 0, 0},  {T + 2, 1, {3}, 0, 0},
                                     {T + 3, 1, {73}, 0, 0}, {T + 4, 1, {59}, 0, 0}, {T + 5, 1, {12}, 0, 0}, {T + 6, 1, {35}, 0, 0}};
  /* 2 * 5 * 7 + 3 = 73;  5 * 7 - 73 = -38 = 59 - 97 */
  const mh_uint_mul_op muls[N_MUL] = {{T, T + 1, T + 2, T + 3, 1, 2, 1, 0, 1}, {T, T + 1, T + 3, T + 4, 1, 1, 1, 1, 2}};
  /* 5 + 7 = 12;  73 + 59 = 35 + 97 */
  const mh_uint_add_op adds[N_ADD] = {{T, T + 1, T + 5, 1, 0, 0, 1}, {T + 3, T + 4, T + 6, 1, 1, 0, 3}};

  /* the planner alone: host only, no context */
  uint32_t bound_index[N_STORE];
  mh_uint_traces_info plan;
  if (mh_uint_traces_plan(rows, N_STORE, muls, N_MUL, adds, N_ADD, -1, -1, bound_index, &plan) != MH_OK) return 3;
  printf("plan: %" PRIu64 " values, %" PRIu64 " multiplications, %" PRIu64 " additions; %" PRIu64 " and %" PRIu64 " rows; bound index of the last value %u\n",
         plan.n_store, plan.n_mul, plan.n_add, plan.usm_rows_needed, plan.add_rows_needed, bound_index[N_STORE - 1]);
  if (plan.usm_rows_needed != USM_ROWS || plan.add_rows_needed != ADD_ROWS) return 4;

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));

  /* a remainder that is not the canonical one is refused by the device's witness pass; the out-pointers stay as they were */
  mh_uint_mul_op bad_muls[N_MUL] = {muls[0], muls[1]};
  bad_muls[1].r = T + 2;
  mh_trace *usm = NULL, *add = NULL;
  mh_uint_traces_info bad;
  if (mh_uint_traces_build(ctx, rows, N_STORE, bad_muls, N_MUL, adds, N_ADD, -1, -1, &usm, &add, &bad) != MH_ERR_INVALID || usm || add ||
      bad.defect_section != 1 || bad.defect_kind != 10 || bad.defect_index != 1) {
    fprintf(stderr, "the wrong remainder was not refused as kind 10 at multiplication 1\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  mh_uint_traces_info info;
  CHECK(mh_uint_traces_build(ctx, rows, N_STORE, muls, N_MUL, adds, N_ADD, -1, -1, &usm, &add, &info));
  printf("uint traces: %" PRIu64 " x %d and %" PRIu64 " x %d\n", info.usm_rows, USM_WIDTH, info.add_rows, ADD_WIDTH);
  uint64_t* u = (uint64_t*)malloc((size_t)USM_ROWS * USM_WIDTH * sizeof(uint64_t));
  uint64_t* a = (uint64_t*)malloc((size_t)ADD_ROWS * ADD_WIDTH * sizeof(uint64_t));
  if (!u || !a) return 3;
  CHECK(mh_trace_download(ctx, usm, u));
  CHECK(mh_trace_download(ctx, add, a));
  /* the store's multiplicities stand on the second row of a value's block, cells 8 and 9; the multiplier's half starts at column 18:
   * the quotient on row 3 of a relation's block, the borrow in the last column; the adder's k on the closing row, cell 20 */
  printf("reads of the modulus row: %" PRIu64 " UintVal, %" PRIu64 " UintLimbs; of 73: %" PRIu64 ", %" PRIu64 "\n", u[1 * USM_WIDTH + 8], u[1 * USM_WIDTH + 9],
         u[(4 * 4 + 1) * USM_WIDTH + 8], u[(4 * 4 + 1) * USM_WIDTH + 9]);
  printf("quotients %" PRIu64 " %" PRIu64 ", borrows %" PRIu64 " %" PRIu64 ", first carries %" PRIu64 " %" PRIu64 "; k %" PRIu64 " %" PRIu64 "; last pointer %" PRIu64 "\n",
         u[3 * USM_WIDTH + 18], u[11 * USM_WIDTH + 18], u[0 * USM_WIDTH + 43], u[8 * USM_WIDTH + 43], u[5 * USM_WIDTH + 18], u[13 * USM_WIDTH + 18],
         a[1 * ADD_WIDTH + 20], a[3 * ADD_WIDTH + 20], u[(USM_ROWS - 1) * USM_WIDTH + 16]);
  if (u[1 * USM_WIDTH + 8] != 1 + 8 + 2 || u[1 * USM_WIDTH + 9] != 2 || u[8 * USM_WIDTH + 43] != 1 || a[3 * ADD_WIDTH + 20] != 1 ||
      u[(USM_ROWS - 1) * USM_WIDTH + 16] != T + 6) {
    fprintf(stderr, "unexpected cells\n");
    return 6;
  }
  mh_trace_free(add);
  mh_trace_free(usm);
  mh_ctx_destroy(ctx);
  free(a);
  free(u);
  return 0;
}
