/* The precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces from plain C: the secp256k1 group, its point at infinity,
 * G, 2 G, 3 G and three negatives, four additions (a pass-through, two chords, a cancel) and six MSM expressions (two intros, their
 * combine, three negs) go to the device as five plain lists of pointers (mh_ec_traces_build); the device checks them against each other,
 * counts who reads which group, point and expression, derives the merge cursors and writes the 6, 14, 21 and 38 columns -- what a Rust
 * shim does instead of running EcStoreRequires / EcAddRequires / EcMsmRequires' generate_trace and uploading the matrices.  The traces are
 * the ones mh_prove_precompile_traces takes at indices 8..11.
 *
 *   gcc -O2 -Iinclude examples/ec_traces_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o ec_traces
 *   ./ec_traces
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

enum { N_GROUPS = 1, N_POINTS = 7, N_ADD = 4, N_EXPRS = 6, N_TERMS = 8, T = 65536, ONE = T + 17 /* the literal 1 under the scalar bound */, MINUS_ONE = 3 /* the scalar bound's own row */ };
enum { GROUPS_W = 6, POINTS_W = 14, ADD_W = 21, MSM_W = 38, GROUPS_ROWS = 2, POINTS_ROWS = 8, ADD_ROWS = 16, MSM_ROWS = 8 };

int main(void) {
  if (sizeof(mh_ec_group) != 24 || sizeof(mh_ec_point) != 32 || sizeof(mh_ec_add_op) != 56 || sizeof(mh_msm_expr) != 48 || sizeof(mh_msm_term) != 8 ||
      sizeof(mh_ec_traces_info) != 128)
    return 3;
  /* the VM-owned curve slot: a, b, the base-field bound, the scalar bound; read once by the verifier's boundary term */
  const mh_ec_group groups[N_GROUPS] = {{8, 9, 2, 3, 1}};
  /* 1 the point at infinity (read once from outside: EcRequire.neg), 2..4 G, 2 G, 3 G with their membership trios, 5 -2 G (a member),
   * 6 -G and 7 -3 G closure-certified by the MSM's negs */
  const mh_ec_point points[N_POINTS] = {{1, 0, 0, 0, 0, 1, 1},
                                        {1, T, T + 1, T + 2, T + 3, 0, 0},
                                        {1, T + 4, T + 5, T + 6, T + 7, 0, 0},
                                        {1, T + 8, T + 9, T + 10, T + 11, 0, 0},
                                        {1, T + 4, T + 16, T + 6, T + 7, 0, 0},
                                        {1, T, T + 20, 0, 0, 2, 0},
                                        {1, T + 8, T + 21, 0, 0, 2, 0}};
  /* G + O = G (pai_q); 2 G + G = 3 G twice over (a chord, multiplicity 2); 2 G + (-2 G) = O (cancel); G + 2 G = 3 G (the combine's) */
  const mh_ec_add_op adds[N_ADD] = {{1, 2, 1, 2, 1, 0, {0, 0, 0, 0, 0, 0}, 1},
                                    {1, 3, 2, 4, 5, 0, {T + 12, T + 13, T + 14, T + 9, T + 15, T + 8}, 2},
                                    {1, 3, 5, 1, 3, 0, {0, 0, 0, 0, 0, 0}, 1},
                                    {1, 2, 3, 4, 5, 0, {T + 18, T + 13, T + 14, T + 9, T + 19, T + 8}, 1}};
  /* <G>, <2 G>, their combine, -<G> (its value point minted, resolved once), -<2 G> (onto the stored row), -(the combine) */
  const mh_msm_expr exprs[N_EXPRS] = {{0, 1, 2, 0, 0, 1, 0, 0, 0, 0}, {0, 1, 3, 0, 0, 1, 0, 0, 0, 0}, {1, 1, 4, 1, 2, 2, 0, 0, 0, 0},
                                      {2, 1, 6, 1, 0, 1, 1, 0, 0, 1}, {2, 1, 5, 2, 0, 1, 0, 0, 0, 0}, {2, 1, 7, 3, 0, 2, 1, 0, 0, 0}};
  const mh_msm_term terms[N_TERMS] = {{2, ONE}, {3, ONE}, {2, ONE}, {3, ONE}, {2, MINUS_ONE}, {3, MINUS_ONE}, {2, MINUS_ONE}, {3, MINUS_ONE}};

  /* the planner alone: host only, no context */
  uint32_t row_start[N_EXPRS];
  mh_ec_traces_info plan;
  if (mh_ec_traces_plan(groups, N_GROUPS, points, N_POINTS, adds, N_ADD, exprs, N_EXPRS, terms, N_TERMS, -1, -1, -1, -1, row_start, &plan) != MH_OK) return 3;
  printf("plan: %" PRIu64 " x %" PRIu64 " x %" PRIu64 " x %" PRIu64 " rows; the last expression starts at row %u\n", plan.groups_rows_needed,
         plan.points_rows_needed, plan.add_rows_needed, plan.msm_rows_needed, row_start[N_EXPRS - 1]);
  if (plan.groups_rows_needed != GROUPS_ROWS || plan.points_rows_needed != POINTS_ROWS || plan.add_rows_needed != ADD_ROWS || plan.msm_rows_needed != MSM_ROWS)
    return 4;

  mh_ctx* ctx = NULL;
  CHECK(mh_ctx_create(0, &ctx));

  /* a pass-through (Q at infinity) recorded as a chord is refused by the device's checking pass; the out-pointers stay as they were */
  mh_ec_add_op bad_adds[N_ADD] = {adds[0], adds[1], adds[2], adds[3]};
  bad_adds[0].kind = 5;
  mh_trace *tg = NULL, *tp = NULL, *ta = NULL, *tm = NULL;
  mh_ec_traces_info bad;
  if (mh_ec_traces_build(ctx, groups, N_GROUPS, points, N_POINTS, bad_adds, N_ADD, exprs, N_EXPRS, terms, N_TERMS, -1, -1, -1, -1, &tg, &tp, &ta, &tm,
                         &bad) != MH_ERR_INVALID ||
      tg || tp || ta || tm || bad.defect_section != 2 || bad.defect_kind != 11 || bad.defect_index != 0) {
    fprintf(stderr, "the pass-through recorded as a chord was not refused as kind 11 at addition 0\n");
    return 4;
  }
  printf("refused: %s\n", mh_last_error(ctx));

  mh_ec_traces_info info;
  CHECK(mh_ec_traces_build(ctx, groups, N_GROUPS, points, N_POINTS, adds, N_ADD, exprs, N_EXPRS, terms, N_TERMS, -1, -1, -1, -1, &tg, &tp, &ta, &tm, &info));
  printf("ec traces: %" PRIu64 " x %d, %" PRIu64 " x %d, %" PRIu64 " x %d, %" PRIu64 " x %d\n", info.groups_rows, GROUPS_W, info.points_rows, POINTS_W,
         info.add_rows, ADD_W, info.msm_rows, MSM_W);
  uint64_t* g = (uint64_t*)malloc((size_t)GROUPS_ROWS * GROUPS_W * sizeof(uint64_t));
  uint64_t* p = (uint64_t*)malloc((size_t)POINTS_ROWS * POINTS_W * sizeof(uint64_t));
  uint64_t* a = (uint64_t*)malloc((size_t)ADD_ROWS * ADD_W * sizeof(uint64_t));
  uint64_t* m = (uint64_t*)malloc((size_t)MSM_ROWS * MSM_W * sizeof(uint64_t));
  if (!g || !p || !a || !m) return 3;
  CHECK(mh_trace_download(ctx, tg, g));
  CHECK(mh_trace_download(ctx, tp, p));
  CHECK(mh_trace_download(ctx, ta, a));
  CHECK(mh_trace_download(ctx, tm, m));
  /* the group's demand in column 5; a point's in column 11; the adder's case flags in columns 10..14; the MSM's mult in column 9, its
   * cursors i, j in 14, 15, the takes in 16..18 and neg's coordinates in 33, 35, 36 on a boundary row */
  printf("reads of the group: %" PRIu64 "; of the point at infinity, G, 2 G: %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g[5], p[0 * POINTS_W + 11],
         p[1 * POINTS_W + 11], p[2 * POINTS_W + 11]);
  printf("case flags of the four additions:");
  for (int i = 0; i < N_ADD; i++)
    printf(" %" PRIu64 "%" PRIu64 "%" PRIu64 "%" PRIu64 "%" PRIu64, a[4 * i * ADD_W + 10], a[4 * i * ADD_W + 11], a[4 * i * ADD_W + 12], a[4 * i * ADD_W + 13],
           a[4 * i * ADD_W + 14]);
  printf("\nuses of the expressions:");
  for (int k = 0; k < N_EXPRS; k++) printf(" %" PRIu64, m[row_start[k] * MSM_W + 9]);
  printf("\nthe combine's rows: i j takes %" PRIu64 " %" PRIu64 " %" PRIu64 "%" PRIu64 "%" PRIu64 " | %" PRIu64 " %" PRIu64 " %" PRIu64 "%" PRIu64 "%" PRIu64
         "; the last neg's x, y, -y: %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
         m[2 * MSM_W + 14], m[2 * MSM_W + 15], m[2 * MSM_W + 16], m[2 * MSM_W + 17], m[2 * MSM_W + 18], m[3 * MSM_W + 14], m[3 * MSM_W + 15], m[3 * MSM_W + 16],
         m[3 * MSM_W + 17], m[3 * MSM_W + 18], m[7 * MSM_W + 33], m[7 * MSM_W + 35], m[7 * MSM_W + 36]);
  if (g[5] != 1 + 7 + 3 + 4 || p[0 * POINTS_W + 11] != 1 + 2 || a[8 * ADD_W + 12] != 1 || m[0 * MSM_W + 9] != 2 || m[3 * MSM_W + 15] != 0 ||
      m[7 * MSM_W + 36] != T + 21) {
    fprintf(stderr, "unexpected cells\n");
    return 6;
  }
  mh_trace_free(tm);
  mh_trace_free(ta);
  mh_trace_free(tp);
  mh_trace_free(tg);
  mh_ctx_destroy(ctx);
  free(m);
  free(a);
  free(p);
  free(g);
  return 0;
}
