/* The range-check table of a statement, laid on the device, from plain C through libmidenhip: upload a trace whose value column and
 * multiplicity column were never computed and let mh_fill_range_table write both from the bus messages of the lookup program -- the
 * 16-bit values the statement looks up, ascending, gaps bridged by rows 3^k apart, the table at the end of the trace -- then read the
 * exact balance report of the filled trace.
 *
 * Input: one file of little-endian u64 words --
 *     log_n, width, lookup_column, fraction, value_column, mult_column     the range slot (instance 0)
 *     n_lookup_words
 *     lookup blob ("MHLKP001")
 *     trace[2^log_n][width]                                                row-major
 * Exit 0: the table is laid and every bus balances.  Exit 1: the table does not fit the trace (the rows it needs are printed), or a
 * looked-up value is no 16-bit value (the unmatched denominators are printed).  tests/test_gpu_range_table_c_abi.py runs it on a
 * three-column test AIR.
 *
 *   gcc -O2 -Wall -Werror -Iinclude examples/range_table_c_abi.c -Lmiden-vm_amd/lib -lmidenhip -Wl,-rpath,$PWD/miden-vm_amd/lib -o range_table
 *   ./range_table statement.bin
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
  uint64_t* head = read_words(f, 7);
  const int log_n = (int)head[0];
  const size_t width = (size_t)head[1], n_lookup = (size_t)head[6];
  if (log_n < 1 || log_n > 24 || width < 2 || width > 1024 || head[4] >= width || head[5] >= width) {
    fprintf(stderr, "log height outside 1..24 or a column outside the trace\n");
    return 2;
  }
  const mh_range_slot slot = {0, (uint32_t)head[2], (uint32_t)head[3], (uint32_t)head[4], (uint32_t)head[5]};
  uint64_t* lookup_blob = read_words(f, n_lookup);
  uint64_t* rows = read_words(f, width << log_n);
  fclose(f);

  mh_ctx* ctx = NULL;
  if (mh_ctx_create(0, &ctx) != MH_OK) {
    fprintf(stderr, "mh_ctx_create failed\n");
    return 3;
  }
  mh_lookup* lookup = NULL;
  mh_trace* trace = NULL;
  CHECK(mh_lookup_load(ctx, lookup_blob, n_lookup, &lookup));
  CHECK(mh_trace_upload(ctx, rows, log_n, width, &trace));

  /* any full extension-field challenges do: the table does not depend on them */
  const uint64_t challenges[4] = {0x1234567890abcdefULL, 0x0fedcba987654321ULL, 3141592653589793ULL, 2718281828459045ULL};
  const mh_lookup* lookups[1] = {lookup};
  mh_trace* traces[1] = {trace};
  enum { ENTRY_CAP = 8 };
  mh_balance_entry entries[ENTRY_CAP];
  mh_range_table_info info;
  uint64_t written = 0;
  size_t n_entries = 0, n_pushes = 0;
  int rc = mh_fill_range_table(ctx, 1, lookups, traces, NULL, challenges, 2, NULL, NULL, 0, &slot, &info, &written, entries, ENTRY_CAP, &n_entries,
                               NULL, 0, &n_pushes);
  if (rc == MH_ERR_INVALID && info.rows_needed > info.rows_available) {
    printf("the table of %" PRIu64 " values needs %" PRIu64 " rows, the trace has %" PRIu64 ": nothing written\n", info.n_values, info.rows_needed,
           info.rows_available);
    return 1;
  }
  if (rc != MH_OK && rc != MH_ERR_UNSATISFIED) {
    fprintf(stderr, "mh_fill_range_table failed (%d): %s\n", rc, mh_last_error(ctx));
    return 3;
  }
  CHECK(mh_trace_download(ctx, trace, rows));
  const size_t n = (size_t)1 << log_n, first = n - (size_t)info.rows_needed;
  uint64_t total = 0;
  for (size_t r = 0; r < n; r++) total += rows[r * width + slot.mult_column];
  printf("%" PRIu64 " values in %" PRIu64 " rows, the table starts at row %zu; %" PRIu64 " multiplicity cells written, their sum %" PRIu64 "\n",
         info.n_values, info.rows_needed, first, written, total);
  printf("table:");
  for (size_t r = first; r < n; r++)
    if (rows[r * width + slot.mult_column]) printf(" %" PRIu64 "x%" PRIu64, rows[r * width + slot.value_column], rows[r * width + slot.mult_column]);
  printf("\n");
  if (rc == MH_ERR_UNSATISFIED) {
    for (size_t i = 0; i < n_entries && i < ENTRY_CAP; i++)
      printf("unmatched denominator (%" PRIu64 ", %" PRIu64 "): net (%" PRIu64 ", %" PRIu64 ") over %" PRIu64 " pushes\n", entries[i].denom[0],
             entries[i].denom[1], entries[i].net[0], entries[i].net[1], entries[i].pushes);
    printf("%zu unmatched denominators; first: %s\n", n_entries, mh_last_error(ctx));
    return 1;
  }
  printf("balanced\n");
  mh_trace_free(trace);
  mh_lookup_free(lookup);
  mh_ctx_destroy(ctx);
  free(head); free(lookup_blob); free(rows);
  return 0;
}
