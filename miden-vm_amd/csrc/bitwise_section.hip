// The bitwise chiplet's trace section built on the device from an op list (mh_bitwise_section_build, mh_miden_bitwise_section), gfx950.
//
// Replaces Bitwise::fill_trace (processor/src/trace/chiplets/bitwise/mod.rs): 8 rows per operation, 4 bits per row from the most
// significant nibble, the result accumulated a nibble a row.
//   rows   a lane per row: the op of row r is r >> 3, its shift 28 - 4 (r & 7); prev and result are prefixes of the op's 32-bit result, so
//          no row waits for another.  13 column-major stores (+ the two selectors in place), consecutive lanes on consecutive rows; the
//          lane of an op's last row also writes the op's result when the caller wants it.
// The one defect of an op (op > 1) is found by a pass over the host list before the launch; nothing is computed on the host.
#include "section_out.cuh"

static_assert(sizeof(mh_bitwise_op) == 12, "mh_bitwise_op is 12 bytes");

namespace {
constexpr int BW_BT = 256;
constexpr int BW_WIDTH = 13;
}  // namespace

__global__ __launch_bounds__(BW_BT) void k_bw_rows(const mh_bitwise_op* __restrict__ ops, u64 n_rows, SecOut o, u32* __restrict__ results) {
  const u64 r = (u64)blockIdx.x * BW_BT + threadIdx.x;
  if (r >= n_rows) return;
  const mh_bitwise_op op = ops[r >> 3];
  const u32 i = (u32)r & 7, off = 28 - 4 * i;
  const u32 full = op.op ? op.a ^ op.b : op.a & op.b;
  const u32 aa = op.a >> off, ba = op.b >> off;
  const u32 result = full >> off, prev = i ? full >> (off + 4) : 0;  // off + 4 <= 28 for i >= 1
  const u64 row[BW_WIDTH] = {op.op, aa, ba, aa & 1, (aa >> 1) & 1, (aa >> 2) & 1, (aa >> 3) & 1, ba & 1, (ba >> 1) & 1, (ba >> 2) & 1,
                             (ba >> 3) & 1, prev, result};
  sec_store_row(o, r, row);
  if (results && i == 7) results[r >> 3] = full;
}

namespace {
void bw_fill_info(mh_bitwise_section_info* info, u64 rows, int log_n, int defect, u64 index) {
  if (!info) return;
  info->n_rows = rows;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_index = index;
}

[[noreturn]] void bw_refuse(mh_bitwise_section_info* info, int log_n, int defect, u64 index, const mh_bitwise_op* ops, const char* entry) {
  bw_fill_info(info, 0, log_n, defect, index);
  char buf[256];
  if (defect == 1)
    snprintf(buf, sizeof buf, "%s: defect 1, op %llu has op %u (0 AND, 1 XOR)", entry, (unsigned long long)index, ops[index].op);
  else
    snprintf(buf, sizeof buf, "%s: defect 2, the section does not fit: op %llu is the first without its rows", entry, (unsigned long long)index);
  throw MhError(MH_ERR_INVALID, buf);
}

void bw_check_ops(mh_bitwise_section_info* info, int log_n, const mh_bitwise_op* ops, size_t n_ops, const char* entry) {
  for (size_t i = 0; i < n_ops; i++)
    if (ops[i].op > 1) bw_refuse(info, log_n, 1, i, ops, entry);
}

// n_ops >= 1, the target has room.  Returns with the kernel enqueued, or after the copy of the results
void bw_run(mh_ctx* c, const mh_bitwise_op* ops, size_t n_ops, SecOut o, uint32_t* results) {
  const u64 n_rows = 8 * (u64)n_ops;
  DevBuf dops(n_ops * sizeof(mh_bitwise_op)), dres(results ? n_ops * 4 : 0);
  c->h2d(dops.p, ops, n_ops * sizeof(mh_bitwise_op));
  {
    ProfScope ps(c, "bw_rows", (1.5 + 8.0 * BW_WIDTH) * (double)n_rows);
    MH_LAUNCH(k_bw_rows, dim3(sec_grid(n_rows, BW_BT)), dim3(BW_BT), 0, c->stream, (const mh_bitwise_op*)dops.p, n_rows, o,
              results ? (u32*)dres.p : nullptr);
  }
  if (results) c->d2h(results, dres.p, n_ops * 4);
}
}  // namespace

extern "C" int mh_bitwise_section_build(mh_ctx* c, const mh_bitwise_op* ops, size_t n_ops, int log_n, mh_trace** out, uint32_t* results,
                                        mh_bitwise_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_bitwise_section_build";
    if (out) *out = nullptr;
    bw_fill_info(info, 0, log_n, 0, 0);
    MH_REQUIRE(out && (ops || !n_ops), "mh_bitwise_section_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_bitwise_section_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(n_ops <= SEC_MAX_ROWS / 8, "mh_bitwise_section_build: more than 2^24 rows");
    const u64 n_rows = 8 * (u64)n_ops;
    if (log_n < 0) log_n = sec_log_n(n_rows);
    bw_check_ops(info, log_n, ops, n_ops, entry);
    const u64 height = (u64)1 << log_n;
    if (n_rows > height) bw_refuse(info, log_n, 2, height / 8, ops, entry);
    HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<mh_trace> t = sec_new_trace(c, log_n, BW_WIDTH, n_rows);
    if (n_ops) bw_run(c, ops, n_ops, SecOut{t->cols.u(), height, 0, 0, -1}, results);
    bw_fill_info(info, n_rows, log_n, 0, 0);
    *out = t.release();
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_miden_bitwise_section(mh_ctx* c, mh_trace* chiplets, uint64_t start_row, const mh_bitwise_op* ops, size_t n_ops,
                                        uint32_t* results, mh_bitwise_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_miden_bitwise_section";
    bw_fill_info(info, 0, 0, 0, 0);
    MH_REQUIRE(ops || !n_ops, "mh_miden_bitwise_section: null argument");
    sec_require_chiplets(c, chiplets, entry);
    MH_REQUIRE(n_ops <= SEC_MAX_ROWS / 8, "mh_miden_bitwise_section: more than 2^24 rows");
    const int log_n = chiplets->log_n;
    const u64 height = (u64)1 << log_n, n_rows = 8 * (u64)n_ops;
    bw_fill_info(info, 0, log_n, 0, 0);
    bw_check_ops(info, log_n, ops, n_ops, entry);
    if (start_row > height || n_rows > height - start_row) bw_refuse(info, log_n, 2, start_row < height ? (height - start_row) / 8 : 0, ops, entry);
    if (!n_ops) return MH_OK;
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    bw_run(c, ops, n_ops, SecOut{chiplets->cols.u(), height, start_row, 2, 1}, results);
    bw_fill_info(info, n_rows, log_n, 0, 0);
    return MH_OK;
  }
  SEC_CATCH
}
