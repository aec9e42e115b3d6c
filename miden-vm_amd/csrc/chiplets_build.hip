// The whole chiplets trace built on the device from the five lists of an executed program (mh_miden_chiplets_build), and its frame
// (mh_miden_chiplets_frame), gfx950.
//
// Replaces Chiplets::fill_trace (processor/src/trace/chiplets/mod.rs:58-73, 134-173, 213-310): the five sections stacked in the order
// hasher, bitwise, memory, ACE, kernel ROM, each behind its selector prefix, at least one padding row with five selector ones, and
// chip_clk = row + 1 in the last column.
//   frame   a lane per row: column 21 := row + 1; from padding_start on also columns 0..4 := 1 and columns 5..20 := 0.  Column-major
//           stores, consecutive lanes on consecutive rows; no other cell is touched.
// The build allocates the trace, zero-fills it, calls the five in-place builders (hasher_section.hip, bitwise_section.hip,
// memory_section.hip, ace_section.hip, kernel_rom_section.hip) at the starts it has computed and enqueues the frame.
#include "section_out.cuh"

u64 kernel_rom_count_rows(mh_ctx* c, const uint64_t* procs, size_t n_procs);  // kernel_rom_section.hip

namespace {
constexpr int CB_BT = 256;
constexpr int CB_CLK = 21;
}  // namespace

__global__ __launch_bounds__(CB_BT) void k_cb_frame(u64* __restrict__ base, u64 height, u64 padding_start) {
  const u64 r = (u64)blockIdx.x * CB_BT + threadIdx.x;
  if (r >= height) return;
  base[(size_t)CB_CLK * height + r] = r + 1;
  if (r >= padding_start) {
#pragma unroll
    for (int i = 0; i < CB_CLK; i++) base[(size_t)i * height + r] = i < 5;
  }
}

namespace {
void cb_frame(mh_ctx* c, mh_trace* t, u64 padding_start) {
  const u64 height = (u64)1 << t->log_n;
  ProfScope ps(c, "cb_frame", 8.0 * (double)height + 168.0 * (double)(height - padding_start));
  MH_LAUNCH(k_cb_frame, dim3(sec_grid(height, CB_BT)), dim3(CB_BT), 0, c->stream, t->cols.u(), height, padding_start);
}

// rows of the hasher section by the ops' headers as they stand: 0 for an unknown kind
u64 cb_hasher_rows(const mh_hash_op* ops, size_t n) {
  u64 perms = 0;
  for (size_t i = 0; i < n; i++) perms += ops[i].kind < 2 ? 1 : ops[i].kind == 2 || ops[i].kind == 3 ? ops[i].count : ops[i].kind == 4 ? 2 * (u64)ops[i].count : 0;
  return (2 * perms + 7) & ~(u64)7;
}

struct CbRefused {
  int rc;
};
}  // namespace

extern "C" int mh_miden_chiplets_frame(mh_ctx* c, mh_trace* chiplets, uint64_t padding_start) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    sec_require_chiplets(c, chiplets, "mh_miden_chiplets_frame");
    MH_REQUIRE(padding_start <= ((u64)1 << chiplets->log_n), "mh_miden_chiplets_frame: padding_start lies beyond the trace");
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    cb_frame(c, chiplets, padding_start);
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_miden_chiplets_build(mh_ctx* c, const mh_chiplets_lists* l, int log_n, mh_trace** out, mh_chiplets_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_chiplets_info local;
  if (!info) info = &local;
  try {
    const char* entry = "mh_miden_chiplets_build";
    if (out) *out = nullptr;
    *info = mh_chiplets_info{};
    info->log_n = log_n;
    info->defect_section = -1;
    MH_REQUIRE(out && l, "mh_miden_chiplets_build: null argument");
    MH_REQUIRE((l->hash_ops || !l->n_hash_ops) && (l->hash_felts || !l->n_hash_felts) && (l->bitwise_ops || !l->n_bitwise_ops) &&
                   (l->mem_accesses || !l->n_mem_accesses) && (l->ace_evals || !l->n_ace_evals) && (l->ace_felts || !l->n_ace_felts) &&
                   (l->kernel_procs || !l->n_kernel_procs) && (l->kernel_calls || !l->n_kernel_calls),
               "mh_miden_chiplets_build: null list");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_miden_chiplets_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(l->n_hash_ops <= SEC_MAX_ROWS && l->n_bitwise_ops <= SEC_MAX_ROWS / 8 && l->n_mem_accesses <= SEC_MAX_ROWS && l->n_ace_evals <= SEC_MAX_ROWS,
               "mh_miden_chiplets_build: a list of more than 2^24 rows");
    HIP_CHECK(hipSetDevice(c->device));
    u64 rows[5];
    rows[0] = cb_hasher_rows(l->hash_ops, l->n_hash_ops);
    rows[1] = 8 * (u64)l->n_bitwise_ops;
    rows[2] = l->n_mem_accesses;
    rows[3] = 0;
    for (size_t i = 0; i < l->n_ace_evals; i++) rows[3] += (u64)l->ace_evals[i].num_vars / 2 + l->ace_evals[i].num_eval;
    rows[4] = kernel_rom_count_rows(c, l->kernel_procs, l->n_kernel_procs);  // a wait, for two procedures and more
    u64 at = 0;
    for (int s = 0; s < 5; s++) {
      info->start[s] = at;
      at += rows[s];  // five terms below 2^36
    }
    info->padding_start = at;
    info->trace_len = at + 1;
    if (log_n < 0) log_n = sec_log_n(info->trace_len);
    info->log_n = log_n;
    if (info->trace_len > ((u64)1 << log_n)) {
      info->defect_section = 5;
      info->defect = 1;
      info->defect_index = info->trace_len;
      char buf[160];
      snprintf(buf, sizeof buf, "%s: the trace does not fit: %llu rows with the padding row, 2^%d at hand", entry, (unsigned long long)info->trace_len, log_n);
      throw MhError(MH_ERR_INVALID, buf);
    }
    const u64 height = (u64)1 << log_n;
    std::unique_ptr<mh_trace> t = trace_new(c, log_n, SEC_CHIPLETS_WIDTH);
    HIP_CHECK(hipMemsetAsync(t->cols.p, 0, height * SEC_CHIPLETS_WIDTH * 8, c->stream));
    // a builder's refusal has filled its info and the context's error text: hand both on
    auto section = [&](int s, int rc, int defect, u64 index, u64 got_rows) {
      if (rc != MH_OK) {
        info->defect_section = s;
        info->defect = defect;
        info->defect_index = index;
        throw CbRefused{rc};
      }
      MH_REQUIRE(got_rows == rows[s], std::string(entry) + ": internal error, a section has other rows than its headers say");
    };
    int rc = mh_miden_hasher_section(c, t.get(), l->hash_ops, l->n_hash_ops, l->hash_felts, l->n_hash_felts, nullptr, &info->hasher);
    section(0, rc, info->hasher.defect, info->hasher.defect_index, info->hasher.n_rows);
    rc = mh_miden_bitwise_section(c, t.get(), info->start[1], l->bitwise_ops, l->n_bitwise_ops, nullptr, &info->bitwise);
    section(1, rc, info->bitwise.defect, info->bitwise.defect_index, info->bitwise.n_rows);
    rc = mh_miden_memory_section(c, t.get(), info->start[2], l->mem_accesses, l->n_mem_accesses, nullptr, &info->memory);
    section(2, rc, info->memory.defect, info->memory.defect_index, info->memory.n_rows);
    rc = mh_miden_ace_section(c, t.get(), info->start[3], l->ace_evals, l->n_ace_evals, l->ace_felts, l->n_ace_felts, &info->ace);
    section(3, rc, info->ace.defect, info->ace.defect_index, info->ace.n_rows);
    rc = mh_miden_kernel_rom_section(c, t.get(), info->start[4], l->kernel_procs, l->n_kernel_procs, l->kernel_calls, l->n_kernel_calls, nullptr,
                                     &info->kernel_rom);
    section(4, rc, info->kernel_rom.defect, info->kernel_rom.defect_index, info->kernel_rom.n_rows);
    cb_frame(c, t.get(), info->padding_start);
    *out = t.release();
    return MH_OK;
  } catch (const CbRefused& r) {
    return r.rc;  // c->err is the builder's
  }
  SEC_CATCH
}
