// The kernel ROM's trace section built on the device (mh_kernel_rom_section_build, mh_miden_kernel_rom_section), gfx950.
//
// Replaces KernelRom (processor/src/trace/chiplets/kernel_rom/mod.rs): a map from the procedure digests' bytes to call counts, walked in
// key order.  At most 255 procedures, so one block holds the table:
//   sort    one block.  A digest goes into LDS as four byte-reversed canonical words, so that comparing the words as unsigned numbers
//           from h0 to h3 is the lexicographic comparison of the 32 little-endian bytes.  A lane per digest counts the digests below
//           its own (ties by declaration index): its place.  A digest that equals its left neighbour is a declared duplicate; the
//           number of run heads left of a digest is its row.  The distinct digests, in row order -> table[], their number -> words.
//   calls   a lane per call, the table in LDS: binary search, one LDS integer atomic on the row's count, the block's counts added to
//           the global ones at the end; a call that finds no row -> atomicMin of its index.  The host reads the words back: the wait.
//   rows    a lane per row: m | h0..h3, column-major stores.
// Integer sums and minima: no output depends on the order the atomics land in.
#include "section_out.cuh"

namespace {
constexpr int KR_BT = 256;
constexpr int KR_WIDTH = 5;
constexpr u32 KR_MAX_PROCS = 255;
constexpr unsigned long long KR_NONE = ~0ull;

struct KrWords {  // what the host reads back
  unsigned long long n_rows;
  unsigned long long miss;  // lowest call of an undeclared digest
};

struct KrKey {
  u64 w[4];  // byte-reversed canonical felts
};

__device__ __forceinline__ u64 kr_bswap(u64 x) { return __builtin_bswap64(x); }

__device__ __forceinline__ KrKey kr_key(const u64* d) {
  KrKey k;
#pragma unroll
  for (int i = 0; i < 4; i++) k.w[i] = kr_bswap(gl_canon(d[i]));
  return k;
}

// -1, 0, 1
__device__ __forceinline__ int kr_cmp(const KrKey& a, const KrKey& b) {
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
}  // namespace

// one block; n <= KR_MAX_PROCS.  table: [n] keys of the distinct digests in row order
__global__ __launch_bounds__(KR_BT) void k_kr_sort(const u64* __restrict__ procs, u32 n, KrKey* __restrict__ table, KrWords* w) {
  __shared__ KrKey s_in[KR_BT], s_sorted[KR_BT];
  __shared__ u32 s_head[KR_BT];
  const u32 i = threadIdx.x;
  KrKey mine{};
  if (i < n) {
    mine = kr_key(procs + 4 * (size_t)i);
    s_in[i] = mine;
  }
  __syncthreads();
  if (i < n) {
    u32 place = 0;
    for (u32 j = 0; j < n; j++) {
      const int cmp = kr_cmp(s_in[j], mine);
      place += cmp < 0 || (cmp == 0 && j < i);
    }
    s_sorted[place] = mine;  // a permutation of 0 .. n - 1
  }
  __syncthreads();
  if (i < n) s_head[i] = i == 0 || kr_cmp(s_sorted[i - 1], s_sorted[i]) != 0;
  __syncthreads();
  if (i < n && s_head[i]) {
    u32 row = 0;
    for (u32 j = 0; j < i; j++) row += s_head[j];
    table[row] = s_sorted[i];
  }
  if (i == 0) {
    u32 rows = 0;
    for (u32 j = 0; j < n; j++) rows += s_head[j];
    w->n_rows = rows;
  }
}

// n_rows is read from the words the sort left
__global__ __launch_bounds__(KR_BT) void k_kr_calls(const u64* __restrict__ calls, u64 n_calls, const KrKey* __restrict__ table, KrWords* w,
                                                    u32* __restrict__ counts) {
  __shared__ KrKey s_table[KR_BT];
  __shared__ u32 s_count[KR_BT];
  u32 n_rows = (u32)w->n_rows;
  if (n_rows > KR_MAX_PROCS) n_rows = KR_MAX_PROCS;  // never
  if (threadIdx.x < n_rows) s_table[threadIdx.x] = table[threadIdx.x];
  s_count[threadIdx.x] = 0;
  __syncthreads();
  const u64 call = (u64)blockIdx.x * KR_BT + threadIdx.x;
  if (call < n_calls) {
    const KrKey k = kr_key(calls + 4 * (size_t)call);
    u32 lo = 0, hi = n_rows;  // the first row whose key is not below k
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (kr_cmp(s_table[mid], k) < 0) lo = mid + 1;
      else hi = mid;
    }
    if (lo < n_rows && kr_cmp(s_table[lo], k) == 0) atomicAdd(&s_count[lo], 1u);
    else atomicMin(&w->miss, (unsigned long long)call);
  }
  __syncthreads();
  if (threadIdx.x < n_rows && s_count[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_count[threadIdx.x]);
}

__global__ __launch_bounds__(KR_BT) void k_kr_rows(const KrKey* __restrict__ table, const u32* __restrict__ counts, u32 n_rows, SecOut o,
                                                   u64* __restrict__ digests) {
  const u32 r = threadIdx.x;
  if (r >= n_rows) return;
  const KrKey k = table[r];
  u64 row[KR_WIDTH];
  row[0] = counts[r];
#pragma unroll
  for (int i = 0; i < 4; i++) row[1 + i] = kr_bswap(k.w[i]);
  sec_store_row(o, r, row);
  if (digests) {
#pragma unroll
    for (int i = 0; i < 4; i++) digests[4 * (size_t)r + i] = row[1 + i];
  }
}

namespace {
void kr_fill_info(mh_kernel_rom_section_info* info, u64 rows, u64 calls, int log_n, int defect, u64 index) {
  if (!info) return;
  info->n_rows = rows;
  info->n_calls = calls;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_index = index;
}

[[noreturn]] void kr_refuse(mh_kernel_rom_section_info* info, u64 calls, int log_n, int defect, u64 index, const char* entry) {
  kr_fill_info(info, 0, calls, log_n, defect, index);
  char buf[256];
  if (defect == 1)
    snprintf(buf, sizeof buf, "%s: defect 1, call %llu names a digest that no kernel procedure has (SyscallTargetNotInKernel)", entry,
             (unsigned long long)index);
  else
    snprintf(buf, sizeof buf, "%s: defect 2, the section does not fit: row %llu is the first without room", entry, (unsigned long long)index);
  throw MhError(MH_ERR_INVALID, buf);
}

struct KrTarget {
  virtual ~KrTarget() {}
  virtual u64 cap_rows() const = 0;                     // rows the target has; ~0 when it is sized by the section
  virtual SecOut resolve(u64 n_rows, int* log_n) = 0;   // called once the section is known to fit
};

// n_procs <= 255.  Returns after the read-back with the rows kernel enqueued, or after the copy of the digests
void kr_run(mh_ctx* c, const uint64_t* procs, size_t n_procs, const uint64_t* calls, size_t n_calls, KrTarget& target, int shown_log_n,
            uint64_t* digests, mh_kernel_rom_section_info* info, const char* entry) {
  DevBuf dprocs((n_procs ? n_procs : 1) * 32), dcalls((n_calls ? n_calls : 1) * 32), words(sizeof(KrWords));
  DevBuf table(KR_BT * sizeof(KrKey)), counts(KR_BT * 4), ddig(digests ? KR_BT * 32 : 0);
  KrWords* dw = (KrWords*)words.p;
  const KrWords init{0, KR_NONE};
  c->h2d(words.p, &init, sizeof init);
  if (n_procs) c->h2d(dprocs.p, procs, n_procs * 32);
  if (n_calls) c->h2d(dcalls.p, calls, n_calls * 32);
  HIP_CHECK(hipMemsetAsync(counts.p, 0, KR_BT * 4, c->stream));
  if (n_procs) {
    ProfScope ps(c, "kr_sort", 64.0 * (double)n_procs);
    MH_LAUNCH(k_kr_sort, dim3(1), dim3(KR_BT), 0, c->stream, dprocs.u(), (u32)n_procs, (KrKey*)table.p, dw);
  }
  if (n_calls) {
    ProfScope ps(c, "kr_calls", 32.0 * (double)n_calls);
    MH_LAUNCH(k_kr_calls, dim3(sec_grid(n_calls, KR_BT)), dim3(KR_BT), 0, c->stream, dcalls.u(), (u64)n_calls, (const KrKey*)table.p, dw, (u32*)counts.p);
  }
  KrWords w;
  c->d2h(&w, words.p, sizeof w);  // the wait: the row count and the undeclared call, before anything but scratch is written
  const u64 n_rows = w.n_rows;
  if (shown_log_n < 0) shown_log_n = sec_log_n(n_rows);
  MH_REQUIRE(n_rows <= n_procs, std::string(entry) + ": internal error, more rows than procedures");
  if (w.miss != KR_NONE) kr_refuse(info, n_calls, shown_log_n, 1, w.miss, entry);
  if (n_rows > target.cap_rows()) kr_refuse(info, n_calls, shown_log_n, 2, target.cap_rows(), entry);
  int log_n = shown_log_n;
  const SecOut o = target.resolve(n_rows, &log_n);
  if (n_rows) {
    ProfScope ps(c, "kr_rows", 72.0 * (double)n_rows);
    MH_LAUNCH(k_kr_rows, dim3(1), dim3(KR_BT), 0, c->stream, (const KrKey*)table.p, (const u32*)counts.p, (u32)n_rows, o,
              digests ? ddig.u() : nullptr);
  }
  if (digests && n_rows) c->d2h(digests, ddig.p, n_rows * 32);
  kr_fill_info(info, n_rows, n_calls, log_n, 0, 0);
}

struct KrBuildTarget : KrTarget {
  mh_ctx* c;
  int log_n;  // -1: sized by the section
  std::unique_ptr<mh_trace> t;
  KrBuildTarget(mh_ctx* ctx, int l) : c(ctx), log_n(l) {}
  u64 cap_rows() const override { return log_n < 0 ? ~(u64)0 : (u64)1 << log_n; }
  SecOut resolve(u64 n_rows, int* out_log_n) override {
    const int l = log_n < 0 ? sec_log_n(n_rows) : log_n;
    t = sec_new_trace(c, l, KR_WIDTH, n_rows);
    *out_log_n = l;
    return SecOut{t->cols.u(), (u64)1 << l, 0, 0, -1};
  }
};

struct KrChipletsTarget : KrTarget {
  mh_trace* chiplets;
  u64 start_row;
  KrChipletsTarget(mh_trace* t, u64 s) : chiplets(t), start_row(s) {}
  u64 cap_rows() const override { return ((u64)1 << chiplets->log_n) - start_row; }
  SecOut resolve(u64, int* out_log_n) override {
    *out_log_n = chiplets->log_n;
    return SecOut{chiplets->cols.u(), (u64)1 << chiplets->log_n, start_row, 5, 4};
  }
};
}  // namespace

// the number of distinct digests among procs[0 .. n_procs): what mh_miden_chiplets_build needs before it can place the sections
u64 kernel_rom_count_rows(mh_ctx* c, const uint64_t* procs, size_t n_procs) {
  MH_REQUIRE(n_procs <= KR_MAX_PROCS, "mh_miden_chiplets_build: more than 255 kernel procedures");
  if (n_procs < 2) return n_procs;
  DevBuf dprocs(n_procs * 32), words(sizeof(KrWords)), table(KR_BT * sizeof(KrKey));
  const KrWords init{0, KR_NONE};
  c->h2d(words.p, &init, sizeof init);
  c->h2d(dprocs.p, procs, n_procs * 32);
  {
    ProfScope ps(c, "kr_sort", 64.0 * (double)n_procs);
    MH_LAUNCH(k_kr_sort, dim3(1), dim3(KR_BT), 0, c->stream, dprocs.u(), (u32)n_procs, (KrKey*)table.p, (KrWords*)words.p);
  }
  KrWords w;
  c->d2h(&w, words.p, sizeof w);
  return w.n_rows;
}

extern "C" int mh_kernel_rom_section_build(mh_ctx* c, const uint64_t* procs, size_t n_procs, const uint64_t* calls, size_t n_calls, int log_n,
                                           mh_trace** out, uint64_t* digests, mh_kernel_rom_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_kernel_rom_section_build";
    if (out) *out = nullptr;
    kr_fill_info(info, 0, n_calls, log_n, 0, 0);
    MH_REQUIRE(out && (procs || !n_procs) && (calls || !n_calls), "mh_kernel_rom_section_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_kernel_rom_section_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(n_procs <= KR_MAX_PROCS, "mh_kernel_rom_section_build: more than 255 kernel procedures");
    MH_REQUIRE(n_calls <= 0xFFFFFFFFull, "mh_kernel_rom_section_build: more than 2^32 - 1 calls");
    HIP_CHECK(hipSetDevice(c->device));
    KrBuildTarget target(c, log_n);
    kr_run(c, procs, n_procs, calls, n_calls, target, log_n, digests, info, entry);
    *out = target.t.release();
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_miden_kernel_rom_section(mh_ctx* c, mh_trace* chiplets, uint64_t start_row, const uint64_t* procs, size_t n_procs,
                                           const uint64_t* calls, size_t n_calls, uint64_t* digests, mh_kernel_rom_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_miden_kernel_rom_section";
    kr_fill_info(info, 0, n_calls, 0, 0, 0);
    MH_REQUIRE((procs || !n_procs) && (calls || !n_calls), "mh_miden_kernel_rom_section: null argument");
    sec_require_chiplets(c, chiplets, entry);
    MH_REQUIRE(n_procs <= KR_MAX_PROCS, "mh_miden_kernel_rom_section: more than 255 kernel procedures");
    MH_REQUIRE(n_calls <= 0xFFFFFFFFull, "mh_miden_kernel_rom_section: more than 2^32 - 1 calls");
    const int log_n = chiplets->log_n;
    kr_fill_info(info, 0, n_calls, log_n, 0, 0);
    if (start_row > ((u64)1 << log_n)) kr_refuse(info, n_calls, log_n, 2, 0, entry);
    if (!n_procs && !n_calls) return MH_OK;
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    KrChipletsTarget target(chiplets, start_row);
    kr_run(c, procs, n_procs, calls, n_calls, target, log_n, digests, info, entry);
    return MH_OK;
  }
  SEC_CATCH
}
