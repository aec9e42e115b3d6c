// The Poseidon2 permutation trace of the Miden statement, built on the device (mh_poseidon2_trace_build, mh_miden_poseidon2_trace),
// gfx950.
//
// Replaces fill_poseidon2_permutation_trace (processor/src/trace/chiplets/hasher/trace.rs:361-408) with its
// write_poseidon2_permutation_cycle (trace.rs:279-359)
// and, for the chiplets entry, the request ledger of record_perm_request (hasher/mod.rs:469-480): the ledger is a function of the
// hasher controller's input rows, every one of which carries its perm_id.
//   scan    one lane per chiplets row.  An input row (column 0 = 0, column 1 = 1) with id = column 20: mult[id] += 1,
//           first_row[id] = min(.., row), k = max(.., id + 1), all integer atomics.  The tables have N/2 + 1 entries (an input row is
//           followed by its output row); an id beyond them is never an index: the lowest such row is kept (defect 1).
//   check   the next launch reads the tables plainly.  One lane per row: an input row whose 12 state cells differ from those of row
//           first_row[id] is a conflict, the lowest such row is kept (defect 3).  One lane per id < k: mult == 0 is a gap, the lowest
//           such id is kept (defect 2).
//   cycles  one lane per 16-row cycle: the permutation with the plain canonical round functions of poseidon2.cuh, every row boundary
//           written as write_poseidon2_permutation_cycle writes it.  Cycle c < k reads its state from chiplets row first_row[c] (or from
//           the uploaded list), c >= k is a padding cycle (zero state, zero multiplicity, perm_id = c).
// Sums, minima and maxima of integers do not depend on the order of the atomics, and the cycles kernel has one writer per cell: two
// calls on the same input leave the same bytes.
// The host reads the words of the scan back once (k sizes the output when log_n = -1, and a defect is the caller's to see before the
// trace is used); the cycles kernel is enqueued behind that and nobody waits for it.
#include "../../include/midenhip.h"
#include "ctx.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include "poseidon2.cuh"
#include <memory>
#include <string>

namespace {
constexpr int P2T_BT = 256;            // scan / check
constexpr int P2T_CHIPLETS_WIDTH = 22;
constexpr int P2T_COL_S0 = 1, P2T_COL_STATE = 4, P2T_COL_PERM_ID = 20;  // chiplets_air.py: hasher selectors 1..3, state 4..15, perm_id 20
constexpr int P2T_WIDTH = 16;          // miden_air.py: COL_WITNESS 0..2, COL_STATE 3..14, COL_PERM_ID 15
constexpr int P2T_OUT_WITNESS = 0, P2T_OUT_STATE = 3, P2T_OUT_PERM_ID = 15;
constexpr int P2T_CYCLE = 16;

// the words one call reads back
struct P2tWords {
  unsigned long long k;          // max id + 1 over the input rows with an id inside the tables
  unsigned long long n_input;    // input rows
  unsigned long long bad_row;    // lowest input row whose id lies beyond the tables (all ones: none)
  unsigned long long conflict;   // lowest input row whose state differs from its id's first row
  unsigned long long gap;        // lowest id < k nobody requested
};

struct P2tScan {
  const u64* chip;  // [22][n]
  u64 n;            // chiplets rows
  u64 table;        // entries of mult / first_row
  u32* mult;
  u32* first_row;
  P2tWords* w;
};

__device__ __forceinline__ bool p2t_is_input(const P2tScan& a, u64 r) { return a.chip[r] == 0 && a.chip[(size_t)P2T_COL_S0 * a.n + r] == 1; }
}  // namespace

__global__ __launch_bounds__(P2T_BT) void k_p2t_scan(P2tScan a) {
  __shared__ u32 sc[P2T_BT];
  const u64 r = (u64)blockIdx.x * P2T_BT + threadIdx.x;
  u32 input = 0;
  if (r < a.n && p2t_is_input(a, r)) {
    input = 1;
    const u64 id = a.chip[(size_t)P2T_COL_PERM_ID * a.n + r];
    if (id >= a.table) {
      atomicMin(&a.w->bad_row, (unsigned long long)r);
    } else {
      atomicAdd(&a.mult[id], 1u);
      atomicMin(&a.first_row[id], (u32)r);
      atomicMax(&a.w->k, (unsigned long long)(id + 1));
    }
  }
  sc[threadIdx.x] = input;
  __syncthreads();
  for (int off = P2T_BT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) sc[threadIdx.x] += sc[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sc[0]) atomicAdd(&a.w->n_input, (unsigned long long)sc[0]);
}

// a launch of its own: mult, first_row and w->k are complete
__global__ __launch_bounds__(P2T_BT) void k_p2t_check(P2tScan a) {
  const u64 t = (u64)blockIdx.x * P2T_BT + threadIdx.x;
  if (t >= a.n) return;
  if (p2t_is_input(a, t)) {
    const u64 id = a.chip[(size_t)P2T_COL_PERM_ID * a.n + t];
    if (id < a.table) {
      const u64 first = a.first_row[id];  // <= t: this row took part in the minimum
      if (first != t) {
        bool same = true;
#pragma unroll
        for (int i = 0; i < 12; i++) {
          const u64* col = a.chip + (size_t)(P2T_COL_STATE + i) * a.n;
          same = same && col[t] == col[first];
        }
        if (!same) atomicMin(&a.w->conflict, (unsigned long long)t);
      }
    }
  }
  if (t < a.w->k && a.mult[t] == 0) atomicMin(&a.w->gap, (unsigned long long)t);  // k <= table <= n
}

namespace {
struct P2tCycles {
  // the requests: either rows of the chiplets trace ...
  const u64* chip;
  u64 chip_n;
  const u32* first_row;
  const u32* mult32;
  // ... or the host list
  const u64* states;  // [k][12]
  const u64* mults;   // [k]
  u64 k;
  u64 cycles;  // n / 16
  u64 n;       // rows of the output
  u64* out;    // [16][n]
};

__device__ __forceinline__ void p2t_ext_round(u64 s[12], const unsigned long long* rc) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = p2_sbox(gl_add(s[i], rc[i]));
  p2_external_linear(s);
}
__device__ __forceinline__ u64 p2t_int_round(u64 s[12], int r) {
  const u64 w = p2_sbox(gl_add(s[0], p2c::P2_ARK_INT[r]));
  s[0] = w;
  p2_internal_linear(s);
  return w;
}

// ---- the store layout: a block's 32 cycles go through an LDS tile [15 columns][32 cycles][16 rows (+1 pad)], then every column of the
// tile leaves as 512 consecutive felts: each store instruction of the wave covers two whole 128-byte lines.  Writing, lane j holds
// cycle j and stores 8 bytes at a stride of 17 felts = 34 banks: the 16 lanes of a ds_write_b64 group fall on 16 different bank
// pairs.  The perm_id column is a function of the index and needs no tile.
constexpr int P2T_TILE_CYCLES = 32;
constexpr int P2T_TILE_STRIDE = P2T_CYCLE + 1;
constexpr int P2T_TILE_COLS = 15;
struct P2tTileSink {
  u64* tile;  // + lane * P2T_TILE_STRIDE
  __device__ __forceinline__ void put(int col, int r, u64 v) { tile[(size_t)col * P2T_TILE_CYCLES * P2T_TILE_STRIDE + r] = v; }
  __device__ __forceinline__ void state(int r, const u64 s[12]) {
#pragma unroll
    for (int i = 0; i < 12; i++) put(P2T_OUT_STATE + i, r, s[i]);
  }
  __device__ __forceinline__ void witness(int r, u64 w0, u64 w1, u64 w2) {
    put(P2T_OUT_WITNESS, r, w0);
    put(P2T_OUT_WITNESS + 1, r, w1);
    put(P2T_OUT_WITNESS + 2, r, w2);
  }
  __device__ __forceinline__ void row(int r, const u64 s[12], u64 w0, u64 w1, u64 w2) {
    state(r, s);
    witness(r, w0, w1, w2);
  }
};

// write_poseidon2_permutation_cycle (trace.rs:279-359) = miden_air.poseidon2_permutation_trace: sink.row(r, state, w0, w1, w2) per row
__device__ __forceinline__ void p2t_cycle(u64 s[12], u64 mult, P2tTileSink& sink) {
  sink.row(0, s, mult, 0, 0);
  p2_external_linear(s);
  p2t_ext_round(s, p2c::P2_ARK_EXT_INITIAL);
#pragma unroll
  for (int r = 1; r < 4; r++) {
    sink.row(r, s, 0, 0, 0);
    p2t_ext_round(s, p2c::P2_ARK_EXT_INITIAL + 12 * r);
  }
#pragma unroll 1
  for (int t = 0; t < 7; t++) {
    sink.state(4 + t, s);
    const u64 w0 = p2t_int_round(s, 3 * t), w1 = p2t_int_round(s, 3 * t + 1), w2 = p2t_int_round(s, 3 * t + 2);
    sink.witness(4 + t, w0, w1, w2);
  }
  sink.state(11, s);
  sink.witness(11, p2t_int_round(s, 21), 0, 0);
  p2t_ext_round(s, p2c::P2_ARK_EXT_TERMINAL);
#pragma unroll
  for (int r = 1; r < 4; r++) {
    sink.row(11 + r, s, 0, 0, 0);
    p2t_ext_round(s, p2c::P2_ARK_EXT_TERMINAL + 12 * r);
  }
  sink.row(15, s, mult, 0, 0);
}

// cycle c's input: canonical state and multiplicity (zero for a padding cycle)
__device__ __forceinline__ u64 p2t_load(const P2tCycles& a, u64 c, u64 s[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = 0;
  if (c >= a.k) return 0;
  if (a.states) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_canon(a.states[c * 12 + i]);
    return gl_canon(a.mults[c]);
  }
  const u64 row = a.first_row[c];
  if (row >= a.chip_n) return 0;  // a gap: the host refuses the call before this kernel is launched
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = a.chip[(size_t)(P2T_COL_STATE + i) * a.chip_n + row];
  return a.mult32[c];
}
}  // namespace

__global__ __launch_bounds__(P2T_TILE_CYCLES) void k_p2t_cycles(P2tCycles a) {
  __shared__ u64 tile[P2T_TILE_COLS * P2T_TILE_CYCLES * P2T_TILE_STRIDE];
  const u64 c0 = (u64)blockIdx.x * P2T_TILE_CYCLES, c = c0 + threadIdx.x;
  if (c < a.cycles) {
    u64 s[12];
    const u64 mult = p2t_load(a, c, s);
    P2tTileSink sink{tile + threadIdx.x * P2T_TILE_STRIDE};
    p2t_cycle(s, mult, sink);
  }
  __syncthreads();
  const u64 live = (a.cycles - c0 < P2T_TILE_CYCLES ? a.cycles - c0 : P2T_TILE_CYCLES) * P2T_CYCLE;  // rows of this block
  u64* out = a.out + c0 * P2T_CYCLE;
  for (u32 e = threadIdx.x; e < live; e += P2T_TILE_CYCLES) {
    const u32 at = (e / P2T_CYCLE) * P2T_TILE_STRIDE + e % P2T_CYCLE;
#pragma unroll
    for (int col = 0; col < P2T_TILE_COLS; col++) out[(size_t)col * a.n + e] = tile[col * P2T_TILE_CYCLES * P2T_TILE_STRIDE + at];
    out[(size_t)P2T_OUT_PERM_ID * a.n + e] = c0 + e / P2T_CYCLE;
  }
}

namespace {
unsigned p2t_grid(u64 n, u64 per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// -1: max(6, ceil log2((k + 1) * 16)); 33 when that is more than a trace can have
int p2t_min_log_n(u64 k) {
  int l = 6;
  while (l < 33 && (((u64)1 << l) >> 4) < k + 1) l++;
  return l;
}

void p2t_fill_info(mh_p2_trace_info* info, u64 k, u64 n_input, int log_n, int defect, u64 row) {
  if (!info) return;
  info->n_requests = k;
  info->n_input_rows = n_input;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_row = row;
}

[[noreturn]] void p2t_refuse(mh_p2_trace_info* info, u64 k, u64 n_input, int log_n, int defect, u64 row, const char* entry) {
  p2t_fill_info(info, k, n_input, log_n, defect, row);
  char buf[256];
  switch (defect) {
    case 1: snprintf(buf, sizeof buf, "%s: defect 1, the perm_id of controller input row %llu lies beyond the id table", entry, (unsigned long long)row); break;
    case 2: snprintf(buf, sizeof buf, "%s: defect 2, perm_id %llu is skipped (no controller input row requests it, a larger id is requested)", entry, (unsigned long long)row); break;
    case 3: snprintf(buf, sizeof buf, "%s: defect 3, controller input row %llu carries another state than the first row of its perm_id", entry, (unsigned long long)row); break;
    default: snprintf(buf, sizeof buf, "%s: defect 4, %llu requests and one padding cycle do not fit 2^%d rows (first request without a cycle: %llu)", entry,
                      (unsigned long long)k, log_n, (unsigned long long)row);
  }
  throw MhError(MH_ERR_INVALID, buf);
}

// resolves log_n (refusing defect 4) and enqueues the cycles kernel into a fresh trace
mh_trace* p2t_build(mh_ctx* c, P2tCycles a, u64 n_input, int log_n, mh_p2_trace_info* info, const char* entry) {
  if (log_n < 0) log_n = p2t_min_log_n(a.k);
  if (log_n > 32 || (((u64)1 << log_n) >> 4) < a.k + 1) {
    const int shown = log_n > 32 ? 32 : log_n;
    p2t_refuse(info, a.k, n_input, shown, 4, (((u64)1 << shown) >> 4) - 1, entry);
  }
  const u64 n = (u64)1 << log_n;
  std::unique_ptr<mh_trace> t = trace_new(c, log_n, P2T_WIDTH);
  a.n = n;
  a.cycles = n / P2T_CYCLE;
  a.out = t->cols.u();
  {
    ProfScope ps(c, "p2t_cycles", 8.0 * P2T_WIDTH * (double)n);
    MH_LAUNCH(k_p2t_cycles, dim3(p2t_grid(a.cycles, P2T_TILE_CYCLES)), dim3(P2T_TILE_CYCLES), 0, c->stream, a);
  }
  p2t_fill_info(info, a.k, n_input, log_n, 0, 0);
  return t.release();
}
}  // namespace

#define P2T_CATCH                  \
  catch (const MhError& e) {       \
    c->err = e.what();             \
    return e.code;                 \
  }                                \
  catch (const std::exception& e) { \
    c->err = e.what();             \
    return MH_ERR_INTERNAL;        \
  }

extern "C" int mh_poseidon2_trace_build(mh_ctx* c, const uint64_t* states, const uint64_t* multiplicities, size_t k, int log_n, mh_trace** out,
                                        mh_p2_trace_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    if (out) *out = nullptr;
    MH_REQUIRE(out && ((states && multiplicities) || !k), "mh_poseidon2_trace_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_poseidon2_trace_build: log_n lies in 6..32, or is -1");
    MH_REQUIRE(k < ((u64)1 << 32), "mh_poseidon2_trace_build: too many requests");
    HIP_CHECK(hipSetDevice(c->device));
    P2tCycles a{};
    a.k = k;
    DevBuf list(k * 13 * 8);
    if (k) {
      c->h2d(list.p, states, k * 12 * 8);
      c->h2d(list.u() + k * 12, multiplicities, k * 8);
      a.states = list.u();
      a.mults = list.u() + k * 12;
    }
    *out = p2t_build(c, a, 0, log_n, info, "mh_poseidon2_trace_build");
    return MH_OK;
  }
  P2T_CATCH
}

extern "C" int mh_miden_poseidon2_trace(mh_ctx* c, const mh_trace* chiplets, int log_n, mh_trace** out, mh_p2_trace_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    if (out) *out = nullptr;
    MH_REQUIRE(chiplets && out, "mh_miden_poseidon2_trace: null argument");
    MH_REQUIRE(chiplets->ctx == c, "mh_miden_poseidon2_trace: the chiplets trace belongs to another context");
    MH_REQUIRE(chiplets->width == P2T_CHIPLETS_WIDTH, "mh_miden_poseidon2_trace: the chiplets trace is 22 columns wide");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_miden_poseidon2_trace: log_n lies in 6..32, or is -1");
    MH_REQUIRE(chiplets->log_n >= 1 && chiplets->log_n <= 31, "mh_miden_poseidon2_trace: bad chiplets height");
    HIP_CHECK(hipSetDevice(c->device));
    const u64 n = (u64)1 << chiplets->log_n, table = n / 2 + 1;
    DevBuf tables(2 * table * 4), words(sizeof(P2tWords));
    P2tScan s{chiplets->cols.u(), n, table, (u32*)tables.p, (u32*)tables.p + table, (P2tWords*)words.p};
    const P2tWords init{0, 0, ~0ull, ~0ull, ~0ull};
    c->h2d(words.p, &init, sizeof init);
    trace_wait_ready(c, chiplets);
    {
      ProfScope ps(c, "p2t_scan", 24.0 * (double)n);
      HIP_CHECK(hipMemsetAsync(s.mult, 0, table * 4, c->stream));
      HIP_CHECK(hipMemsetAsync(s.first_row, 0xFF, table * 4, c->stream));
      MH_LAUNCH(k_p2t_scan, dim3(p2t_grid(n, P2T_BT)), dim3(P2T_BT), 0, c->stream, s);
    }
    {
      ProfScope ps(c, "p2t_check", 24.0 * (double)n);
      MH_LAUNCH(k_p2t_check, dim3(p2t_grid(n, P2T_BT)), dim3(P2T_BT), 0, c->stream, s);
    }
    P2tWords w;
    c->d2h(&w, words.p, sizeof w);  // the call's one wait
    const char* entry = "mh_miden_poseidon2_trace";
    const int shown = log_n < 0 ? p2t_min_log_n(w.k) : log_n;
    if (w.bad_row != ~0ull) p2t_refuse(info, w.k, w.n_input, shown, 1, w.bad_row, entry);
    if (w.conflict != ~0ull) p2t_refuse(info, w.k, w.n_input, shown, 3, w.conflict, entry);
    if (w.gap != ~0ull) p2t_refuse(info, w.k, w.n_input, shown, 2, w.gap, entry);
    P2tCycles a{};
    a.chip = s.chip; a.chip_n = n; a.first_row = s.first_row; a.mult32 = s.mult;
    a.k = w.k;
    *out = p2t_build(c, a, w.n_input, log_n, info, entry);
    return MH_OK;
  }
  P2T_CATCH
}
