// Constraint checker (mh_check_*), gfx950.
//
// Replaces crates/lifted-stark/src/debug.rs:70-133 (check_constraints: every constraint of every AIR on every row, aux traces from debug
// challenges, the external assertions), wrapped by processor/src/trace/mod.rs:261-278 (ExecutionTrace::check_constraints) and
// precompiles-prover/src/session/prove.rs:269-275 (SessionTraces::check).  Two stages whose results agree:
//   screen  the AIR's own constraint program (compiled chunks or interpreter, whichever mh_air_load chose) on the trace domain
//           (quotient.hip constraint_fold_trace_domain): F(r) = sum_k alpha^(K-1-k) s_k(r) C_k(r) with a fresh random alpha per call,
//           s_k(r) != 0 wherever the reference's selector is 1.  A row fails when F(r) != 0; a failing row escapes with probability
//           <= K / p^2.  The failing rows are compacted into an ascending list by prefix sums (deterministic, no atomic appends).
//   exact   an interpreter loop (k_eval_quotient's) with the reference's debug selectors, one lane per listed row (or every row,
//           MH_CHECK_EXACT): each constraint that does not vanish adds to fail_count[k] and lowers first_row[k] -- aggregated per wave
//           first (one ballot, one atomic pair per wave and constraint), so a wholly wrong column costs n / 64 atomics per word.
//           Integer add and min do not depend on arrival order: the report is bit-reproducible.  A last launch evaluates every
//           failing constraint at its first row for the reported value.
// Roofline: the screen is the quotient evaluation at 1/D of its points; the exact stage runs on the failing rows only (screen mode).
#include "../../include/midenhip.h"
#include "air.hpp"
#include "air_jit.hpp"
#include "challenger.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include "poseidon2.cuh"
#include <algorithm>
#include <memory>
#include <random>
#include <string>

struct ExactArgs {
  const AirIns* code;
  u32 n_ins;
  const u64* main;  // the raw matrices, column-major (mh_trace::cols)
  const u64* aux;
  const u64* prep;
  int log_n;
  const u64* rows;  // the rows of the lanes (ascending), or null: lane i is row i
  size_t count;
  const u64* periodic;  // [n_periodic][periodic_rows]: the raw columns tiled to the longest period
  u32 periodic_rows;
  const u64* publics;
  const u64* randomness;  // EF pairs
  const u64* aux_values;  // EF pairs
  unsigned long long* fail_count;  // [K]
  unsigned long long* first_row;   // [K], ~0 = none
  u32* row_bad;                    // [n]: some constraint fails on the row
  const u32* target;               // value mode: the constraint of each lane (rows = its first row); null otherwise
  u64* value;                      // value mode: [2 * count]
};

__global__ __launch_bounds__(256) void k_check_exact(ExactArgs a) {
  extern __shared__ u64 slots[];
  const u32 T = blockDim.x, tid = threadIdx.x;
  const size_t n = (size_t)1 << a.log_n;
  const size_t i = blockIdx.x * (size_t)T + tid;
  const bool live = i < a.count;  // dead lanes run along (rows 0) so that the ballots below see whole waves
  const size_t r = live ? (a.rows ? a.rows[i] : i) : 0;
  const size_t r_next = (r + 1) & (n - 1);
  const u32 target = a.target && live ? a.target[i] : 0xFFFFFFFFu;
  bool bad = false;
#define SLOT0(s) slots[(size_t)(2 * (s)) * T + tid]
#define SLOT1(s) slots[(size_t)(2 * (s) + 1) * T + tid]
  auto fetch = [&](uint8_t kind, u32 idx, bool ext, u64 imm) -> e2 {
    switch (kind) {
      case OPK_SLOT: return e2{SLOT0(idx), ext ? SLOT1(idx) : 0};
      case DOP_CONST: return e2_make(imm);
      case DOP_MAIN: return e2_make(a.main[((size_t)(idx & 0x7FFFFFFFu) << a.log_n) + ((idx >> 31) ? r_next : r)]);
      case DOP_AUX: {
        const size_t rr = (idx >> 31) ? r_next : r, cc = idx & 0x7FFFFFFFu;
        return e2{a.aux[((2 * cc) << a.log_n) + rr], a.aux[((2 * cc + 1) << a.log_n) + rr]};
      }
      case DOP_PREP: return e2_make(a.prep[((size_t)(idx & 0x7FFFFFFFu) << a.log_n) + ((idx >> 31) ? r_next : r)]);
      case DOP_PUBLIC: return e2_make(a.publics[idx]);
      case DOP_PERIODIC: return e2_make(a.periodic[(size_t)idx * a.periodic_rows + (r % a.periodic_rows)]);
      case DOP_IS_FIRST: return e2_make(r == 0 ? 1 : 0);
      case DOP_IS_LAST: return e2_make(r == n - 1 ? 1 : 0);
      case DOP_IS_TRANSITION: return e2_make(r != n - 1 ? 1 : 0);
      case DOP_RANDOMNESS: return e2{a.randomness[2 * idx], a.randomness[2 * idx + 1]};
      default: return e2{a.aux_values[2 * idx], a.aux_values[2 * idx + 1]};  // DOP_AUX_VALUE
    }
  };
#pragma unroll 1
  for (u32 pc = 0; pc < a.n_ins; pc++) {
    const AirIns ins = a.code[pc];
    const bool a_ext = ins.ext & 1, b_ext = ins.ext & 2;
    const e2 va = fetch(ins.a_kind, ins.a, a_ext, ins.imm);
    if (ins.op == DOP_FOLD) {  // constraint ins.b has the value va on this row
      const e2 v = e2{gl_canon(va.c0), a_ext ? gl_canon(va.c1) : 0};
      if (a.target) {
        if (ins.b == target) {
          a.value[2 * i] = v.c0;
          a.value[2 * i + 1] = v.c1;
        }
        continue;
      }
      const bool f = live && !e2_is_zero(v);
      bad |= f;
      const unsigned long long mask = __ballot(f);  // uniform: every lane runs every instruction
      if (mask && __lane_id() == (unsigned)__builtin_ctzll(mask)) {
        // the lowest failing lane holds the wave's smallest failing row (rows ascend with the lane)
        atomicAdd(&a.fail_count[ins.b], (unsigned long long)__popcll(mask));
        atomicMin(&a.first_row[ins.b], (unsigned long long)r);
      }
      continue;
    }
    e2 v;
    if (ins.op == DOP_NEG) {
      v = a_ext ? e2_neg(va) : e2_make(gl_neg(va.c0));
    } else {
      const e2 vb = fetch(ins.b_kind, ins.b, b_ext, ins.imm);
      const bool ext = a_ext || b_ext;
      if (ins.op == DOP_ADD) v = ext ? e2_add(va, vb) : e2_make(gl_add(va.c0, vb.c0));
      else if (ins.op == DOP_SUB) v = ext ? e2_sub(va, vb) : e2_make(gl_sub(va.c0, vb.c0));
      else {  // MUL
        if (a_ext && b_ext) v = e2_mul(va, vb);
        else if (a_ext) v = e2_mulf(va, vb.c0);
        else if (b_ext) v = e2_mulf(vb, va.c0);
        else v = e2_make(gl_mul(va.c0, vb.c0));
      }
    }
    SLOT0(ins.dst) = v.c0;
    if (a_ext || b_ext) SLOT1(ins.dst) = v.c1;
  }
#undef SLOT0
#undef SLOT1
  if (bad) a.row_bad[r] = 1;
}

// trace-domain selector tables of the screen: [r == 0], [r == n-1]
__global__ void k_check_selectors(u64* first, u64* last, size_t n) {
  const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (r >= n) return;
  first[r] = r == 0 ? 1 : 0;
  last[r] = r == n - 1 ? 1 : 0;
}
// the screen's verdict: F(r) != 0 mod p (any representative)
__global__ void k_check_screen_flags(const u64* __restrict__ acc, size_t n, u32* __restrict__ flags) {
  const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (r >= n) return;
  flags[r] = (gl_canon(acc[r]) | gl_canon(acc[n + r])) != 0;
}

// ---- compaction: flagged rows -> ascending row list (tile counts, exclusive scan over the tiles, scatter; logup.hip's tile pattern) ----
static constexpr int CT = 256, CI = 8, CTILE = CT * CI;
__global__ __launch_bounds__(CT) void k_compact_count(const u32* __restrict__ flags, size_t n, u64* __restrict__ tile_cnt) {
  __shared__ u64 part[CT];
  const size_t base = (size_t)blockIdx.x * CTILE + (size_t)threadIdx.x * CI;
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < CI; k++) s += base + k < n && flags[base + k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = CT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = part[0];
}
// one workgroup: tile counts -> exclusive tile offsets; the total goes to `total`
__global__ __launch_bounds__(CT) void k_compact_offsets(u64* __restrict__ tile_cnt, size_t tiles, u64* __restrict__ total) {
  __shared__ u64 part[CT];
  __shared__ u64 carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t base = 0; base < tiles; base += CT) {
    const size_t i = base + threadIdx.x;
    const u64 v = i < tiles ? tile_cnt[i] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < CT; off <<= 1) {
      const u64 x = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
      __syncthreads();
      part[threadIdx.x] += x;
      __syncthreads();
    }
    const u64 incl = carry + part[threadIdx.x];
    if (i < tiles) tile_cnt[i] = incl - v;
    __syncthreads();
    if (threadIdx.x == CT - 1) carry = incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = carry;
}
__global__ __launch_bounds__(CT) void k_compact_write(const u32* __restrict__ flags, size_t n, const u64* __restrict__ tile_off,
                                                      u64* __restrict__ rows) {
  __shared__ u64 part[CT];
  const size_t base = (size_t)blockIdx.x * CTILE + (size_t)threadIdx.x * CI;
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < CI; k++) s += base + k < n && flags[base + k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < CT; off <<= 1) {
    const u64 x = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  u64 run = tile_off[blockIdx.x] + part[threadIdx.x] - s;
#pragma unroll
  for (int k = 0; k < CI; k++)
    if (base + k < n && flags[base + k]) rows[run++] = base + k;
}

// flags [n] -> rows [n] (ascending); returns their number (waits for the stream)
size_t compact_rows(mh_ctx* c, const u32* flags, size_t n, u64* rows) {
  const size_t tiles = (n + CTILE - 1) / CTILE;
  DevBuf cnt(tiles * 8), total(8);
  MH_LAUNCH(k_compact_count, dim3((unsigned)tiles), dim3(CT), 0, c->stream, flags, n, cnt.u());
  MH_LAUNCH(k_compact_offsets, dim3(1), dim3(CT), 0, c->stream, cnt.u(), tiles, total.u());
  MH_LAUNCH(k_compact_write, dim3((unsigned)tiles), dim3(CT), 0, c->stream, flags, n, cnt.u(), rows);
  u64 m = 0;
  HIP_CHECK(hipMemcpyAsync(&m, total.p, 8, hipMemcpyDeviceToHost, c->stream));
  c->sync();
  return (size_t)m;
}

static e2 random_ef() {
  static thread_local std::mt19937_64 rng{std::random_device{}()};
  auto felt = [] {
    u64 x;
    do x = rng(); while (x >= GL_P);
    return x;
  };
  const u64 c0 = felt();
  return e2{c0, felt()};
}

// the argument checks shared by check_air and mh_constraint_fold -> the preprocessed matrix the AIR reads (null: none)
static const mh_trace* check_air_args(const mh_air* air, const mh_trace* main, const mh_trace* aux, const mh_trace* prep, size_t n_public,
                                      size_t n_randomness, size_t n_aux_values) {
  MH_REQUIRE(air && main, "null AIR or trace");
  MH_REQUIRE(main->width == air->main_width, "trace width does not match the AIR");
  MH_REQUIRE(main->log_n >= 1, "trace needs at least 2 rows");
  const int log_n = main->log_n;
  const size_t n = (size_t)1 << log_n;
  MH_REQUIRE(air->max_period() <= n, "trace shorter than a periodic column");
  if (air->aux_width) {
    MH_REQUIRE(aux, "the AIR has aux columns: the aux trace is required");
    MH_REQUIRE(aux->width == 2 * air->aux_width && aux->log_n == log_n, "aux trace shape does not match the AIR / main trace");
  }
  if (!prep) prep = air->prep_raw;
  if (air->preprocessed_width) {
    MH_REQUIRE(prep, "the AIR has preprocessed columns: the preprocessed matrix is required");
    MH_REQUIRE(prep->width == air->preprocessed_width && prep->log_n == log_n, "preprocessed matrix shape does not match the AIR / trace");
  } else {
    prep = nullptr;
  }
  MH_REQUIRE(n_public == air->num_public, "AIR expects a different number of public values");
  MH_REQUIRE(n_randomness >= air->num_randomness, "not enough randomness for the AIR");
  MH_REQUIRE(n_aux_values >= air->num_aux_values, "not enough aux values for the AIR");
  return prep;
}

void check_air(mh_ctx* c, const mh_air* air, const mh_trace* main, const mh_trace* aux, const mh_trace* prep, const std::vector<u64>& publics,
               const std::vector<e2>& randomness, const std::vector<e2>& aux_values, bool exact, int instance,
               std::vector<mh_check_entry>& out, std::vector<u64>* failing_rows) {
  prep = check_air_args(air, main, aux, prep, publics.size(), randomness.size(), aux_values.size());
  const int log_n = main->log_n;
  const size_t n = (size_t)1 << log_n;
  if (failing_rows) failing_rows->clear();
  const size_t K = air->n_constraints;
  if (!K) return;
  trace_wait_ready(c, main);
  trace_wait_ready(c, aux);
  trace_wait_ready(c, prep);

  // small tables of the exact stage
  const size_t Pm = air->max_period(), prow = Pm ? Pm : 1;
  std::vector<u64> blob;
  for (size_t col = 0; col < air->periodic.size(); col++)
    for (size_t i = 0; i < prow; i++) blob.push_back(air->periodic[col][i % air->periodic[col].size()] % GL_P);
  const size_t o_pub = blob.size();
  for (u64 v : publics) blob.push_back(gl_canon(v));
  const size_t o_rnd = blob.size();
  for (e2 v : randomness) { blob.push_back(gl_canon(v.c0)); blob.push_back(gl_canon(v.c1)); }
  const size_t o_av = blob.size();
  for (e2 v : aux_values) { blob.push_back(gl_canon(v.c0)); blob.push_back(gl_canon(v.c1)); }
  blob.push_back(0);
  DevBuf dblob(blob.size() * 8);
  c->h2d(dblob.p, blob.data(), blob.size() * 8);
  DevBuf count(K * 8), first(K * 8), bad(n * 4), rows;
  HIP_CHECK(hipMemsetAsync(count.p, 0, K * 8, c->stream));
  HIP_CHECK(hipMemsetAsync(first.p, 0xFF, K * 8, c->stream));
  HIP_CHECK(hipMemsetAsync(bad.p, 0, n * 4, c->stream));

  size_t lanes = n;
  if (!exact) {
    DevBuf sel(2 * n * 8), acc(2 * n * 8), flags(n * 4);
    MH_LAUNCH(k_check_selectors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, sel.u(), sel.u() + n, n);
    std::vector<u64> pub(publics.begin(), publics.end());
    constraint_fold_trace_domain(c, air, main, aux, prep, sel.u(), sel.u() + n, pub, randomness, aux_values, random_ef(), acc.u());
    MH_LAUNCH(k_check_screen_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, acc.u(), n, (u32*)flags.p);
    rows.alloc(n * 8);
    lanes = compact_rows(c, (const u32*)flags.p, n, rows.u());
    if (!lanes) return;
  }
  ExactArgs a{};
  a.code = (const AirIns*)air->d_code.p;
  a.n_ins = (u32)air->code.size();
  a.main = main->cols.u();
  a.aux = aux ? aux->cols.u() : main->cols.u();  // an AIR without aux columns never reads them
  a.prep = prep ? prep->cols.u() : main->cols.u();
  a.log_n = log_n;
  a.rows = exact ? nullptr : rows.u();
  a.count = lanes;
  a.periodic = dblob.u();
  a.periodic_rows = (u32)prow;
  a.publics = dblob.u() + o_pub;
  a.randomness = dblob.u() + o_rnd;
  a.aux_values = dblob.u() + o_av;
  a.fail_count = (unsigned long long*)count.p;
  a.first_row = (unsigned long long*)first.p;
  a.row_bad = (u32*)bad.p;
  unsigned T = 256;
  while (T > 64 && (size_t)air->n_slots * 16 * T > 48 * 1024) T >>= 1;
  const size_t lds = (size_t)air->n_slots * 16 * T;
  MH_REQUIRE(lds <= 160 * 1024, "constraint DAG needs more live values than fit in LDS (160 KiB per workgroup)");
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void*)k_check_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  {
    ProfScope ps(c, "check_exact", (double)lanes * (8.0 * air->touched_base_columns));
    MH_LAUNCH(k_check_exact, dim3((unsigned)((lanes + T - 1) / T)), dim3(T), lds, c->stream, a);
  }
  std::vector<u64> cnt(K), fr(K);
  c->d2h(cnt.data(), count.p, K * 8);
  c->d2h(fr.data(), first.p, K * 8);
  c->sync();
  std::vector<u32> failing;
  std::vector<u64> at;
  for (size_t k = 0; k < K; k++)
    if (cnt[k]) {
      failing.push_back((u32)k);
      at.push_back(fr[k]);
    }
  if (!failing.empty()) {  // the value of every failing constraint at its first row
    const size_t m = failing.size();
    DevBuf drows(m * 8), dtarget(m * 4), dval(2 * m * 8);
    c->h2d(drows.p, at.data(), m * 8);
    c->h2d(dtarget.p, failing.data(), m * 4);
    ExactArgs v = a;
    v.rows = drows.u();
    v.count = m;
    v.target = (const u32*)dtarget.p;
    v.value = dval.u();
    MH_LAUNCH(k_check_exact, dim3((unsigned)((m + T - 1) / T)), dim3(T), lds, c->stream, v);
    std::vector<u64> val(2 * m);
    c->d2h(val.data(), dval.p, 2 * m * 8);
    c->sync();
    for (size_t j = 0; j < m; j++) out.push_back(mh_check_entry{instance, failing[j], cnt[failing[j]], at[j], {val[2 * j], val[2 * j + 1]}});
  }
  if (failing_rows && !failing.empty()) {
    if (!rows.p) rows.alloc(n * 8);
    const size_t m = compact_rows(c, (const u32*)bad.p, n, rows.u());
    failing_rows->resize(m);
    if (m) {
      c->d2h(failing_rows->data(), rows.p, m * 8);
      c->sync();
    }
  }
}

// order (instance, first_row, constraint), external entries last; copy out, count, name the first
static int report(mh_ctx* c, std::vector<mh_check_entry>& e, const char* const* names, mh_check_entry* out, size_t cap, size_t* n_entries) {
  std::stable_sort(e.begin(), e.end(), [](const mh_check_entry& x, const mh_check_entry& y) {
    const uint32_t ix = (uint32_t)x.instance, iy = (uint32_t)y.instance;  // -1 sorts last
    if (ix != iy) return ix < iy;
    if (x.first_row != y.first_row) return x.first_row < y.first_row;
    return x.constraint < y.constraint;
  });
  *n_entries = e.size();
  for (size_t i = 0; i < e.size() && i < cap; i++) out[i] = e[i];
  if (e.empty()) return MH_OK;
  const mh_check_entry& f = e[0];
  char buf[256];
  if (f.instance < 0)
    snprintf(buf, sizeof buf, "external assertion %u does not vanish: (%llu, %llu)", f.constraint, (unsigned long long)f.value[0],
             (unsigned long long)f.value[1]);
  else if (names)
    snprintf(buf, sizeof buf, "%s row %llu constraint %u: (%llu, %llu), fails on %llu rows", names[f.instance], (unsigned long long)f.first_row,
             f.constraint, (unsigned long long)f.value[0], (unsigned long long)f.value[1], (unsigned long long)f.rows);
  else
    snprintf(buf, sizeof buf, "instance %d row %llu constraint %u: (%llu, %llu), fails on %llu rows", f.instance, (unsigned long long)f.first_row,
             f.constraint, (unsigned long long)f.value[0], (unsigned long long)f.value[1], (unsigned long long)f.rows);
  c->err = buf;
  return MH_ERR_UNSATISFIED;
}

// debug challenges of a statement: the transcript of a proof up to the main commitment, which is left out
std::vector<e2> debug_challenges(const u64 challenger_state[12], const u64* pre_observe, size_t n_pre, int n_airs, mh_trace* const* traces,
                                 size_t count) {
  HostChallenger ch;
  ch.hash = MH_LMCS_POSEIDON2;
  ch.init_from_state(challenger_state);
  for (size_t i = 0; i < n_pre; i++) ch.observe_framing(pre_observe[i]);
  ch.observe((u64)n_airs);
  for (int i = 0; i < n_airs; i++) ch.observe((u64)traces[i]->log_n);
  std::vector<e2> rnd;
  for (size_t i = 0; i < count; i++) rnd.push_back(ch.sample_ef());
  return rnd;
}

int check_statement(mh_ctx* c, int n_airs, mh_air* const* airs, mh_trace* const* traces, const mh_trace* const* preps, const u64* publics,
                    size_t n_publics, const u64 challenger_state[12], const u64* pre_observe, size_t n_pre, mh_external_assertions ext,
                    void* ext_user, const char* const* names, int flags, mh_check_entry* out, size_t cap, size_t* n_entries) {
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n_entries && (out || !cap), "null n_entries / out");
    MH_REQUIRE((flags & ~MH_CHECK_EXACT) == 0, "unknown check flags");
    *n_entries = 0;
    MH_REQUIRE_NO_SALT(c, "mh_check_*");
    HIP_CHECK(hipSetDevice(c->device));
    size_t max_rand = 0;
    for (int i = 0; i < n_airs; i++) {
      MH_REQUIRE(airs[i] && traces[i], "null AIR or trace");
      MH_REQUIRE(airs[i]->ctx == c && traces[i]->ctx == c, "AIR / trace of another context");
      MH_REQUIRE(traces[i]->width == airs[i]->main_width, "trace width does not match the AIR");
      MH_REQUIRE(!airs[i]->aux_width || airs[i]->lookup, "an AIR with aux columns needs its lookup program attached");
      max_rand = std::max(max_rand, airs[i]->num_randomness);
    }
    const std::vector<e2> rnd = debug_challenges(challenger_state, pre_observe, n_pre, n_airs, traces, max_rand);
    // aux traces on the device, the statement's aux values
    std::vector<std::unique_ptr<mh_trace>> aux(n_airs);
    std::vector<std::vector<e2>> aux_vals(n_airs);
    for (int i = 0; i < n_airs; i++) {
      const mh_air* a = airs[i];
      aux_vals[i].assign(a->num_aux_values, e2_make(0));
      if (!a->lookup) continue;
      const mh_trace* prep = preps && preps[i] ? preps[i] : a->prep_raw;
      e2 fin;
      aux[i].reset(lookup_build_aux(c, a->lookup, traces[i], prep, rnd, &fin));
      if (!aux_vals[i].empty()) aux_vals[i][0] = fin;
    }
    std::vector<mh_check_entry> entries;
    for (int i = 0; i < n_airs; i++) {
      const mh_air* a = airs[i];
      std::vector<u64> pub(publics, publics + n_publics);
      std::vector<e2> r(rnd.begin(), rnd.begin() + a->num_randomness);
      check_air(c, a, traces[i], aux[i].get(), preps ? preps[i] : nullptr, pub, r, aux_vals[i], (flags & MH_CHECK_EXACT) != 0, i, entries,
                nullptr);
    }
    if (ext) {
      std::vector<std::vector<u64>> flat(n_airs);
      std::vector<const u64*> vp(n_airs);
      std::vector<size_t> nv(n_airs);
      std::vector<uint8_t> lhs(n_airs);
      for (int i = 0; i < n_airs; i++) {
        for (e2 v : aux_vals[i]) { flat[i].push_back(v.c0); flat[i].push_back(v.c1); }
        flat[i].push_back(0);
        vp[i] = flat[i].data();
        nv[i] = aux_vals[i].size();
        lhs[i] = (uint8_t)traces[i]->log_n;
      }
      std::vector<u64> rflat;
      for (e2 v : rnd) { rflat.push_back(v.c0); rflat.push_back(v.c1); }
      rflat.push_back(0);
      std::vector<u64> asr(2 * 64);
      const int na = ext(ext_user, rflat.data(), rnd.size(), vp.data(), nv.data(), lhs.data(), n_airs, asr.data(), 64);
      MH_REQUIRE(na >= 0, "the statement's external assertions could not be evaluated (a zero denominator)");
      for (int k = 0; k < na && k < 64; k++)
        if (gl_canon(asr[2 * k]) | gl_canon(asr[2 * k + 1]))
          entries.push_back(mh_check_entry{-1, (uint32_t)k, 1, 0, {gl_canon(asr[2 * k]), gl_canon(asr[2 * k + 1])}});
    }
    return report(c, entries, names, out, cap, n_entries);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}

extern "C" int mh_check_constraints(mh_ctx* c, const mh_air* air, const mh_trace* main_trace, const mh_trace* aux, const mh_trace* preprocessed,
                                    const uint64_t* public_values, size_t n_public, const uint64_t* randomness, size_t n_randomness,
                                    const uint64_t* aux_values, size_t n_aux_values, int flags, mh_check_entry* out, size_t cap,
                                    size_t* n_entries, uint64_t* failing_rows) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(air && main_trace && n_entries && (out || !cap), "null argument");
    MH_REQUIRE(air->ctx == c && main_trace->ctx == c && (!aux || aux->ctx == c), "AIR / trace of another context");
    MH_REQUIRE_NO_SALT(c, "mh_check_constraints");
    MH_REQUIRE((public_values || !n_public) && (randomness || !n_randomness) && (aux_values || !n_aux_values), "null value array");
    MH_REQUIRE((flags & ~MH_CHECK_EXACT) == 0, "unknown check flags");
    *n_entries = 0;
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<u64> pub(public_values, public_values + n_public);
    std::vector<e2> rnd, av;
    for (size_t i = 0; i < n_randomness; i++) rnd.push_back(e2{gl_canon(randomness[2 * i]), gl_canon(randomness[2 * i + 1])});
    for (size_t i = 0; i < n_aux_values; i++) av.push_back(e2{gl_canon(aux_values[2 * i]), gl_canon(aux_values[2 * i + 1])});
    std::vector<mh_check_entry> entries;
    std::vector<u64> rows;
    check_air(c, air, main_trace, aux, preprocessed, pub, rnd, av, (flags & MH_CHECK_EXACT) != 0, 0, entries, failing_rows ? &rows : nullptr);
    if (failing_rows) {
      failing_rows[0] = rows.size();
      std::copy(rows.begin(), rows.end(), failing_rows + 1);
    }
    return report(c, entries, nullptr, out, cap, n_entries);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}

// accumulator planes [2][n], any representative -> canonical EF pairs [n][2]
__global__ void k_fold_pairs(const u64* __restrict__ acc, size_t n, u64* __restrict__ out) {
  const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (r >= n) return;
  out[2 * r] = gl_canon(acc[r]);
  out[2 * r + 1] = gl_canon(acc[n + r]);
}

// Test and diagnostic entry (as mh_pcs_download_deep is): the screen's fold itself, with the caller's alpha instead of a fresh random one.
// out [n][2] receives F(r) = sum_k alpha^(K-1-k) s_k(r) C_k(r) as canonical EF pairs, computed by the AIR's own constraint program on the
// trace domain (quotient.hip constraint_fold_trace_domain: compiled chunks or interpreter, whichever mh_air_load chose) with the screen's
// selector values: x = w_n^r, Z_H = 1/Z_H = 1, is_first = [r == 0], is_last = [r == n-1], is_transition = w_n^r - w_n^-1 (zero on the
// last row only, NOT [r != n-1]), next row = (r + 1) mod n.  K = 0: all zero.
extern "C" int mh_constraint_fold(mh_ctx* c, const mh_air* air, const mh_trace* main_trace, const mh_trace* aux, const mh_trace* preprocessed,
                                  const uint64_t* public_values, size_t n_public, const uint64_t* randomness, size_t n_randomness,
                                  const uint64_t* aux_values, size_t n_aux_values, const uint64_t alpha[2], uint64_t* out) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(air && main_trace && alpha && out, "null argument");
    MH_REQUIRE(air->ctx == c && main_trace->ctx == c && (!aux || aux->ctx == c), "AIR / trace of another context");
    MH_REQUIRE_NO_SALT(c, "mh_constraint_fold");
    MH_REQUIRE((public_values || !n_public) && (randomness || !n_randomness) && (aux_values || !n_aux_values), "null value array");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<u64> pub(public_values, public_values + n_public);
    std::vector<e2> rnd, av;
    for (size_t i = 0; i < n_randomness; i++) rnd.push_back(e2{gl_canon(randomness[2 * i]), gl_canon(randomness[2 * i + 1])});
    for (size_t i = 0; i < n_aux_values; i++) av.push_back(e2{gl_canon(aux_values[2 * i]), gl_canon(aux_values[2 * i + 1])});
    const mh_trace* prep = check_air_args(air, main_trace, aux, preprocessed, n_public, n_randomness, n_aux_values);
    const size_t n = (size_t)1 << main_trace->log_n;
    if (!air->n_constraints) {
      std::fill(out, out + 2 * n, (uint64_t)0);
      return MH_OK;
    }
    trace_wait_ready(c, main_trace);
    trace_wait_ready(c, aux);
    trace_wait_ready(c, prep);
    DevBuf sel(2 * n * 8), acc(2 * n * 8), pairs(2 * n * 8);
    MH_LAUNCH(k_check_selectors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, sel.u(), sel.u() + n, n);
    constraint_fold_trace_domain(c, air, main_trace, aux, prep, sel.u(), sel.u() + n, pub, rnd, av,
                                 e2{gl_canon(alpha[0]), gl_canon(alpha[1])}, acc.u());
    MH_LAUNCH(k_fold_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, acc.u(), n, pairs.u());
    c->d2h(out, pairs.p, 2 * n * 8);
    c->sync();
    return MH_OK;
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}
