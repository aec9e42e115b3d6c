// The range-check table laid on the device from the statement's lookups (mh_fill_range_table*), gfx950.
//
// Replaces the ledger next to the reference's range checker (processor/src/trace/range/mod.rs:62-204: add_range_checks collects every
// 16-bit value a stack u32 operation or a memory row looks up, emit_table_rows sorts them and bridges the gaps with rows 3^k apart,
// k <= 7).  Every request is a push of a lookup program, and the table is a function of the SET of values pushed, so the pass reads
// the planes of logup.hip the way balance.hip and multiplicity.hip do (balance.cuh):
//   probe    a scratch copy of the declaring instance's trace with the value column 0 (planes P0), then 1 (P1).  The provider
//            fraction's denominator has to be d0 + g * cell with d0, g the same on every row and g != 0, its multiplicity the same in
//            P0 and P1, and no other fraction may differ between them: k_rng_probe holds the declaration to that numerically and one
//            lane leaves d0 and 1 / g behind.
//   mark     one lane per push of the statement (boundary pushes included) with a non-zero multiplicity, the provider fraction left
//            out: t = (d - d0) / g; c1 = 0 and c0 < 2^16 make it a range lookup of c0 -> atomicOr into a 65 536-bit map.  Bits 0 and
//            65 535 are always set (RangeChecker::new).
//   rows     one workgroup, a lane per 64-bit word of the map: the last present value before the word (max-scan through LDS), per
//            present value 1 + get_num_bridge_rows(gap), an exclusive block sum -> the first row of every word; rows_needed = total + 1
//            (the trailing (0, 65535) row).  The host reads rows_needed, n_values and the probe's word: the one read-back before
//            anything is written.
//   emit     rows [0, n - rows_needed) of both columns := 0 (k_rng_pad); the table in the last rows_needed rows of the value column,
//            bridge rows by write_rows' strides, its multiplicity cells := 0 (k_rng_emit).  One writer per cell, plain stores.
//   fill     fill_run of multiplicity.hip with the one slot: counts and the exact balance report.  Under its owner rule (lowest push
//            id) the count of value 0 lands on row 0 when front padding exists; the reference keeps it on the table's first row, both
//            rows carry the key of value 0, and k_rng_first_row exchanges the two cells.
// Every phase is a launch of its own; words several lanes write within a launch are touched through atomicOr / atomicMin only.
#include "balance.cuh"
#include <string>

static constexpr u32 RNG_VALUES = 1u << 16;          // the reference's rule: 16-bit values
static constexpr u32 RNG_WORDS = RNG_VALUES / 64;    // lanes of the rows / emit kernels
static constexpr u32 RNG_MAX_STRIDE = 2187;          // 3^7

struct RngCoef {  // the provider denominator is d0 + g * cell
  e2 d0, ginv;
};
struct RngScratch {
  u32* map;                   // [RNG_VALUES / 32] presence bits
  u32* first;                 // [RNG_WORDS] first table row of the word's values
  u32* prev;                  // [RNG_WORDS] last present value before the word
  unsigned long long* words;  // bad (atomicMin), rows_needed, n_values
  RngCoef* coef;
};

// get_num_bridge_rows (range/mod.rs:167-180)
__device__ __forceinline__ u32 rng_bridge_rows(u32 gap) {
  u32 rows = 0, stride = RNG_MAX_STRIDE;
  while (gap != stride) {  // ends: gap == 0 meets stride == 0 after 3^0 / 3
    if (gap > stride) {
      rows++;
      gap -= stride;
    } else {
      stride /= 3;
    }
  }
  return rows;
}
__device__ __forceinline__ e2 rng_value1(const BalArgs& a, const BalInst& in, const u64* planes1, u32 out, u64 r) {
  const u64* p = planes1 + (size_t)(2 * out) * in.n + r;
  return e2{gl_canon(p[0]), a.ext[in.ext_off + out] ? gl_canon(p[in.n]) : 0};
}

__global__ __launch_bounds__(BT) void k_rng_set(u64* __restrict__ col, u64 n, u64 value) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t < n) col[t] = value;
}

enum { RNG_BAD_MULT = 1, RNG_BAD_DENOM = 2, RNG_BAD_READER = 3 };
// P0 against P1 over the pushes of the declaring instance `si`.  bad: min over the offending lanes of (fraction << 2 | reason)
__global__ __launch_bounds__(BT) void k_rng_probe(BalArgs a, u32 si, u32 kslot, const u64* __restrict__ planes1, RngScratch sc) {
  const BalInst& in = a.inst[si];
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= in.n * in.K) return;
  const u32 k = (u32)(t >> in.log_n);
  const u64 r = t & (in.n - 1);
  const e2 m0 = bal_value(a, in, 2 * k, r), d0 = bal_value(a, in, 2 * k + 1, r);
  const e2 m1 = rng_value1(a, in, planes1, 2 * k, r), d1 = rng_value1(a, in, planes1, 2 * k + 1, r);
  u32 code = 0;
  if (k == kslot) {
    const e2 ref0 = bal_value(a, in, 2 * k + 1, 0);
    const e2 g = e2_sub(rng_value1(a, in, planes1, 2 * k + 1, 0), ref0);
    if (!e2_eq(m0, m1)) code = RNG_BAD_MULT;
    else if (e2_is_zero(g) || !e2_eq(d0, ref0) || !e2_eq(e2_sub(d1, d0), g)) code = RNG_BAD_DENOM;
    if (r == 0) *sc.coef = RngCoef{ref0, e2_inv(g)};  // the one inverse of the call (of 0: 0, and the call is refused)
  } else if (!e2_eq(m0, m1) || !e2_eq(d0, d1)) {
    code = RNG_BAD_READER;
  }
  if (code) atomicMin(&sc.words[0], ((unsigned long long)k << 2) | code);
}

// one lane per push of the statement; P0 serves every fraction but the provider's, which is left out
__global__ __launch_bounds__(BT) void k_rng_mark(BalArgs a, u32 si, u32 kslot, RngScratch sc) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t == 0) {
    atomicOr(&sc.map[0], 1u);
    atomicOr(&sc.map[RNG_VALUES / 32 - 1], 1u << 31);
  }
  if (t >= a.total) return;
  const u32 i = bal_instance(a, t);
  const BalLane ln = bal_lane(a, t);
  if (i == si && ln.k == kslot) return;
  if (e2_is_zero(bal_value(a, *ln.in, 2 * ln.k, ln.row))) return;
  const e2 d = bal_value(a, *ln.in, 2 * ln.k + 1, ln.row);
  const e2 v = e2_mul(e2_sub(d, sc.coef->d0), sc.coef->ginv);
  if (gl_canon(v.c1) == 0 && gl_canon(v.c0) < RNG_VALUES) {
    const u32 x = (u32)gl_canon(v.c0), bit = 1u << (x & 31);
    // a few values (0 above all) take most of the lookups: a set bit needs no second atomic on its word
    if (!(__hip_atomic_load(&sc.map[x >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&sc.map[x >> 5], bit);
  }
}

// one workgroup of RNG_WORDS lanes, lane l owns values [64 l, 64 l + 64)
__global__ __launch_bounds__(RNG_WORDS) void k_rng_rows(RngScratch sc) {
  __shared__ int s_hi[RNG_WORDS];
  __shared__ unsigned long long s_sum[RNG_WORDS];
  const u32 l = threadIdx.x;
  const u64 w = (u64)sc.map[2 * l] | ((u64)sc.map[2 * l + 1] << 32);
  // inclusive max-scan of the highest present value per word (-1: none)
  s_hi[l] = w ? (int)(64 * l + 63 - __clzll((long long)w)) : -1;
  __syncthreads();
  for (u32 off = 1; off < RNG_WORDS; off <<= 1) {
    const int other = l >= off ? s_hi[l - off] : -1;
    __syncthreads();
    if (other > s_hi[l]) s_hi[l] = other;
    __syncthreads();
  }
  const u32 pv = l ? (u32)s_hi[l - 1] : 0;  // bit 0 is set: s_hi[l - 1] >= 0
  u32 rows = 0, p = pv;
  for (u64 x = w; x; x &= x - 1) {
    const u32 v = 64 * l + (u32)__ffsll((long long)x) - 1;
    rows += 1 + rng_bridge_rows(v - p);
    p = v;
  }
  // inclusive sum-scan of (rows, values) packed: rows <= 2^16 * 44 < 2^32
  s_sum[l] = (unsigned long long)rows | ((unsigned long long)__popcll(w) << 32);
  __syncthreads();
  for (u32 off = 1; off < RNG_WORDS; off <<= 1) {
    const unsigned long long other = l >= off ? s_sum[l - off] : 0;
    __syncthreads();
    s_sum[l] += other;
    __syncthreads();
  }
  sc.first[l] = (u32)s_sum[l] - rows;
  sc.prev[l] = pv;
  if (l == RNG_WORDS - 1) {
    sc.words[1] = (s_sum[l] & 0xFFFFFFFFu) + 1;
    sc.words[2] = s_sum[l] >> 32;
  }
}

// front padding (range/mod.rs:80-91): rows [0, pad) of both columns
__global__ __launch_bounds__(BT) void k_rng_pad(u64* __restrict__ vcol, u64* __restrict__ mcol, u64 pad) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= pad) return;
  vcol[t] = 0;
  mcol[t] = 0;
}

// write_rows (range/mod.rs:184-204) per word; the lane of the last word adds the trailing row.  Rows [pad, n): one writer each
__global__ __launch_bounds__(BT) void k_rng_emit(RngScratch sc, u64* __restrict__ vcol, u64* __restrict__ mcol, u64 pad, u64 n) {
  const u32 l = blockIdx.x * BT + threadIdx.x;
  if (l >= RNG_WORDS) return;
  const u64 w = (u64)sc.map[2 * l] | ((u64)sc.map[2 * l + 1] << 32);
  u64 row = pad + sc.first[l];
  u32 p = sc.prev[l];
  auto put = [&](u32 v) {
    if (row < n) {
      vcol[row] = v;
      mcol[row] = 0;
    }
    row++;
  };
  for (u64 x = w; x; x &= x - 1) {
    const u32 v = 64 * l + (u32)__ffsll((long long)x) - 1;
    u32 gap = v - p, stride = RNG_MAX_STRIDE;
    while (gap != stride) {
      if (gap > stride) {
        gap -= stride;
        p += stride;
        put(p);
      } else {
        stride /= 3;
      }
    }
    put(v);
    p = v;
  }
  if (l == RNG_WORDS - 1) put(RNG_VALUES - 1);
}

// rows 0 and pad both carry value 0: the count goes where the reference writes it
__global__ void k_rng_first_row(u64* __restrict__ mcol, u64 pad) {
  if (blockIdx.x || threadIdx.x) return;
  const u64 a = mcol[0], b = mcol[pad];
  mcol[0] = b;
  mcol[pad] = a;
}

namespace {
std::string rng_name(const FillInput& f, const char* const* names, u32 column, u32 fraction) {
  char buf[128];
  if (names) snprintf(buf, sizeof buf, "%s (instance %d) column %u fraction %u", names[f.label], f.label, column, fraction);
  else snprintf(buf, sizeof buf, "instance %d column %u fraction %u", f.label, column, fraction);
  return buf;
}

// slot.instance indexes `in`
void range_run(mh_ctx* c, const std::vector<FillInput>& in, const std::vector<e2>& rnd, const std::vector<BoundaryPush>& boundary,
               const mh_range_slot& slot, const char* const* names, mh_range_table_info* info, u64* n_written, BalanceReport& rep) {
  const size_t n_in = in.size(), si = (size_t)slot.instance;
  mh_trace* tr = in[si].main;
  const u64 n = (u64)1 << tr->log_n;
  if (info) *info = mh_range_table_info{0, 0, n};
  u32 kslot = slot.fraction;
  for (u32 col = 0; col < slot.lookup_column; col++) kslot += in[si].b.lk->col_count[col];
  u64* vcol = tr->cols.u() + (size_t)slot.value_column * n;
  u64* mcol = tr->cols.u() + (size_t)slot.mult_column * n;

  // ---- planes: P0 of every instance, P1 of the declaring one ----
  std::vector<DevBuf> p0(n_in);
  DevBuf p1, bplanes;
  std::vector<BalInst> inst;
  std::vector<unsigned char> ext;
  u64 total = 0;
  {
    ProfScope ps(c, "range_planes");
    for (size_t i = 0; i < n_in; i++) {
      const mh_lookup* lk = in[i].b.lk;
      const mh_trace* t = in[i].main;
      const u64 ni = (u64)1 << t->log_n;
      if (i != si) {
        lookup_planes(c, lk, t, in[i].b.prep, rnd, p0[i]);
      } else {
        mh_trace scratch;
        scratch.ctx = c; scratch.log_n = t->log_n; scratch.width = t->width;
        scratch.cols.alloc(t->width * ni * 8);
        trace_wait_ready(c, t);
        HIP_CHECK(hipMemcpyAsync(scratch.cols.p, t->cols.p, t->width * ni * 8, hipMemcpyDeviceToDevice, c->stream));
        u64* sv = scratch.cols.u() + (size_t)slot.value_column * ni;
        MH_LAUNCH(k_rng_set, dim3(grid_for(ni)), dim3(BT), 0, c->stream, sv, ni, (u64)0);
        lookup_planes(c, lk, &scratch, in[i].b.prep, rnd, p0[i]);
        MH_LAUNCH(k_rng_set, dim3(grid_for(ni)), dim3(BT), 0, c->stream, sv, ni, (u64)1);
        lookup_planes(c, lk, &scratch, in[i].b.prep, rnd, p1);
      }
      inst.push_back(BalInst{p0[i].u(), ni, total, (u32)lk->n_fractions(), (u32)ext.size(), t->log_n});
      ext.insert(ext.end(), lk->out_ext.begin(), lk->out_ext.begin() + 2 * lk->n_fractions());
      total += ni * lk->n_fractions();
    }
  }
  const size_t nb = boundary.size();
  if (nb) {
    balance_boundary_planes(c, boundary, bplanes);
    inst.push_back(BalInst{bplanes.u(), (u64)nb, total, 1, (u32)ext.size(), 63});
    ext.push_back(0);
    ext.push_back(1);
    total += nb;
  }
  MH_REQUIRE(total < ((u64)1 << 40), "too many pushes for one range-table fill");
  DevBuf dinst(inst.size() * sizeof(BalInst)), dext(ext.size());
  // map | first | prev | words[3] | coef
  const size_t map_bytes = RNG_VALUES / 8, lane_bytes = RNG_WORDS * 4;
  DevBuf scratch_words(map_bytes + 2 * lane_bytes + 3 * 8 + sizeof(RngCoef));
  c->h2d(dinst.p, inst.data(), inst.size() * sizeof(BalInst));
  c->h2d(dext.p, ext.data(), ext.size());
  RngScratch sc{};
  char* base = (char*)scratch_words.p;
  sc.map = (u32*)base;
  sc.first = (u32*)(base + map_bytes);
  sc.prev = (u32*)(base + map_bytes + lane_bytes);
  sc.words = (unsigned long long*)(base + map_bytes + 2 * lane_bytes);
  sc.coef = (RngCoef*)(base + map_bytes + 2 * lane_bytes + 3 * 8);
  HIP_CHECK(hipMemsetAsync(scratch_words.p, 0, scratch_words.bytes, c->stream));
  HIP_CHECK(hipMemsetAsync(sc.words, 0xFF, 8, c->stream));
  BalArgs a{(const BalInst*)dinst.p, (u32)inst.size(), (const unsigned char*)dext.p, total};
  const u64 lanes_si = inst[si].n * inst[si].K;
  {
    ProfScope ps(c, "range_probe", 64.0 * (double)lanes_si);
    MH_LAUNCH(k_rng_probe, dim3(grid_for(lanes_si)), dim3(BT), 0, c->stream, a, (u32)si, kslot, (const u64*)p1.u(), sc);
  }
  {
    ProfScope ps(c, "range_mark", 32.0 * (double)total);
    MH_LAUNCH(k_rng_mark, dim3(grid_for(total)), dim3(BT), 0, c->stream, a, (u32)si, kslot, sc);
  }
  {
    ProfScope ps(c, "range_rows", (double)(map_bytes + 2 * lane_bytes));
    MH_LAUNCH(k_rng_rows, dim3(1), dim3(RNG_WORDS), 0, c->stream, sc);
  }
  u64 got[3];
  c->d2h(got, sc.words, sizeof got);
  c->sync();
  if (got[0] != ~(u64)0) {
    u32 k = (u32)(got[0] >> 2), col = 0;
    while (k >= in[si].b.lk->col_count[col]) k -= in[si].b.lk->col_count[col++];
    const std::string who = rng_name(in[si], names, col, k);
    switch (got[0] & 3) {
      case RNG_BAD_MULT: throw MhError(MH_ERR_INVALID, "range slot " + who + ": its multiplicity reads the value column");
      case RNG_BAD_DENOM:
        throw MhError(MH_ERR_INVALID, "range slot " + who + ": its denominator is not d0 + g * (value cell) with d0 and g != 0 the same on every row");
      default: throw MhError(MH_ERR_INVALID, "undeclared reader: " + who + " reads the range value column and is not the range slot");
    }
  }
  const u64 rows_needed = got[1];
  if (info) *info = mh_range_table_info{got[2], rows_needed, n};
  if (rows_needed > n) {
    char buf[160];
    snprintf(buf, sizeof buf, "the range table needs %llu rows (%llu values) and the trace has %llu", (unsigned long long)rows_needed,
             (unsigned long long)got[2], (unsigned long long)n);
    throw MhError(MH_ERR_INVALID, buf);
  }
  const u64 pad = n - rows_needed;
  {
    ProfScope ps(c, "range_emit", 16.0 * (double)n);
    if (pad) MH_LAUNCH(k_rng_pad, dim3(grid_for(pad)), dim3(BT), 0, c->stream, vcol, mcol, pad);
    MH_LAUNCH(k_rng_emit, dim3(grid_for(RNG_WORDS)), dim3(BT), 0, c->stream, sc, vcol, mcol, pad, n);
  }
  // ---- multiplicities and verify ----
  for (DevBuf& b : p0) b.release();
  p1.release();
  bplanes.release();
  const std::vector<mh_mult_slot> slots{mh_mult_slot{slot.instance, slot.lookup_column, slot.fraction, slot.mult_column}};
  fill_run(c, in, rnd, boundary, slots, names, n_written, rep);
  if (pad) {
    MH_LAUNCH(k_rng_first_row, dim3(1), dim3(64), 0, c->stream, mcol, pad);
    c->sync();
  }
}

// the caller's slot -> instance = index into `in`
mh_range_slot range_slot(const std::vector<FillInput>& in, const std::vector<int>& index_of, const mh_range_slot* slot) {
  MH_REQUIRE(slot, "null range slot");
  mh_range_slot s = *slot;
  char buf[192];
  snprintf(buf, sizeof buf, "range slot (instance %d column %u fraction %u, value column %u, multiplicity column %u) is out of range", s.instance,
           s.lookup_column, s.fraction, s.value_column, s.mult_column);
  MH_REQUIRE(s.instance >= 0 && (size_t)s.instance < index_of.size() && index_of[s.instance] >= 0, buf);
  s.instance = index_of[s.instance];
  const FillInput& f = in[s.instance];
  MH_REQUIRE(s.lookup_column < f.b.lk->num_cols && s.fraction < f.b.lk->col_count[s.lookup_column] && s.value_column < f.main->width &&
                 s.mult_column < f.main->width,
             buf);
  MH_REQUIRE(s.value_column != s.mult_column, "range slot: the value column and the multiplicity column are the same");
  return s;
}
}  // namespace

int range_statement(mh_ctx* c, int n_airs, mh_air* const* airs, mh_trace* const* traces, const mh_trace* const* preps,
                    const u64 challenger_state[12], const u64* pre_observe, size_t n_pre,
                    const std::function<bool(const std::vector<e2>&, std::vector<BoundaryPush>&)>& boundary, const char* const* names,
                    const mh_range_slot* slot, mh_range_table_info* info, uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap,
                    size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n_written && n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    *n_entries = *n_pushes = 0;
    *n_written = 0;
    if (info) *info = mh_range_table_info{0, 0, 0};
    MH_REQUIRE_NO_SALT(c, "mh_fill_range_table*");
    HIP_CHECK(hipSetDevice(c->device));
    size_t max_rand = 0;
    std::vector<FillInput> in;
    std::vector<BalanceInput> bin;
    std::vector<int> index_of(n_airs, -1), instance_of;
    for (int i = 0; i < n_airs; i++) {
      MH_REQUIRE(airs[i] && traces[i], "null AIR or trace");
      MH_REQUIRE(airs[i]->ctx == c && traces[i]->ctx == c, "AIR / trace of another context");
      MH_REQUIRE(!airs[i]->aux_width || airs[i]->lookup, "an AIR with aux columns needs its lookup program attached");
      max_rand = std::max(max_rand, airs[i]->num_randomness);
      if (!airs[i]->lookup) continue;
      index_of[i] = (int)in.size();
      in.push_back(FillInput{BalanceInput{airs[i]->lookup, traces[i], preps && preps[i] ? preps[i] : airs[i]->prep_raw}, traces[i], i});
      bin.push_back(in.back().b);
      instance_of.push_back(i);
    }
    balance_validate(c, bin);
    const mh_range_slot s = range_slot(in, index_of, slot);
    const std::vector<e2> rnd = debug_challenges(challenger_state, pre_observe, n_pre, n_airs, traces, max_rand);
    std::vector<BoundaryPush> bnd;
    MH_REQUIRE(boundary(rnd, bnd), "the statement's boundary pushes could not be evaluated (a zero denominator)");
    BalanceReport rep;
    range_run(c, in, rnd, bnd, s, names, info, n_written, rep);
    for (mh_balance_push& p : rep.pushes)
      if (p.instance >= 0) p.instance = instance_of[p.instance];
    return balance_report(c, rep, names, entries, entry_cap, n_entries, pushes, push_cap, n_pushes);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}

extern "C" int mh_fill_range_table(mh_ctx* c, int n, const mh_lookup* const* lookups, mh_trace* const* traces,
                                   const mh_trace* const* preprocessed, const uint64_t* randomness, size_t n_randomness,
                                   const uint64_t* boundary_denoms, const int32_t* boundary_signs, size_t n_boundary, const mh_range_slot* slot,
                                   mh_range_table_info* info, uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap,
                                   size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n >= 1 && n <= 256 && lookups && traces, "between 1 and 256 instances, with their arrays");
    MH_REQUIRE(n_written && n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    MH_REQUIRE((randomness || !n_randomness) && ((boundary_denoms && boundary_signs) || !n_boundary), "null value array");
    *n_entries = *n_pushes = 0;
    *n_written = 0;
    if (info) *info = mh_range_table_info{0, 0, 0};
    MH_REQUIRE_NO_SALT(c, "mh_fill_range_table*");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<FillInput> in;
    std::vector<BalanceInput> bin;
    std::vector<int> index_of;
    for (int i = 0; i < n; i++) {
      in.push_back(FillInput{BalanceInput{lookups[i], traces[i], preprocessed ? preprocessed[i] : nullptr}, traces[i], i});
      bin.push_back(in.back().b);
      index_of.push_back(i);
    }
    balance_validate(c, bin);
    const mh_range_slot s = range_slot(in, index_of, slot);
    std::vector<e2> rnd;
    for (size_t i = 0; i < n_randomness; i++) rnd.push_back(e2{gl_canon(randomness[2 * i]), gl_canon(randomness[2 * i + 1])});
    for (const BalanceInput& b : bin) MH_REQUIRE(rnd.size() >= b.lk->num_randomness, "not enough lookup challenges");
    std::vector<BoundaryPush> bnd;
    for (size_t i = 0; i < n_boundary; i++) {
      MH_REQUIRE(boundary_signs[i] == 1 || boundary_signs[i] == -1, "a boundary sign is +1 or -1");
      bnd.push_back(BoundaryPush{e2{gl_canon(boundary_denoms[2 * i]), gl_canon(boundary_denoms[2 * i + 1])}, boundary_signs[i]});
      MH_REQUIRE(!e2_is_zero(bnd.back().denom), "a boundary denominator is zero");
    }
    BalanceReport rep;
    range_run(c, in, rnd, bnd, s, nullptr, info, n_written, rep);
    return balance_report(c, rep, nullptr, entries, entry_cap, n_entries, pushes, push_cap, n_pushes);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}
