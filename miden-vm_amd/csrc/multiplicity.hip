// LogUp multiplicity columns filled on the device (mh_fill_multiplicities*), gfx950.
//
// Replaces the host-side ledgers next to the reference's trace generators (precompiles-prover byte_pair_lut.rs:134-226 "the per-pair
// multiplicity ledger the consumers fill", uint/add/trace.rs:37-103 UintAddRequires, RangeChecker::emit_table_rows): the one step of
// trace building that is not row-local.  A multiplicity cell is the value that makes its key's net zero, and the lookup programs
// already say who pushes what, so the pass is generic over the planes of logup.hip and the table of balance.hip (balance.cuh):
//   probe    per instance with declared columns: a scratch copy of its trace, the declared columns set to 0 (planes P0), then to 1
//            (P1).  A slot's multiplicity is a(r) + b(r) * cell with a = m_P0, b = m_P1 - m_P0; k_mul_probe holds the declaration to
//            that numerically (the library keeps no expression nodes), counts the table's entries and flags live zero denominators.
//   insert   every push with a != 0, every boundary push and every slot push with b != 0 (a provider candidate, also with a = 0) into
//            one table; per key the sum of the a's and, in a 64-bit owner word (atomicMin, all ones = none), the lowest candidate id.
//   final    the sums mod p.
//   resolve  one lane per (instance, declared column, row): the first slot of the column in declaration order with b(r) != 0 decides;
//            the cell becomes -net_c0 / b when that push owns its key, 0 when it does not; no such slot: the cell is not touched.
//   verify   the exact stage of balance.hip over the filled traces: its report is the call's.
// Every phase is a launch of its own: within a launch, words other lanes write are touched through atomics only; the net and the owner
// are read plainly in the next launch.  The owner is a minimum over ids and the sums are integer sums, so nothing of the slot order
// reaches a written value.
#include "balance.cuh"
#include <algorithm>
#include <memory>
#include <string>

struct MulInst {
  const u64* planes1;  // P1 [2 * n_out][n]; null: the instance declares no column (and for the boundary instance)
  u32 frac_off;        // offset of its fractions in MulArgs::slot_col
};
struct MulArgs {
  const MulInst* inst;  // per instance of BalArgs
  const u32* slot_col;  // per fraction: 1 + the main column its multiplicity is affine in; 0: not a slot
};
struct MulCol {  // a declared column: lanes [base, base + n) of the resolve pass are its rows
  u64 base;
  u64* cell;          // the column in the trace's storage
  u32 inst;
  u32 s_begin, s_end;  // its slots (global fraction indices of the instance) in MulResolve::slot_k, declaration order
};
struct MulResolve {
  const MulCol* col;
  const u32* slot_k;
  u32 n_col;
  u64 total;
};

__device__ __forceinline__ e2 mul_value1(const BalArgs& a, const BalInst& in, const u64* planes1, u32 out, u64 r) {
  const u64* p = planes1 + (size_t)(2 * out) * in.n + r;
  return e2{gl_canon(p[0]), a.ext[in.ext_off + out] ? gl_canon(p[in.n]) : 0};
}

// scratch trace: the declared columns := value
__global__ __launch_bounds__(BT) void k_mul_fill(u64* __restrict__ cols, u64 n, const u32* __restrict__ list, u32 n_list, u64 value) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= n * n_list) return;
  cols[(size_t)list[t / n] * n + t % n] = value;
}

enum { MUL_BAD_KEY = 1, MUL_BAD_EF = 2, MUL_BAD_READER = 3 };
// P0 against P1.  bad: min over the offending lanes of (instance << 32 | fraction << 2 | reason); zero: a live push has denominator 0;
// count: pushes with a != 0 plus provider candidates (the table's size)
__global__ __launch_bounds__(BT) void k_mul_probe(BalArgs a, MulArgs ma, unsigned long long* bad, u32* zero, unsigned long long* count) {
  __shared__ u32 sc[BT];
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  u32 add = 0;
  if (t < a.total) {
    const u32 i = bal_instance(a, t);
    const BalLane ln = bal_lane(a, t);
    const e2 m0 = bal_value(a, *ln.in, 2 * ln.k, ln.row), d0 = bal_value(a, *ln.in, 2 * ln.k + 1, ln.row);
    add = !e2_is_zero(m0);
    const u64* p1 = ma.inst[i].planes1;
    if (p1) {
      const e2 m1 = mul_value1(a, *ln.in, p1, 2 * ln.k, ln.row), d1 = mul_value1(a, *ln.in, p1, 2 * ln.k + 1, ln.row);
      u32 code = 0;
      if (ma.slot_col[ma.inst[i].frac_off + ln.k]) {
        const e2 b = e2_sub(m1, m0);
        if (!e2_eq(d0, d1)) code = MUL_BAD_KEY;
        else if (b.c1) code = MUL_BAD_EF;
        else add += b.c0 != 0;
      } else if (!e2_eq(m0, m1) || !e2_eq(d0, d1)) {
        code = MUL_BAD_READER;
      }
      if (code) atomicMin(bad, ((unsigned long long)i << 32) | ((unsigned long long)ln.k << 2) | code);
    }
    if (add && e2_is_zero(d0)) atomicOr(zero, 1u);
  }
  sc[threadIdx.x] = add;
  __syncthreads();
  for (int off = BT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) sc[threadIdx.x] += sc[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sc[0]) atomicAdd(count, (unsigned long long)sc[0]);
}

__global__ __launch_bounds__(BT) void k_mul_insert(BalArgs a, MulArgs ma, BalTable tb, unsigned long long* owner) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= a.total) return;
  const u32 i = bal_instance(a, t);
  const BalLane ln = bal_lane(a, t);
  const e2 m0 = bal_value(a, *ln.in, 2 * ln.k, ln.row);
  u64 b = 0;
  const u64* p1 = ma.inst[i].planes1;
  if (p1 && ma.slot_col[ma.inst[i].frac_off + ln.k]) b = gl_sub(mul_value1(a, *ln.in, p1, 2 * ln.k, ln.row).c0, m0.c0);
  if (e2_is_zero(m0) && !b) return;
  const e2 d = bal_value(a, *ln.in, 2 * ln.k + 1, ln.row);
  const u64 slot = bal_probe<true>(a, tb, d, ln.id);
  bal_accumulate(tb, slot, m0);
  if (b) atomicMin(&owner[slot], (unsigned long long)ln.id);
}

__global__ __launch_bounds__(BT) void k_mul_final(BalTable tb) {
  const u64 s = (u64)blockIdx.x * BT + threadIdx.x;
  if (s <= tb.mask && tb.claim[s]) bal_reduce_slot(tb, s);
}

// one lane per (declared column, row); no two lanes write one cell
__global__ __launch_bounds__(BT) void k_mul_resolve(BalArgs a, MulArgs ma, MulResolve rs, BalTable tb, const unsigned long long* __restrict__ owner,
                                                    unsigned long long* written) {
  __shared__ u32 sc[BT];
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  u32 wrote = 0;
  if (t < rs.total) {
    u32 ci = 0;
    while (ci + 1 < rs.n_col && t >= rs.col[ci + 1].base) ci++;
    const MulCol& col = rs.col[ci];
    const BalInst& in = a.inst[col.inst];
    const u64* p1 = ma.inst[col.inst].planes1;
    const u64 r = t - col.base;
    for (u32 s = col.s_begin; s < col.s_end; s++) {
      const u32 k = rs.slot_k[s];
      const u64 b = gl_sub(mul_value1(a, in, p1, 2 * k, r).c0, bal_value(a, in, 2 * k, r).c0);
      if (!b) continue;
      const u64 id = in.base + r * in.K + k;
      const u64 slot = bal_probe<false>(a, tb, bal_value(a, in, 2 * k + 1, r), id);
      u64 v = 0;
      if (tb.claim[slot] && owner[slot] == id) v = gl_mul(gl_neg(tb.lo[0][slot]), gl_inv(b));
      col.cell[r] = v;
      wrote = 1;
      break;
    }
  }
  sc[threadIdx.x] = wrote;
  __syncthreads();
  for (int off = BT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) sc[threadIdx.x] += sc[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sc[0]) atomicAdd(written, (unsigned long long)sc[0]);
}

namespace {
std::string slot_name(const FillInput& f, const char* const* names, u32 column, u32 fraction) {
  char buf[128];
  if (names) snprintf(buf, sizeof buf, "%s (instance %d) column %u fraction %u", names[f.label], f.label, column, fraction);
  else snprintf(buf, sizeof buf, "instance %d column %u fraction %u", f.label, column, fraction);
  return buf;
}
}  // namespace

// slots[i].instance indexes `in` (balance.cuh: range_table.hip runs it as its last stage)
void fill_run(mh_ctx* c, const std::vector<FillInput>& in, const std::vector<e2>& rnd, const std::vector<BoundaryPush>& boundary,
              const std::vector<mh_mult_slot>& slots, const char* const* names, u64* n_written, BalanceReport& rep) {
  const size_t n_in = in.size();
  *n_written = 0;
  std::vector<BalanceInput> bin;
  for (const FillInput& f : in) bin.push_back(f.b);
  if (slots.empty()) {
    balance_run(c, bin, rnd, boundary, true, rep);
    return;
  }
  // ---- the declaration: per instance the fractions that are slots, per declared column its slots in order ----
  std::vector<u32> frac_off(n_in + 1, 0);
  for (size_t i = 0; i < n_in; i++) frac_off[i + 1] = frac_off[i] + (u32)in[i].b.lk->n_fractions();
  std::vector<u32> slot_col(std::max<u32>(1, frac_off[n_in]), 0);
  std::vector<std::vector<u32>> declared(n_in);  // per instance its declared columns, first appearance first
  auto global_k = [&](const mh_mult_slot& s) {
    u32 k = s.fraction;
    for (u32 col = 0; col < s.lookup_column; col++) k += in[s.instance].b.lk->col_count[col];
    return k;
  };
  for (const mh_mult_slot& s : slots) {
    u32& sc = slot_col[frac_off[s.instance] + global_k(s)];
    MH_REQUIRE(!sc, "two multiplicity slots name " + slot_name(in[s.instance], names, s.lookup_column, s.fraction));
    sc = s.main_column + 1;
    auto& d = declared[s.instance];
    if (std::find(d.begin(), d.end(), s.main_column) == d.end()) d.push_back(s.main_column);
  }
  std::vector<MulCol> cols;
  std::vector<u32> slot_k;
  u64 cells = 0;
  for (size_t i = 0; i < n_in; i++)
    for (u32 mc : declared[i]) {
      const u64 n = (u64)1 << in[i].main->log_n;
      MulCol col{cells, in[i].main->cols.u() + (size_t)mc * n, (u32)i, (u32)slot_k.size(), 0};
      for (const mh_mult_slot& s : slots)
        if ((size_t)s.instance == i && s.main_column == mc) slot_k.push_back(global_k(s));
      col.s_end = (u32)slot_k.size();
      cols.push_back(col);
      cells += n;
    }

  // ---- probe: P0 (every instance), P1 (the declaring ones) ----
  std::vector<DevBuf> p0(n_in), p1(n_in);
  DevBuf bplanes;
  std::vector<BalInst> inst;
  std::vector<MulInst> minst;
  std::vector<unsigned char> ext;
  u64 total = 0;
  {
    ProfScope ps(c, "fill_planes");
    for (size_t i = 0; i < n_in; i++) {
      const mh_lookup* lk = in[i].b.lk;
      const mh_trace* tr = in[i].main;
      const u64 n = (u64)1 << tr->log_n;
      if (declared[i].empty()) {
        lookup_planes(c, lk, tr, in[i].b.prep, rnd, p0[i]);
      } else {
        mh_trace scratch;
        scratch.ctx = c; scratch.log_n = tr->log_n; scratch.width = tr->width;
        scratch.cols.alloc(tr->width * n * 8);
        DevBuf dlist(declared[i].size() * 4);
        c->h2d(dlist.p, declared[i].data(), declared[i].size() * 4);
        trace_wait_ready(c, tr);
        HIP_CHECK(hipMemcpyAsync(scratch.cols.p, tr->cols.p, tr->width * n * 8, hipMemcpyDeviceToDevice, c->stream));
        const u32 nl = (u32)declared[i].size();
        MH_LAUNCH(k_mul_fill, dim3(grid_for(n * nl)), dim3(BT), 0, c->stream, scratch.cols.u(), n, (const u32*)dlist.p, nl, (u64)0);
        lookup_planes(c, lk, &scratch, in[i].b.prep, rnd, p0[i]);
        MH_LAUNCH(k_mul_fill, dim3(grid_for(n * nl)), dim3(BT), 0, c->stream, scratch.cols.u(), n, (const u32*)dlist.p, nl, (u64)1);
        lookup_planes(c, lk, &scratch, in[i].b.prep, rnd, p1[i]);
      }
      inst.push_back(BalInst{p0[i].u(), n, total, (u32)lk->n_fractions(), (u32)ext.size(), tr->log_n});
      minst.push_back(MulInst{p1[i].u(), frac_off[i]});
      ext.insert(ext.end(), lk->out_ext.begin(), lk->out_ext.begin() + 2 * lk->n_fractions());
      total += n * lk->n_fractions();
    }
  }
  const size_t nb = boundary.size();
  if (nb) {
    balance_boundary_planes(c, boundary, bplanes);
    inst.push_back(BalInst{bplanes.u(), (u64)nb, total, 1, (u32)ext.size(), 63});
    minst.push_back(MulInst{nullptr, 0});
    ext.push_back(0);
    ext.push_back(1);
    total += nb;
  }
  MH_REQUIRE(total < ((u64)1 << 40), "too many pushes for one multiplicity fill");
  DevBuf dinst(inst.size() * sizeof(BalInst)), dminst(minst.size() * sizeof(MulInst)), dext(ext.size()), dslot(slot_col.size() * 4);
  DevBuf dcols(cols.size() * sizeof(MulCol)), dslotk(slot_k.size() * 4), words(4 * 8);
  c->h2d(dinst.p, inst.data(), inst.size() * sizeof(BalInst));
  c->h2d(dminst.p, minst.data(), minst.size() * sizeof(MulInst));
  c->h2d(dext.p, ext.data(), ext.size());
  c->h2d(dslot.p, slot_col.data(), slot_col.size() * 4);
  c->h2d(dcols.p, cols.data(), cols.size() * sizeof(MulCol));
  c->h2d(dslotk.p, slot_k.data(), slot_k.size() * 4);
  const u64 init[4] = {~(u64)0, 0, 0, 0};  // bad, zero, count, written
  c->h2d(words.p, init, sizeof init);
  BalArgs a{(const BalInst*)dinst.p, (u32)inst.size(), (const unsigned char*)dext.p, total};
  MulArgs ma{(const MulInst*)dminst.p, (const u32*)dslot.p};
  unsigned long long* w = (unsigned long long*)words.p;
  {
    ProfScope ps(c, "fill_probe", 48.0 * (double)total);
    MH_LAUNCH(k_mul_probe, dim3(grid_for(total)), dim3(BT), 0, c->stream, a, ma, w, (u32*)(w + 1), w + 2);
  }
  u64 got[4];
  c->d2h(got, words.p, sizeof got);
  c->sync();
  if (got[0] != ~(u64)0) {
    const size_t i = (size_t)(got[0] >> 32);
    u32 k = (u32)((got[0] & 0xFFFFFFFFu) >> 2), col = 0;
    while (k >= in[i].b.lk->col_count[col]) k -= in[i].b.lk->col_count[col++];
    const std::string who = slot_name(in[i], names, col, k);
    switch (got[0] & 3) {
      case MUL_BAD_KEY: throw MhError(MH_ERR_INVALID, "multiplicity slot " + who + ": its denominator reads a declared column (the key depends on a multiplicity cell)");
      case MUL_BAD_EF: throw MhError(MH_ERR_INVALID, "multiplicity slot " + who + ": the coefficient of its column is EF-valued (a cell is a base-field value)");
      default: throw MhError(MH_ERR_INVALID, "undeclared reader: " + who + " reads a declared multiplicity column and is not a slot");
    }
  }
  MH_REQUIRE((u32)got[1] == 0, "LogUp denominator is zero on a live push (aux_builder.rs:226-228: bus_prefix is never zero)");
  const u64 live = got[2];
  if (live) {
    // ---- insert, final, resolve ----
    u64 S = 1024;
    while (S < 2 * live) S <<= 1;  // load factor <= 1/2
    DevBuf table(7 * S * 8);
    BalTable tb{};
    unsigned long long* tw = (unsigned long long*)table.p;
    tb.claim = tw; tb.lo[0] = tw + S; tb.hi[0] = tw + 2 * S; tb.lo[1] = tw + 3 * S; tb.hi[1] = tw + 4 * S; tb.cnt = tw + 5 * S;
    tb.mask = S - 1;
    unsigned long long* owner = tw + 6 * S;
    MulResolve rs{(const MulCol*)dcols.p, (const u32*)dslotk.p, (u32)cols.size(), cells};
    {
      ProfScope ps(c, "fill_insert", 56.0 * (double)S + 36.0 * (double)total);
      HIP_CHECK(hipMemsetAsync(table.p, 0, 6 * S * 8, c->stream));
      HIP_CHECK(hipMemsetAsync(owner, 0xFF, S * 8, c->stream));
      MH_LAUNCH(k_mul_insert, dim3(grid_for(total)), dim3(BT), 0, c->stream, a, ma, tb, owner);
      MH_LAUNCH(k_mul_final, dim3(grid_for(S)), dim3(BT), 0, c->stream, tb);
    }
    {
      ProfScope ps(c, "fill_resolve", 40.0 * (double)cells);
      MH_LAUNCH(k_mul_resolve, dim3(grid_for(cells)), dim3(BT), 0, c->stream, a, ma, rs, tb, (const unsigned long long*)owner, w + 3);
    }
    c->d2h(got, words.p, sizeof got);
    c->sync();
    *n_written = got[3];
  }
  // ---- verify: the exact balance stage over the filled traces; the planes of the instances that declared nothing are still good ----
  for (size_t i = 0; i < n_in; i++) {
    p1[i].release();
    if (!declared[i].empty()) p0[i].release();
  }
  balance_run(c, bin, rnd, boundary, true, rep, &p0);
}

namespace {
// the caller's slots -> instance = index into `in`; index_of[instance]: that index, or -1 (an AIR without a lookup program)
std::vector<mh_mult_slot> fill_slots(mh_ctx* c, const std::vector<FillInput>& in, const std::vector<int>& index_of, const mh_mult_slot* slots,
                                     size_t n_slots) {
  MH_REQUIRE(slots || !n_slots, "null slot array");
  std::vector<mh_mult_slot> out;
  for (size_t j = 0; j < n_slots; j++) {
    mh_mult_slot s = slots[j];
    char buf[160];
    snprintf(buf, sizeof buf, "multiplicity slot %zu (instance %d column %u fraction %u, main column %u) is out of range", j, s.instance,
             s.lookup_column, s.fraction, s.main_column);
    MH_REQUIRE(s.instance >= 0 && (size_t)s.instance < index_of.size() && index_of[s.instance] >= 0, buf);
    s.instance = index_of[s.instance];
    const FillInput& f = in[s.instance];
    MH_REQUIRE(s.lookup_column < f.b.lk->num_cols && s.fraction < f.b.lk->col_count[s.lookup_column] && s.main_column < f.main->width, buf);
    out.push_back(s);
  }
  return out;
}
}  // namespace

int fill_statement(mh_ctx* c, int n_airs, mh_air* const* airs, mh_trace* const* traces, const mh_trace* const* preps,
                   const u64 challenger_state[12], const u64* pre_observe, size_t n_pre,
                   const std::function<bool(const std::vector<e2>&, std::vector<BoundaryPush>&)>& boundary, const char* const* names,
                   const mh_mult_slot* slots, size_t n_slots, uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap, size_t* n_entries,
                   mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n_written && n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    *n_entries = *n_pushes = 0;
    *n_written = 0;
    MH_REQUIRE_NO_SALT(c, "mh_fill_multiplicities*");
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
    const std::vector<mh_mult_slot> sl = fill_slots(c, in, index_of, slots, n_slots);
    const std::vector<e2> rnd = debug_challenges(challenger_state, pre_observe, n_pre, n_airs, traces, max_rand);
    std::vector<BoundaryPush> bnd;
    MH_REQUIRE(boundary(rnd, bnd), "the statement's boundary pushes could not be evaluated (a zero denominator)");
    BalanceReport rep;
    fill_run(c, in, rnd, bnd, sl, names, n_written, rep);
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

extern "C" int mh_fill_multiplicities(mh_ctx* c, int n, const mh_lookup* const* lookups, mh_trace* const* traces,
                                      const mh_trace* const* preprocessed, const uint64_t* randomness, size_t n_randomness,
                                      const uint64_t* boundary_denoms, const int32_t* boundary_signs, size_t n_boundary,
                                      const mh_mult_slot* slots, size_t n_slots, uint64_t* n_written, mh_balance_entry* entries,
                                      size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n >= 0 && n <= 256 && (!n || (lookups && traces)), "between 0 and 256 instances, with their arrays");
    MH_REQUIRE(n_written && n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    MH_REQUIRE((randomness || !n_randomness) && ((boundary_denoms && boundary_signs) || !n_boundary), "null value array");
    *n_entries = *n_pushes = 0;
    *n_written = 0;
    MH_REQUIRE_NO_SALT(c, "mh_fill_multiplicities*");
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
    const std::vector<mh_mult_slot> sl = fill_slots(c, in, index_of, slots, n_slots);
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
    fill_run(c, in, rnd, bnd, sl, nullptr, n_written, rep);
    return balance_report(c, rep, nullptr, entries, entry_cap, n_entries, pushes, push_cap, n_pushes);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}
