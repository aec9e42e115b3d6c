// Bus-balance checker (mh_check_balance*), gfx950.
//
// Replaces air/src/lookup/debug/trace/mod.rs:44-95,161-189 (check_trace_balance: a row-by-row walk with a HashMap from encoded
// denominator to signed multiplicity; BalanceReport / Unmatched / PushRecord), folded over a statement's instances and boundary pushes as
// precompiles-prover/src/tests/bus_balance.rs:25-108 does.  Input: the planes the compiled lookup programs write (logup.hip
// lookup_planes), one (m, d) per fraction and row; the statement's boundary pushes come in as one more instance of K = 1 fractions.
//   screen  sum of m / d over all live pushes (m != 0): one batched inversion per thread, workgroup sums, one workgroup adds them.
//           Zero: balanced except with probability ~ #pushes / p^2 over the challenges.  The same pass counts the live pushes.
//   exact   one open-addressing table in HBM for the whole statement, sized to a power of two >= 2 * (live pushes) (load <= 1/2).
//           A slot is claimed by a 64-bit compare-and-swap of (push id + 1); a key is compared by re-reading the claimant's denominator
//           from the planes, so no 128-bit key is ever written by two lanes.  Multiplicities are netted per coordinate by a 64-bit
//           atomic add on a low word, the carry out of it (seen in the returned old value) by an atomic add on a high word; the pair is
//           reduced mod p afterwards.  Integer addition does not depend on arrival order.  WHERE a key lands does (linear probing), so
//           nothing of the slot order reaches the report: the slots with a non-zero net are compacted, their entries sorted by
//           denominator on the host, and a second pass over the pushes finds each live push's slot and keeps those of reported entries.
// push id = instance base + row * K + fraction; lane order inside an instance is fraction-major (consecutive lanes = consecutive rows of
// one plane: coalesced).
#include "balance.cuh"
#include <algorithm>
#include <memory>
#include <string>

static constexpr size_t BAL_MAX_COLLECT = (size_t)1 << 22;  // pushes collected for a report (include/midenhip.h)
static constexpr int BI = 4, BTILE = BT * BI;

// ---- pass 1: live count per tile, zero denominators, (SCREEN) sum of m / d per tile ----
template <bool SCREEN>
__global__ __launch_bounds__(BT) void k_bal_scan(BalArgs a, u64* __restrict__ tile_cnt, u64* __restrict__ tile_sum, size_t tiles, u32* err) {
  __shared__ u64 s0[BT], s1[BT], sc[BT];
  const u64 t0 = (u64)blockIdx.x * BTILE + threadIdx.x;
  e2 m[BI], d[BI];
  u64 live = 0;
#pragma unroll
  for (int i = 0; i < BI; i++) {
    const u64 t = t0 + (u64)i * BT;
    m[i] = e2_make(0);
    d[i] = e2_make(1);
    if (t >= a.total) continue;
    const BalLane ln = bal_lane(a, t);
    const e2 mm = bal_value(a, *ln.in, 2 * ln.k, ln.row);
    if (e2_is_zero(mm)) continue;  // not a push (and the reference never pushed it)
    const e2 dd = bal_value(a, *ln.in, 2 * ln.k + 1, ln.row);
    if (e2_is_zero(dd)) {
      atomicOr(err, 1u);
      continue;
    }
    live++;
    m[i] = mm;
    d[i] = dd;
  }
  e2 sum = e2_make(0);
  if (SCREEN && live) {  // one inversion for the lane's BI denominators (dead lanes carry d = 1, m = 0)
    e2 pre[BI];
    pre[0] = d[0];
#pragma unroll
    for (int i = 1; i < BI; i++) pre[i] = e2_mul(pre[i - 1], d[i]);
    e2 inv = e2_inv(pre[BI - 1]);
#pragma unroll
    for (int i = BI - 1; i >= 0; i--) {
      const e2 di = i ? e2_mul(inv, pre[i - 1]) : inv;
      inv = e2_mul(inv, d[i]);
      sum = e2_add(sum, e2_mul(di, m[i]));
    }
  }
  s0[threadIdx.x] = sum.c0;
  s1[threadIdx.x] = sum.c1;
  sc[threadIdx.x] = live;
  __syncthreads();
  for (int off = BT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) {
      sc[threadIdx.x] += sc[threadIdx.x + off];
      if (SCREEN) {
        s0[threadIdx.x] = gl_add(s0[threadIdx.x], s0[threadIdx.x + off]);
        s1[threadIdx.x] = gl_add(s1[threadIdx.x], s1[threadIdx.x + off]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = sc[0];
    tile_sum[blockIdx.x] = s0[0];
    tile_sum[tiles + blockIdx.x] = s1[0];
  }
}
// one workgroup: the tiles' counts and sums -> out[0] = live pushes, out[1..2] = sum of m / d
__global__ __launch_bounds__(BT) void k_bal_totals(const u64* __restrict__ tile_cnt, const u64* __restrict__ tile_sum, size_t tiles,
                                                   u64* __restrict__ out) {
  __shared__ u64 s0[BT], s1[BT], sc[BT];
  u64 c = 0, x0 = 0, x1 = 0;
  for (size_t i = threadIdx.x; i < tiles; i += BT) {
    c += tile_cnt[i];
    x0 = gl_add(x0, tile_sum[i]);
    x1 = gl_add(x1, tile_sum[tiles + i]);
  }
  s0[threadIdx.x] = x0;
  s1[threadIdx.x] = x1;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int off = BT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) {
      sc[threadIdx.x] += sc[threadIdx.x + off];
      s0[threadIdx.x] = gl_add(s0[threadIdx.x], s0[threadIdx.x + off]);
      s1[threadIdx.x] = gl_add(s1[threadIdx.x], s1[threadIdx.x + off]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sc[0];
    out[1] = s0[0];
    out[2] = s1[0];
  }
}

// ---- pass 2: net every live push into its key's slot ----
__global__ __launch_bounds__(BT) void k_bal_insert(BalArgs a, BalTable tb) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= a.total) return;
  const BalLane ln = bal_lane(a, t);
  const e2 m = bal_value(a, *ln.in, 2 * ln.k, ln.row);
  if (e2_is_zero(m)) return;
  const e2 d = bal_value(a, *ln.in, 2 * ln.k + 1, ln.row);
  const u64 slot = bal_probe<true>(a, tb, d, ln.id);
  bal_accumulate(tb, slot, m);
  atomicAdd(&tb.cnt[slot], 1ULL);
}
// per slot: (hi, lo) -> the net multiplicity mod p (into lo); flag = it is not zero
__global__ __launch_bounds__(BT) void k_bal_final(BalTable tb, u32* __restrict__ flags) {
  const u64 s = (u64)blockIdx.x * BT + threadIdx.x;
  if (s > tb.mask) return;
  u32 f = 0;
  if (tb.claim[s]) f = bal_reduce_slot(tb, s);
  flags[s] = f;
}
// the reported slots -> {denom c0, c1, net c0, c1, pushes, slot}
__global__ __launch_bounds__(BT) void k_bal_entries(BalArgs a, BalTable tb, const u64* __restrict__ slots, size_t m, u64* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BT + threadIdx.x;
  if (i >= m) return;
  const u64 s = slots[i];
  const e2 d = bal_denominator(a, tb.claim[s] - 1);
  u64* o = out + 6 * i;
  o[0] = d.c0; o[1] = d.c1; o[2] = tb.lo[0][s]; o[3] = tb.lo[1][s]; o[4] = tb.cnt[s]; o[5] = s;
}
// rank[slot of entry i] = i + 1 (entries in report order)
__global__ __launch_bounds__(BT) void k_bal_rank(const u64* __restrict__ slots, size_t m, u32* __restrict__ rank) {
  const size_t i = (size_t)blockIdx.x * BT + threadIdx.x;
  if (i < m) rank[slots[i]] = (u32)(i + 1);
}
// ---- pass 3: every live push looks its slot up; mark[lane] = its entry + 1, or 0 ----
__global__ __launch_bounds__(BT) void k_bal_mark(BalArgs a, BalTable tb, const u32* __restrict__ rank, u32* __restrict__ mark) {
  const u64 t = (u64)blockIdx.x * BT + threadIdx.x;
  if (t >= a.total) return;
  const BalLane ln = bal_lane(a, t);
  const e2 m = bal_value(a, *ln.in, 2 * ln.k, ln.row);
  u32 v = 0;
  if (!e2_is_zero(m)) v = rank[bal_probe<false>(a, tb, bal_value(a, *ln.in, 2 * ln.k + 1, ln.row), ln.id)];
  mark[t] = v;
}
// the marked lanes -> {push id, entry, multiplicity c0, c1}
__global__ __launch_bounds__(BT) void k_bal_pushes(BalArgs a, const u32* __restrict__ mark, const u64* __restrict__ lanes, size_t m,
                                                   u64* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BT + threadIdx.x;
  if (i >= m) return;
  const u64 t = lanes[i];
  const BalLane ln = bal_lane(a, t);
  const e2 mm = bal_value(a, *ln.in, 2 * ln.k, ln.row);
  u64* o = out + 4 * i;
  o[0] = ln.id; o[1] = mark[t] - 1; o[2] = mm.c0; o[3] = mm.c1;
}

void balance_boundary_planes(mh_ctx* c, const std::vector<BoundaryPush>& boundary, DevBuf& planes) {
  const size_t nb = boundary.size();
  std::vector<u64> h(4 * nb, 0);
  for (size_t i = 0; i < nb; i++) {
    h[i] = boundary[i].sign > 0 ? 1 : GL_P - 1;
    h[2 * nb + i] = boundary[i].denom.c0;
    h[3 * nb + i] = boundary[i].denom.c1;
  }
  planes.alloc(h.size() * 8);
  HIP_CHECK(hipMemcpyAsync(planes.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));  // `h` is pageable and leaves scope
}

void balance_run(mh_ctx* c, const std::vector<BalanceInput>& in, const std::vector<e2>& rnd, const std::vector<BoundaryPush>& boundary,
                 bool exact, BalanceReport& rep, std::vector<DevBuf>* have) {
  const size_t n_in = in.size();
  // the planes of every instance stay alive together: the table compares keys by re-reading them
  std::vector<DevBuf> planes(n_in);
  DevBuf bplanes;
  std::vector<BalInst> inst;
  std::vector<unsigned char> ext;
  u64 total = 0;
  {
    ProfScope ps(c, "balance_planes");
    for (size_t i = 0; i < n_in; i++) {
      const mh_lookup* lk = in[i].lk;
      if (have && (*have)[i].p) planes[i] = std::move((*have)[i]);
      else lookup_planes(c, lk, in[i].main, in[i].prep, rnd, planes[i]);
      const u64 n = (u64)1 << in[i].main->log_n;
      inst.push_back(BalInst{planes[i].u(), n, total, (u32)lk->n_fractions(), (u32)ext.size(), in[i].main->log_n});
      ext.insert(ext.end(), lk->out_ext.begin(), lk->out_ext.begin() + 2 * lk->n_fractions());
      total += n * lk->n_fractions();
    }
  }
  const size_t nb = boundary.size();
  if (nb) {  // one more instance: K = 1, m = +-1 (base field), d = the denominator
    balance_boundary_planes(c, boundary, bplanes);
    inst.push_back(BalInst{bplanes.u(), (u64)nb, total, 1, (u32)ext.size(), 63});
    ext.push_back(0);
    ext.push_back(1);
    total += nb;
  }
  if (!total) return;
  MH_REQUIRE(total < ((u64)1 << 40), "too many pushes for one balance check");
  DevBuf dinst(inst.size() * sizeof(BalInst)), dext(ext.size()), derr(4);
  c->h2d(dinst.p, inst.data(), inst.size() * sizeof(BalInst));
  c->h2d(dext.p, ext.data(), ext.size());
  HIP_CHECK(hipMemsetAsync(derr.p, 0, 4, c->stream));
  BalArgs a{(const BalInst*)dinst.p, (u32)inst.size(), (const unsigned char*)dext.p, total};

  // pass 1
  const size_t tiles = (size_t)((total + BTILE - 1) / BTILE);
  DevBuf tile_cnt(tiles * 8), tile_sum(2 * tiles * 8), totals(3 * 8);
  {
    ProfScope ps(c, exact ? "balance_count" : "balance_screen", 24.0 * (double)total);
    if (exact) MH_LAUNCH(k_bal_scan<false>, dim3((unsigned)tiles), dim3(BT), 0, c->stream, a, tile_cnt.u(), tile_sum.u(), tiles, (u32*)derr.p);
    else MH_LAUNCH(k_bal_scan<true>, dim3((unsigned)tiles), dim3(BT), 0, c->stream, a, tile_cnt.u(), tile_sum.u(), tiles, (u32*)derr.p);
    MH_LAUNCH(k_bal_totals, dim3(1), dim3(BT), 0, c->stream, tile_cnt.u(), tile_sum.u(), tiles, totals.u());
  }
  u64 tot[3];
  u32 err = 0;
  c->d2h(tot, totals.p, 24);
  c->d2h(&err, derr.p, 4);
  c->sync();
  MH_REQUIRE(err == 0, "LogUp denominator is zero on a live push (aux_builder.rs:226-228: bus_prefix is never zero)");
  const u64 live = tot[0];
  if (!live || (!exact && (tot[1] | tot[2]) == 0)) return;

  // pass 2: the table
  u64 S = 1024;
  while (S < 2 * live) S <<= 1;  // load factor <= 1/2
  DevBuf table(6 * S * 8), sflag(S * 4), slots(S * 8);
  BalTable tb{};
  unsigned long long* w = (unsigned long long*)table.p;
  tb.claim = w; tb.lo[0] = w + S; tb.hi[0] = w + 2 * S; tb.lo[1] = w + 3 * S; tb.hi[1] = w + 4 * S; tb.cnt = w + 5 * S;
  tb.mask = S - 1;
  size_t m;
  {
    ProfScope ps(c, "balance_exact", 48.0 * (double)S + 24.0 * (double)total);
    HIP_CHECK(hipMemsetAsync(table.p, 0, 6 * S * 8, c->stream));
    MH_LAUNCH(k_bal_insert, dim3(grid_for(total)), dim3(BT), 0, c->stream, a, tb);
    MH_LAUNCH(k_bal_final, dim3(grid_for(S)), dim3(BT), 0, c->stream, tb, (u32*)sflag.p);
    m = compact_rows(c, (const u32*)sflag.p, (size_t)S, slots.u());
  }
  if (!m) return;
  MH_REQUIRE(m < 0xFFFFFFFFu, "too many unmatched denominators");
  std::vector<u64> raw(6 * m);
  {
    DevBuf dent(6 * m * 8);
    MH_LAUNCH(k_bal_entries, dim3(grid_for(m)), dim3(BT), 0, c->stream, a, tb, slots.u(), m, dent.u());
    HIP_CHECK(hipMemcpyAsync(raw.data(), dent.p, 6 * m * 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
  }
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {  // denominators are distinct: a total order
    return raw[6 * x] != raw[6 * y] ? raw[6 * x] < raw[6 * y] : raw[6 * x + 1] < raw[6 * y + 1];
  });
  rep.entries.resize(m);
  std::vector<u64> sorted_slots(m);
  size_t n_pushes = 0;
  for (size_t i = 0; i < m; i++) {
    const u64* r = &raw[6 * order[i]];
    rep.entries[i] = mh_balance_entry{{r[0], r[1]}, {r[2], r[3]}, r[4], n_pushes};
    sorted_slots[i] = r[5];
    n_pushes += r[4];
  }
  rep.n_pushes = n_pushes;
  if (n_pushes > BAL_MAX_COLLECT) {
    for (auto& e : rep.entries) e.first_push = MH_BALANCE_NO_PUSHES;
    return;
  }

  // pass 3: the pushes of the reported entries
  DevBuf rank(S * 4), mark(total * 4), lanes(total * 8);
  size_t np;
  {
    ProfScope ps(c, "balance_pushes", 28.0 * (double)total);
    HIP_CHECK(hipMemcpyAsync(slots.p, sorted_slots.data(), m * 8, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemsetAsync(rank.p, 0, S * 4, c->stream));
    MH_LAUNCH(k_bal_rank, dim3(grid_for(m)), dim3(BT), 0, c->stream, slots.u(), m, (u32*)rank.p);
    MH_LAUNCH(k_bal_mark, dim3(grid_for(total)), dim3(BT), 0, c->stream, a, tb, (const u32*)rank.p, (u32*)mark.p);
    np = compact_rows(c, (const u32*)mark.p, (size_t)total, lanes.u());  // waits: sorted_slots has been read
  }
  if (np != n_pushes) throw MhError(MH_ERR_INTERNAL, "balance: the push pass disagrees with the table's counts");
  std::vector<u64> praw(4 * np);
  {
    DevBuf dp(4 * np * 8);
    MH_LAUNCH(k_bal_pushes, dim3(grid_for(np)), dim3(BT), 0, c->stream, a, (const u32*)mark.p, lanes.u(), np, dp.u());
    HIP_CHECK(hipMemcpyAsync(praw.data(), dp.p, 4 * np * 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
  }
  std::vector<size_t> po(np);
  for (size_t i = 0; i < np; i++) po[i] = i;
  std::sort(po.begin(), po.end(), [&](size_t x, size_t y) {  // (entry, push id): push ids are distinct
    return praw[4 * x + 1] != praw[4 * y + 1] ? praw[4 * x + 1] < praw[4 * y + 1] : praw[4 * x] < praw[4 * y];
  });
  rep.pushes.resize(np);
  for (size_t i = 0; i < np; i++) {
    const u64* r = &praw[4 * po[i]];
    size_t k = inst.size() - 1;
    while (r[0] < inst[k].base) k--;
    const u64 l = r[0] - inst[k].base;
    mh_balance_push p{};
    p.row = l / inst[k].K;
    p.multiplicity[0] = r[2];
    p.multiplicity[1] = r[3];
    if (k >= n_in) {  // a boundary push: its index in the statement's list
      p.instance = -1;
      p.column = 0;
      p.fraction = (uint32_t)l;
      p.row = 0;
    } else {
      u32 f = (u32)(l % inst[k].K), col = 0;
      while (f >= in[k].lk->col_count[col]) f -= in[k].lk->col_count[col++];
      p.instance = (int32_t)k;
      p.column = col;
      p.fraction = f;
    }
    rep.pushes[i] = p;
  }
}

// copy out, count, name the first entry
int balance_report(mh_ctx* c, const BalanceReport& rep, const char* const* names, mh_balance_entry* entries, size_t entry_cap,
                   size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  *n_entries = rep.entries.size();
  *n_pushes = rep.n_pushes;
  for (size_t i = 0; i < rep.entries.size() && i < entry_cap; i++) entries[i] = rep.entries[i];
  for (size_t i = 0; i < rep.pushes.size() && i < push_cap; i++) pushes[i] = rep.pushes[i];
  if (rep.entries.empty()) return MH_OK;
  const mh_balance_entry& e = rep.entries[0];
  char where[160] = "pushes not collected";
  if (!rep.pushes.empty()) {
    const mh_balance_push& p = rep.pushes[0];
    if (p.instance < 0) snprintf(where, sizeof where, "first push: boundary push %u", p.fraction);
    else if (names)
      snprintf(where, sizeof where, "first push: %s row %llu column %u fraction %u", names[p.instance], (unsigned long long)p.row, p.column,
               p.fraction);
    else
      snprintf(where, sizeof where, "first push: instance %d row %llu column %u fraction %u", p.instance, (unsigned long long)p.row, p.column,
               p.fraction);
  }
  char buf[384];
  snprintf(buf, sizeof buf, "%zu unmatched denominators; (%llu, %llu): net (%llu, %llu) over %llu pushes, %s", rep.entries.size(),
           (unsigned long long)e.denom[0], (unsigned long long)e.denom[1], (unsigned long long)e.net[0], (unsigned long long)e.net[1],
           (unsigned long long)e.pushes, where);
  c->err = buf;
  return MH_ERR_UNSATISFIED;
}

void balance_validate(mh_ctx* c, const std::vector<BalanceInput>& in) {
  for (const BalanceInput& b : in) {
    MH_REQUIRE(b.lk && b.main, "null lookup program or trace");
    MH_REQUIRE(b.lk->ctx == c && b.main->ctx == c && (!b.prep || b.prep->ctx == c), "lookup program / trace of another context");
    MH_REQUIRE(b.main->width == b.lk->main_width, "trace width does not match the lookup program");
  }
}

int balance_statement(mh_ctx* c, int n_airs, mh_air* const* airs, mh_trace* const* traces, const mh_trace* const* preps,
                      const u64 challenger_state[12], const u64* pre_observe, size_t n_pre,
                      const std::function<bool(const std::vector<e2>&, std::vector<BoundaryPush>&)>& boundary, const char* const* names, int flags,
                      mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes) {
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    MH_REQUIRE((flags & ~MH_CHECK_EXACT) == 0, "unknown check flags");
    *n_entries = *n_pushes = 0;
    MH_REQUIRE_NO_SALT(c, "mh_check_balance*");
    HIP_CHECK(hipSetDevice(c->device));
    size_t max_rand = 0;
    std::vector<BalanceInput> in;
    std::vector<int> instance_of;  // instances without a lookup program have no buses
    for (int i = 0; i < n_airs; i++) {
      MH_REQUIRE(airs[i] && traces[i], "null AIR or trace");
      MH_REQUIRE(airs[i]->ctx == c && traces[i]->ctx == c, "AIR / trace of another context");
      MH_REQUIRE(!airs[i]->aux_width || airs[i]->lookup, "an AIR with aux columns needs its lookup program attached");
      max_rand = std::max(max_rand, airs[i]->num_randomness);
      if (!airs[i]->lookup) continue;
      in.push_back(BalanceInput{airs[i]->lookup, traces[i], preps && preps[i] ? preps[i] : airs[i]->prep_raw});
      instance_of.push_back(i);
    }
    balance_validate(c, in);
    const std::vector<e2> rnd = debug_challenges(challenger_state, pre_observe, n_pre, n_airs, traces, max_rand);
    std::vector<BoundaryPush> bnd;
    MH_REQUIRE(boundary(rnd, bnd), "the statement's boundary pushes could not be evaluated (a zero denominator)");
    BalanceReport rep;
    balance_run(c, in, rnd, bnd, (flags & MH_CHECK_EXACT) != 0, rep);
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

extern "C" int mh_check_balance(mh_ctx* c, int n, const mh_lookup* const* lookups, const mh_trace* const* traces,
                                const mh_trace* const* preprocessed, const uint64_t* randomness, size_t n_randomness,
                                const uint64_t* boundary_denoms, const int32_t* boundary_signs, size_t n_boundary, int flags,
                                mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap,
                                size_t* n_pushes) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(n >= 0 && n <= 256 && (!n || (lookups && traces)), "between 0 and 256 instances, with their arrays");
    MH_REQUIRE(n_entries && n_pushes && (entries || !entry_cap) && (pushes || !push_cap), "null argument");
    MH_REQUIRE((randomness || !n_randomness) && ((boundary_denoms && boundary_signs) || !n_boundary), "null value array");
    MH_REQUIRE((flags & ~MH_CHECK_EXACT) == 0, "unknown check flags");
    *n_entries = *n_pushes = 0;
    MH_REQUIRE_NO_SALT(c, "mh_check_balance*");
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<BalanceInput> in;
    for (int i = 0; i < n; i++) in.push_back(BalanceInput{lookups[i], traces[i], preprocessed ? preprocessed[i] : nullptr});
    balance_validate(c, in);
    std::vector<e2> rnd;
    for (size_t i = 0; i < n_randomness; i++) rnd.push_back(e2{gl_canon(randomness[2 * i]), gl_canon(randomness[2 * i + 1])});
    for (const BalanceInput& b : in) MH_REQUIRE(rnd.size() >= b.lk->num_randomness, "not enough lookup challenges");
    std::vector<BoundaryPush> bnd;
    for (size_t i = 0; i < n_boundary; i++) {
      MH_REQUIRE(boundary_signs[i] == 1 || boundary_signs[i] == -1, "a boundary sign is +1 or -1");
      bnd.push_back(BoundaryPush{e2{gl_canon(boundary_denoms[2 * i]), gl_canon(boundary_denoms[2 * i + 1])}, boundary_signs[i]});
      MH_REQUIRE(!e2_is_zero(bnd.back().denom), "a boundary denominator is zero");
    }
    BalanceReport rep;
    balance_run(c, in, rnd, bnd, (flags & MH_CHECK_EXACT) != 0, rep);
    return balance_report(c, rep, nullptr, entries, entry_cap, n_entries, pushes, push_cap, n_pushes);
  } catch (const MhError& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MH_ERR_INTERNAL;
  }
}
