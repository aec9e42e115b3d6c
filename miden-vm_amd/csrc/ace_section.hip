// The ACE chiplet's trace section built on the device from a list of circuit evaluations (mh_ace_section_build, mh_miden_ace_section),
// gfx950.
//
// Replaces eval_circuit (processor/src/execution/operations/eval_circuit.rs:54-118) and the ACE chiplet's trace (processor/src/trace/
// chiplets/ace/{mod,trace,instruction}.rs): an arithmetic circuit over F_p[x]/(x^2 - 7) evaluated gate by gate, every gate reading wires
// that earlier rows inserted, and every wire's fan-out as a multiplicity.  The workload that matters is one or a few circuits of many
// thousands of gates (the recursive verifier's constraint evaluation), so the parallelism is taken inside an evaluation.
//   plan      a lane per evaluation header, HS_TILE headers a block: kinds 1, 2, 3 (the lowest (evaluation, kind) -> one atomicMin); the
//             evaluation's rows and wires (0 for a defective one) are summed per tile -> agg[tile].
//   carries   k_hs_carries (hasher_section.hip): what every tile starts from, and the totals.
//   offsets   the tile scan again from the tile's carry: row0[e], wire0[e] (so gate0 = 2 row0 - wire0: n_read = wires - rows, num_eval =
//             2 rows - wires), and the lowest evaluation whose rows end beyond the target (kind 5).
//   gates     a lane per gate over all evaluations.  A wave finds the evaluation of its first gate by one wave-uniform binary search of
//             gate0[]; a lane walks on from there (an evaluation has at least 4 gates: at most 16 steps).  The lane reduces and decodes
//             its instruction, tests kind 4 (opcode above 2, or wire position nw - 1 - id not below 2 n_read + k) and adds 1 to each
//             operand wire's 32-bit counter.  The host reads the words back: the first wait.  Nothing but scratch has been written.
//   evaluate  a wave per evaluation, 64 gates a window, a lane a gate.  Operands that lie before the window are loaded at once (READ
//             wires from the felts, gate values from the value scratch); an operand inside the window belongs to a LOWER lane (kind 4).
//             A round: every pending lane whose in-window operands are finished (one 64-bit mask, from __ballot) takes their values
//             by __shfl, computes and finishes.  The lowest pending lane is always ready, so a window takes at most 64 rounds, and the
//             loop is bounded by 64 whatever the input.  A finished window's values go to the value scratch, 16 bytes a gate, and a
//             block barrier (one wave) orders them before the next window's loads.  The wave adds its rounds to n_rounds and tests the
//             last wire for zero (kind 6 -> atomicMin of the evaluation).  The host reads the words back: the second wait.
//   rows      a lane per row, the evaluation found as in `gates`: READ rows from the felts, EVAL rows gather v0, v_l, v_r; the
//             multiplicities from the counters; 16 column-major stores (+ 4 selectors in place).
// Sums and minima of integers: no output depends on the order the atomics land in; every output cell has one writer.
#include "section_out.cuh"
#include "hs_scan.cuh"

static_assert(sizeof(mh_ace_eval) == 32, "mh_ace_eval is 32 bytes");

namespace {
constexpr int ACE_BT = 256;
constexpr int ACE_WIDTH = 16;
constexpr u32 ACE_MAX_WIRES = (1u << 30) - 1;
constexpr u32 ACE_ID_MASK = (1u << 30) - 1;
constexpr unsigned long long ACE_NONE = ~0ull;

struct AceWords {                 // what the host reads back
  unsigned long long bad;         // min over kinds 1..3 of (evaluation << 3 | kind)
  unsigned long long bad_gate;    // min over kind 4 of (evaluation << 32 | gate)
  unsigned long long nofit;       // lowest evaluation whose rows end beyond the target
  unsigned long long n_rows;      // saturating
  unsigned long long n_wires;
  unsigned long long nonzero;     // lowest evaluation whose last wire is not zero
  unsigned long long n_rounds;
  unsigned long long unused;
};

struct AceRun {
  const mh_ace_eval* evals;
  u32 n_evals;
  const u64* felts;
  u64 n_felts;
  u64 cap_rows;
  u32* agg;       // [2][tiles]
  u32 tiles;
  u32* row0;      // [n_evals + 1]
  u32* wire0;     // [n_evals + 1]
  u32* gate0;     // [n_evals + 1]
  u32* count;     // [wires]: how often a gate names the wire
  e2* value;      // [gates]
  AceWords* w;
};

struct AcePlan {
  u32 rows, wires, defect;
};

// what evaluation `e` asks for, and the first defect it has in the order 1, 2, 3
__device__ __forceinline__ AcePlan ace_plan(const AceRun& r, u32 e) {
  const mh_ace_eval h = r.evals[e];
  AcePlan p{0, 0, 0};
  const u64 nw = (u64)h.num_vars + h.num_eval, need = 2 * (u64)h.num_vars + h.num_eval;
  if (h.num_vars == 0 || (h.num_vars & 1) || h.num_eval == 0 || (h.num_eval & 3) || nw > ACE_MAX_WIRES) p.defect = 1;
  else if (e && h.clk <= r.evals[e - 1].clk) p.defect = 2;
  else if (h.payload > r.n_felts || need > r.n_felts - h.payload || (u64)h.ptr + need > ((u64)1 << 32)) p.defect = 3;
  if (!p.defect) {
    p.rows = hs_sat(h.num_vars / 2 + h.num_eval);  // < 2^31 before the clamp
    p.wires = (u32)nw;
  }
  return p;
}

struct AceGate {
  u32 pos_l, pos_r, op;
  bool ok;
};

// gate k of an evaluation with n_read2 = 2 n_read READ wires and nw wires
__device__ __forceinline__ AceGate ace_decode(u64 felt, u32 nw, u32 n_read2, u32 k) {
  const u64 ins = gl_canon(felt);
  const u32 id_l = (u32)ins & ACE_ID_MASK, id_r = (u32)(ins >> 30) & ACE_ID_MASK;
  AceGate g;
  g.op = (u32)(ins >> 60);
  g.pos_l = nw - 1 - id_l;  // wraps for id >= nw: then it is not below the bound either
  g.pos_r = nw - 1 - id_r;
  const u32 bound = n_read2 + k;  // wires inserted before gate k
  g.ok = g.op <= 2 && id_l < nw && id_r < nw && g.pos_l < bound && g.pos_r < bound;
  return g;
}

struct AceAt {
  u32 e, local;  // the evaluation, and the index inside it
};

// The evaluation that holds item `i` of a partition given by its starts (start[n] = the total): the wave's first item by a wave-uniform
// binary search, the lane's own by walking on.  i < start[n]
__device__ __forceinline__ AceAt ace_find(const u32* __restrict__ start, u32 n, u32 i, u32 wave_first) {
  u32 lo = 0, hi = n;  // the last e with start[e] <= wave_first
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (start[mid] <= wave_first) lo = mid;
    else hi = mid;
  }
  while (lo + 1 < n && start[lo + 1] <= i) lo++;
  return AceAt{lo, i - start[lo]};
}

// the value of the wire at position `pos` of evaluation h: a READ wire from the felts, a gate's from the value scratch
__device__ __forceinline__ e2 ace_wire(const AceRun& r, const mh_ace_eval& h, u32 gate0, u32 pos) {
  if (pos < h.num_vars) {
    const u64* f = r.felts + h.payload + 2 * (size_t)pos;
    return e2{gl_canon(f[0]), gl_canon(f[1])};
  }
  return r.value[(size_t)gate0 + (pos - h.num_vars)];
}
}  // namespace

// ---- plan ----
__global__ __launch_bounds__(HS_BT) void k_ace_plan(AceRun r) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 a[HS_PER_LANE], b[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 e = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    a[j] = b[j] = 0;
    if (e < r.n_evals) {
      const AcePlan p = ace_plan(r, e);
      a[j] = p.rows;
      b[j] = p.wires;
      if (p.defect) atomicMin(&r.w->bad, ((unsigned long long)e << 3) | p.defect);
    }
  }
  hs_tile_scan(a, b, 0, 0, ea, eb, ta, tb, s_wave);
  if (threadIdx.x == 0) {
    r.agg[blockIdx.x] = ta;
    r.agg[r.tiles + blockIdx.x] = tb;
  }
}

__global__ __launch_bounds__(HS_BT) void k_ace_offsets(AceRun r) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 a[HS_PER_LANE], b[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 e = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    a[j] = b[j] = 0;
    if (e < r.n_evals) {
      const AcePlan p = ace_plan(r, e);
      a[j] = p.rows;
      b[j] = p.wires;
    }
  }
  hs_tile_scan(a, b, r.agg[blockIdx.x], r.agg[r.tiles + blockIdx.x], ea, eb, ta, tb, s_wave);
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 e = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    if (e >= r.n_evals) continue;
    r.row0[e] = ea[j];
    r.wire0[e] = eb[j];
    r.gate0[e] = 2 * ea[j] - eb[j];  // meaningful when nothing saturated: otherwise the call is refused
    if ((u64)ea[j] + a[j] > r.cap_rows) atomicMin(&r.w->nofit, (unsigned long long)e);
    if (e == r.n_evals - 1) {
      r.row0[e + 1] = hs_sat(ea[j] + a[j]);
      r.wire0[e + 1] = eb[j] + b[j];
      r.gate0[e + 1] = 2 * (ea[j] + a[j]) - (eb[j] + b[j]);
    }
  }
}

// ---- gates ----
__global__ __launch_bounds__(ACE_BT) void k_ace_gates(AceRun r, u32 max_wires) {
  const u32 g = blockIdx.x * ACE_BT + threadIdx.x;  // the grid covers what the headers say: < 2^25
  const u32 n_gates = r.gate0[r.n_evals];
  // an evaluation with one of kinds 1..3 takes no rows, wires or gates: the others keep consistent offsets, and their gates are tested,
  // because an earlier evaluation's kind 4 goes before a later one's kind 1
  if (r.w->n_rows > SEC_MAX_ROWS || g >= n_gates) return;  // the first: never (the host has summed the headers)
  const AceAt at = ace_find(r.gate0, r.n_evals, g, g & ~63u);
  const mh_ace_eval h = r.evals[at.e];
  const u32 k = at.local;
  if (k >= h.num_eval) return;  // never
  const u32 nw = h.num_vars + h.num_eval;
  const AceGate d = ace_decode(r.felts[h.payload + 2 * (size_t)h.num_vars + k], nw, h.num_vars, k);
  if (!d.ok) {
    atomicMin(&r.w->bad_gate, ((unsigned long long)at.e << 32) | k);
    return;
  }
  const u32 w0 = r.wire0[at.e];
  if (w0 + nw > max_wires) return;  // never: the counters were sized by the same headers
  atomicAdd(&r.count[w0 + d.pos_l], 1u);
  atomicAdd(&r.count[w0 + d.pos_r], 1u);
}

// ---- evaluate ----
__global__ __launch_bounds__(64) void k_ace_eval(AceRun r) {
  const u32 e = blockIdx.x, lane = threadIdx.x;
  const mh_ace_eval h = r.evals[e];
  const u32 nw = h.num_vars + h.num_eval, gate0 = r.gate0[e];
  const u64* ins = r.felts + h.payload + 2 * (size_t)h.num_vars;
  u32 rounds = 0;
  for (u32 base = 0; base < h.num_eval; base += 64) {  // wave-uniform
    const u32 k = base + lane, first = h.num_vars + base;  // the wire position of the window's lane 0
    bool pending = k < h.num_eval;
    AceGate d{0, 0, 0, false};
    if (pending) d = ace_decode(ins[k], nw, h.num_vars, k);
    pending = pending && d.ok;  // the host has refused a list with a gate that is not: such a lane keeps 0
    const bool l_in = pending && d.pos_l >= first, r_in = pending && d.pos_r >= first;
    const u32 jl = l_in ? d.pos_l - first : 0, jr = r_in ? d.pos_r - first : 0;  // lower lanes
    e2 vl{0, 0}, vr{0, 0}, v{0, 0};
    if (pending && !l_in) vl = ace_wire(r, h, gate0, d.pos_l);
    if (pending && !r_in) vr = ace_wire(r, h, gate0, d.pos_r);
    unsigned long long done = 0;
    for (int round = 0; round < 64; round++) {
      if (__ballot(pending) == 0) break;
      rounds++;
      const e2 sl{(u64)__shfl((unsigned long long)v.c0, (int)jl), (u64)__shfl((unsigned long long)v.c1, (int)jl)};
      const e2 sr{(u64)__shfl((unsigned long long)v.c0, (int)jr), (u64)__shfl((unsigned long long)v.c1, (int)jr)};
      const bool ready = pending && (!l_in || ((done >> jl) & 1)) && (!r_in || ((done >> jr) & 1));
      if (ready) {
        const e2 x = l_in ? sl : vl, y = r_in ? sr : vr;
        v = d.op == 0 ? e2_sub(x, y) : d.op == 1 ? e2_mul(x, y) : e2_add(x, y);
        pending = false;
      }
      done |= __ballot(ready);
    }
    if (k < h.num_eval) {
      *reinterpret_cast<ulonglong2*>(&r.value[(size_t)gate0 + k]) = make_ulonglong2(v.c0, v.c1);
      if (k == h.num_eval - 1 && !e2_is_zero(v)) atomicMin(&r.w->nonzero, (unsigned long long)e);
    }
    __syncthreads();  // one wave: the window's stores before the next window's loads
  }
  if (lane == 0) atomicAdd(&r.w->n_rounds, (unsigned long long)rounds);
}

// ---- rows ----
__global__ __launch_bounds__(ACE_BT) void k_ace_rows(AceRun r, u32 n_rows, SecOut o) {
  const u32 row = blockIdx.x * ACE_BT + threadIdx.x;
  if (row >= n_rows) return;
  const AceAt at = ace_find(r.row0, r.n_evals, row, row & ~63u);
  const mh_ace_eval h = r.evals[at.e];
  const u32 n_read = h.num_vars / 2, nw = h.num_vars + h.num_eval, w0 = r.wire0[at.e], gate0 = r.gate0[at.e];
  u64 c[ACE_WIDTH];
  c[2] = h.ctx;
  c[4] = h.clk;
  if (at.local < n_read) {
    const u32 i = at.local;
    const u64* f = r.felts + h.payload + 4 * (size_t)i;
    c[0] = i == 0;
    c[1] = 0;
    c[3] = h.ptr + 4 * i;
    c[5] = 0;
    c[6] = nw - 1 - 2 * i;
    c[7] = gl_canon(f[0]);
    c[8] = gl_canon(f[1]);
    c[9] = nw - 2 - 2 * i;
    c[10] = gl_canon(f[2]);
    c[11] = gl_canon(f[3]);
    c[12] = h.num_eval - 1;
    c[13] = 0;
    c[14] = r.count[w0 + 2 * i + 1];
    c[15] = r.count[w0 + 2 * i];
  } else {
    const u32 k = at.local - n_read;  // < num_eval: the row lies inside the evaluation
    const AceGate d = ace_decode(r.felts[h.payload + 2 * (size_t)h.num_vars + k], nw, h.num_vars, k);
    const e2 v0 = r.value[(size_t)gate0 + k];
    e2 vl{0, 0}, vr{0, 0};
    if (d.ok) {  // always: the host has refused anything else
      vl = ace_wire(r, h, gate0, d.pos_l);
      vr = ace_wire(r, h, gate0, d.pos_r);
    }
    c[0] = 0;
    c[1] = 1;
    c[3] = h.ptr + 2 * h.num_vars + k;
    c[5] = d.op == 0 ? GL_P - 1 : d.op == 1 ? 0 : 1;
    c[6] = h.num_eval - 1 - k;
    c[7] = v0.c0;
    c[8] = v0.c1;
    c[9] = nw - 1 - d.pos_l;
    c[10] = vl.c0;
    c[11] = vl.c1;
    c[12] = nw - 1 - d.pos_r;
    c[13] = vr.c0;
    c[14] = vr.c1;
    c[15] = r.count[w0 + h.num_vars + k];
  }
  sec_store_row(o, row, c);
}

// ---- host ----
namespace {
void ace_fill_info(mh_ace_section_info* info, u64 rows, u64 wires, u64 gates, u64 rounds, int log_n, int defect, u64 index, u64 gate) {
  if (!info) return;
  info->n_rows = rows;
  info->n_wires = wires;
  info->n_gates = gates;
  info->n_rounds = rounds;
  info->log_n = log_n;
  info->defect = defect;
  info->defect_index = index;
  info->defect_gate = gate;
}

[[noreturn]] void ace_refuse(mh_ace_section_info* info, int log_n, int defect, u64 index, u64 gate, const mh_ace_eval* evals, size_t n_evals,
                             const char* entry) {
  ace_fill_info(info, 0, 0, 0, 0, log_n, defect, index, gate);
  char buf[320];
  const unsigned long long i = index;
  const mh_ace_eval h = index < n_evals ? evals[index] : mh_ace_eval{0, 0, 0, 0, 0, 0, 0};
  switch (defect) {
    case 1:
      snprintf(buf, sizeof buf, "%s: defect 1, evaluation %llu has num_vars %u (even, not 0) and num_eval %u (a multiple of 4, not 0; at most 2^30 - 1 wires)",
               entry, i, h.num_vars, h.num_eval);
      break;
    case 2: snprintf(buf, sizeof buf, "%s: defect 2, evaluation %llu has clk %u, which is not above the previous evaluation's", entry, i, h.clk); break;
    case 3:
      snprintf(buf, sizeof buf, "%s: defect 3, the operands of evaluation %llu (ptr %u, num_vars %u, num_eval %u, payload %llu) leave the felts or the address space",
               entry, i, h.ptr, h.num_vars, h.num_eval, (unsigned long long)h.payload);
      break;
    case 4:
      snprintf(buf, sizeof buf, "%s: defect 4, gate %llu of evaluation %llu has an opcode above 2 or names a wire that is not inserted yet", entry,
               (unsigned long long)gate, i);
      break;
    case 5: snprintf(buf, sizeof buf, "%s: defect 5, the section does not fit: evaluation %llu is the first without its rows", entry, i); break;
    default: snprintf(buf, sizeof buf, "%s: defect 6, the circuit of evaluation %llu does not evaluate to zero", entry, i);
  }
  throw MhError(MH_ERR_INVALID, buf);
}

struct AceTarget {
  virtual ~AceTarget() {}
  virtual u64 cap_rows() const = 0;                    // rows the target has; ~0 when it is sized by the section
  virtual SecOut resolve(u64 n_rows, int* log_n) = 0;  // called once the section is known to fit
};

// what the headers say as they stand: rows, wires, gates (saturating far above the limits)
void ace_header_sums(const mh_ace_eval* evals, size_t n_evals, u64* rows, u64* wires, u64* gates) {
  *rows = *wires = *gates = 0;
  for (size_t i = 0; i < n_evals; i++) {
    *rows += (u64)evals[i].num_vars / 2 + evals[i].num_eval;
    *wires += (u64)evals[i].num_vars + evals[i].num_eval;
    *gates += evals[i].num_eval;
  }
}

// n_evals >= 1, at most 2^24 rows by the headers.  Returns after the second read-back with the rows kernel enqueued
void ace_run(mh_ctx* c, const mh_ace_eval* evals, size_t n_evals, const uint64_t* felts, size_t n_felts, AceTarget& target, int shown_log_n,
             mh_ace_section_info* info, const char* entry) {
  u64 h_rows, h_wires, h_gates;
  ace_header_sums(evals, n_evals, &h_rows, &h_wires, &h_gates);  // <= 2^24, 2^25, 2^24
  const u32 tiles = sec_grid(n_evals, HS_TILE);
  DevBuf devals(n_evals * sizeof(mh_ace_eval)), dfelts((n_felts ? n_felts : 1) * 8), words(sizeof(AceWords));
  DevBuf agg((size_t)tiles * 8), starts(3 * (n_evals + 1) * 4), count((h_wires ? h_wires : 1) * 4), value((h_gates ? h_gates : 1) * sizeof(e2));
  AceWords* dw = (AceWords*)words.p;
  const AceWords init{ACE_NONE, ACE_NONE, ACE_NONE, 0, 0, ACE_NONE, 0, 0};
  c->h2d(words.p, &init, sizeof init);
  c->h2d(devals.p, evals, n_evals * sizeof(mh_ace_eval));
  if (n_felts) c->h2d(dfelts.p, felts, n_felts * 8);
  u32* st = (u32*)starts.p;
  AceRun r{(const mh_ace_eval*)devals.p, (u32)n_evals, dfelts.u(), n_felts, target.cap_rows(), (u32*)agg.p, tiles, st, st + (n_evals + 1),
           st + 2 * (n_evals + 1), (u32*)count.p, (e2*)value.p, dw};
  {
    ProfScope ps(c, "ace_plan", 72.0 * (double)n_evals);
    MH_LAUNCH(k_ace_plan, dim3(tiles), dim3(HS_BT), 0, c->stream, r);
    MH_LAUNCH(k_hs_carries, dim3(1), dim3(64), 0, c->stream, (u32*)agg.p, tiles, &dw->n_rows, &dw->n_wires);
    MH_LAUNCH(k_ace_offsets, dim3(tiles), dim3(HS_BT), 0, c->stream, r);
  }
  if (h_gates) {
    ProfScope ps(c, "ace_gates", 16.0 * (double)h_gates);
    HIP_CHECK(hipMemsetAsync(count.p, 0, (h_wires ? h_wires : 1) * 4, c->stream));
    MH_LAUNCH(k_ace_gates, dim3(sec_grid(h_gates, ACE_BT)), dim3(ACE_BT), 0, c->stream, r, (u32)h_wires);
  }
  AceWords w;
  c->d2h(&w, words.p, sizeof w);  // the first wait: kinds 1..5 and the sizes, before anything but scratch is written
  const u64 n_rows = w.n_rows, n_wires = w.n_wires, n_gates = 2 * n_rows - n_wires;
  if (shown_log_n < 0) shown_log_n = sec_log_n(n_rows);
  const u64 bad_e = w.bad != ACE_NONE ? w.bad >> 3 : ACE_NONE, gate_e = w.bad_gate != ACE_NONE ? w.bad_gate >> 32 : ACE_NONE;
  if (bad_e != ACE_NONE && bad_e < gate_e) ace_refuse(info, shown_log_n, (int)(w.bad & 7), bad_e, 0, evals, n_evals, entry);
  if (gate_e != ACE_NONE) ace_refuse(info, shown_log_n, 4, gate_e, w.bad_gate & 0xFFFFFFFFull, evals, n_evals, entry);
  MH_REQUIRE(n_rows == h_rows && n_wires == h_wires, std::string(entry) + ": internal error, the device's sizes are not the headers'");
  if (w.nofit != ACE_NONE || n_rows > target.cap_rows()) ace_refuse(info, shown_log_n, 5, w.nofit != ACE_NONE ? w.nofit : n_evals, 0, evals, n_evals, entry);
  {
    ProfScope ps(c, "ace_eval", 24.0 * (double)n_gates);
    MH_LAUNCH(k_ace_eval, dim3((unsigned)n_evals), dim3(64), 0, c->stream, r);
  }
  AceWords w2;
  c->d2h(&w2, words.p, sizeof w2);  // the second wait: kind 6 and n_rounds, before any row is written
  if (w2.nonzero != ACE_NONE) ace_refuse(info, shown_log_n, 6, w2.nonzero, 0, evals, n_evals, entry);
  int log_n = shown_log_n;
  const SecOut o = target.resolve(n_rows, &log_n);
  {
    ProfScope ps(c, "ace_rows", (64.0 + 8.0 * ACE_WIDTH) * (double)n_rows);
    MH_LAUNCH(k_ace_rows, dim3(sec_grid(n_rows, ACE_BT)), dim3(ACE_BT), 0, c->stream, r, (u32)n_rows, o);
  }
  ace_fill_info(info, n_rows, n_wires, n_gates, w2.n_rounds, log_n, 0, 0, 0);
}

struct AceBuildTarget : AceTarget {
  mh_ctx* c;
  int log_n;  // -1: sized by the section
  std::unique_ptr<mh_trace> t;
  AceBuildTarget(mh_ctx* ctx, int l) : c(ctx), log_n(l) {}
  u64 cap_rows() const override { return log_n < 0 ? ~(u64)0 : (u64)1 << log_n; }
  SecOut resolve(u64 n_rows, int* out_log_n) override {
    const int l = log_n < 0 ? sec_log_n(n_rows) : log_n;
    t = sec_new_trace(c, l, ACE_WIDTH, n_rows);
    *out_log_n = l;
    return SecOut{t->cols.u(), (u64)1 << l, 0, 0, -1};
  }
};

struct AceChipletsTarget : AceTarget {
  mh_trace* chiplets;
  u64 start_row;
  AceChipletsTarget(mh_trace* t, u64 s) : chiplets(t), start_row(s) {}
  u64 cap_rows() const override { return ((u64)1 << chiplets->log_n) - start_row; }
  SecOut resolve(u64, int* out_log_n) override {
    *out_log_n = chiplets->log_n;
    return SecOut{chiplets->cols.u(), (u64)1 << chiplets->log_n, start_row, 4, 3};
  }
};

void ace_require_size(const mh_ace_eval* evals, size_t n_evals, const char* entry) {
  MH_REQUIRE(n_evals <= SEC_MAX_ROWS, std::string(entry) + ": more than 2^24 rows");
  u64 rows, wires, gates;
  ace_header_sums(evals, n_evals, &rows, &wires, &gates);  // n_evals <= 2^24 terms below 2^33
  MH_REQUIRE(rows <= SEC_MAX_ROWS, std::string(entry) + ": more than 2^24 rows");
}
}  // namespace

extern "C" uint32_t mh_ace_section_tile(void) { return HS_TILE; }

extern "C" int mh_ace_section_build(mh_ctx* c, const mh_ace_eval* evals, size_t n_evals, const uint64_t* felts, size_t n_felts, int log_n,
                                    mh_trace** out, mh_ace_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_ace_section_build";
    if (out) *out = nullptr;
    ace_fill_info(info, 0, 0, 0, 0, log_n, 0, 0, 0);
    MH_REQUIRE(out && (evals || !n_evals) && (felts || !n_felts), "mh_ace_section_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 6 && log_n <= 32), "mh_ace_section_build: log_n lies in 6..32, or is -1");
    ace_require_size(evals, n_evals, entry);
    HIP_CHECK(hipSetDevice(c->device));
    AceBuildTarget target(c, log_n);
    if (n_evals) {
      ace_run(c, evals, n_evals, felts, n_felts, target, log_n, info, entry);
    } else {
      int l = log_n;
      target.resolve(0, &l);
      ace_fill_info(info, 0, 0, 0, 0, l, 0, 0, 0);
    }
    *out = target.t.release();
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_miden_ace_section(mh_ctx* c, mh_trace* chiplets, uint64_t start_row, const mh_ace_eval* evals, size_t n_evals,
                                    const uint64_t* felts, size_t n_felts, mh_ace_section_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    const char* entry = "mh_miden_ace_section";
    ace_fill_info(info, 0, 0, 0, 0, 0, 0, 0, 0);
    MH_REQUIRE((evals || !n_evals) && (felts || !n_felts), "mh_miden_ace_section: null argument");
    sec_require_chiplets(c, chiplets, entry);
    ace_require_size(evals, n_evals, entry);
    const int log_n = chiplets->log_n;
    ace_fill_info(info, 0, 0, 0, 0, log_n, 0, 0, 0);
    if (start_row > ((u64)1 << log_n)) ace_refuse(info, log_n, 5, 0, 0, evals, n_evals, entry);
    if (!n_evals) return MH_OK;
    HIP_CHECK(hipSetDevice(c->device));
    trace_wait_ready(c, chiplets);
    AceChipletsTarget target(chiplets, start_row);
    ace_run(c, evals, n_evals, felts, n_felts, target, log_n, info, entry);
    return MH_OK;
  }
  SEC_CATCH
}
