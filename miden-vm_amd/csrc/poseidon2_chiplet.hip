// The precompile prover's Poseidon2 chiplet trace (Poseidon2Air, 32 columns) built on the device from the absorption ledger
// (mh_poseidon2_chiplet_trace_build), gfx950.
//
// Replaces Poseidon2Requires' generate_trace / write_cycle (transcript/poseidon2/trace.rs:217-420).  The planner
// (poseidon2_chiplet_plan.cpp, host only, no hashing) has validated the ledger and given every absorption its start cycle and level.
//   chains   level by level, the absorptions of a level side by side, longest first.  An absorption walks its blocks: the rate words
//            come from `blocks` or, for a referenced half, from the digest table (written by a lower level); the permutation; the
//            capacity carries over.  Per cycle it leaves one 128-byte record in scratch: the input state (12 felts), in_mult, out_mult,
//            is_absorb, a zero.  At its end it writes its digest into the table.  Two forms:
//              group  16 lanes a chain, a state element a lane (p2l_permute, poseidon2_lanes.cuh): the short dependent chain.  256
//                     lanes = 16 chains a block.  A run of consecutive levels none wider than one block is ONE launch of one block that
//                     loops over the levels with __syncthreads() between: the digests of a level are read by the same block.
//              lane   a lane a chain (p2f_permute): a level wider than 8192 chains (MH_P2C_GROUP_MAX_CHAINS: experiments), where lanes are many.
//            A level's digests reach the next level by the launch boundary or by that block barrier; no kernel waits on a value of
//            another block.  The next block's rate words are fetched before the permutation of the current one.
//   cycles   a lane per cycle reads its record and reruns the permutation with the canonical round functions of poseidon2.cuh,
//            every row boundary as write_cycle writes it.  32 cycles a block go through an LDS tile [columns][32][16 + 1] so that each
//            column leaves as 512 consecutive felts (whole 128-byte lines), as k_p2t_cycles does (p2_trace.hip).  The 28 computed
//            columns do not fit one tile (121 KB): two passes, each a launch that runs the permutation -- pass 0 the state and the
//            witnesses (15 columns, 65 280 B) plus perm_seq_id, the multiplicities and is_absorb; pass 1 the 13 cube registers
//            (56 576 B).  A padding cycle is zeros and its perm_seq_id: no permutation, the tile is not read.
// Every cell of the trace and of the scratch has exactly one writer; no memset, no atomics: a second call leaves the same bytes.
#include "section_out.cuh"
#include "poseidon2_lanes.cuh"
#include <algorithm>
#include <cstdlib>
#include <vector>

static_assert(sizeof(mh_p2c_absorption) == 56, "mh_p2c_absorption is 56 bytes");
static_assert(sizeof(mh_p2c_info) == 48, "mh_p2c_info is 48 bytes");

namespace {
constexpr int P2C_WIDTH = 32, P2C_CYCLE = 16;
constexpr int P2C_COL_IN_MULT = 1, P2C_COL_STATE = 4, P2C_COL_CUBE = 19;
constexpr int P2C_REC = 16;           // felts of a cycle's scratch record: state 0..11, in_mult 12, out_mult 13, is_absorb 14, zero 15
constexpr int P2C_GROUP_BT = 256;     // group form: 16 chains a block
constexpr int P2C_GROUP_CHAINS = P2C_GROUP_BT / 16;
constexpr int P2C_LANE_BT = 64;

struct P2cChains {
  const mh_p2c_absorption* abs;
  const u64* start;          // [n_abs]
  const u32* order;          // absorptions by (level, n_blocks descending)
  const u32* level_off;      // [n_levels + 1] into order
  const u64* blocks;         // [n_cycles][8]
  const long long* refs;     // [n_cycles][2] or null
  u64* rec;                  // [n_cycles][P2C_REC]
  u64* digest;               // [n_abs][4]
  u64* outputs;              // [n_cycles][12] or null
};

// rate word g (0..7) of cycle c: the literal, or word g & 3 of a lower level's digest
__device__ __forceinline__ u64 p2c_rate_word(const P2cChains& a, u64 c, int g) {
  const long long r = a.refs ? a.refs[2 * c + (g >> 2)] : -1;
  return r < 0 ? gl_canon(a.blocks[c * 8 + g]) : a.digest[(size_t)r * 4 + (g & 3)];
}
}  // namespace

// ---- chains, group form: levels l0 .. l1 - 1; more than one level only with a grid of one block ----
__global__ __launch_bounds__(P2C_GROUP_BT) void k_p2c_chains_group(P2cChains a, u32 l0, u32 l1) {
  const int g = threadIdx.x & 15;
  for (u32 l = l0; l < l1; l++) {
    const u32 base = a.level_off[l], width = a.level_off[l + 1] - base;
    const u32 k = blockIdx.x * P2C_GROUP_CHAINS + (threadIdx.x >> 4);
    const bool has = k < width;
    const u32 ai = has ? a.order[base + k] : 0;
    u32 nb = 0;
    u64 st = 0, s = 0, meta = 0;
    if (has) {
      const mh_p2c_absorption& ab = a.abs[ai];
      nb = (u32)ab.n_blocks;  // <= 2^20
      st = a.start[ai];
      if (g >= 8 && g < 12) s = gl_canon(ab.cap[g - 8]);
      if (g == 12) meta = gl_canon(ab.in_mult);
      if (g == 13) meta = gl_canon(ab.out_mult);
    }
    u64 nextv = (g < 8 && nb) ? p2c_rate_word(a, st, g) : 0;
    for (u32 b = 0; __any(b < nb); b++) {  // wave-uniform: the four chains of a wave step together, a finished one idles
      const bool act = b < nb;
      const u64 c = st + b;
      if (act) {
        if (g < 8) s = nextv;
        a.rec[c * P2C_REC + g] = g < 12 ? s : (g == 14 ? (u64)(b > 0) : meta);
      }
      if (g < 8 && b + 1 < nb) nextv = p2c_rate_word(a, c + 1, g);  // under the permutation, not behind it
      const u64 t = p2l_permute(g < 12 ? s : 0);
      if (act && g < 12) {
        s = t;
        if (a.outputs) a.outputs[c * 12 + g] = t;
      }
    }
    if (has && g < 4) a.digest[(size_t)ai * 4 + g] = s;
    if (l + 1 < l1) __syncthreads();  // one block: its digests of level l are visible to its reads of level l + 1
  }
}

// ---- chains, lane form: one level ----
__global__ __launch_bounds__(P2C_LANE_BT) void k_p2c_chains_lane(P2cChains a, u32 l) {
  const u32 base = a.level_off[l], width = a.level_off[l + 1] - base;
  const u32 k = blockIdx.x * P2C_LANE_BT + threadIdx.x;
  if (k >= width) return;
  const u32 ai = a.order[base + k];
  const mh_p2c_absorption ab = a.abs[ai];
  const u64 st = a.start[ai], im = gl_canon(ab.in_mult), om = gl_canon(ab.out_mult);
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 4; i++) s[8 + i] = gl_canon(ab.cap[i]);
  for (u32 b = 0; b < (u32)ab.n_blocks; b++) {
    const u64 c = st + b;
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = p2c_rate_word(a, c, i);
    u64* rec = a.rec + c * P2C_REC;
#pragma unroll
    for (int i = 0; i < 12; i++) rec[i] = s[i];
    rec[12] = im;
    rec[13] = om;
    rec[14] = b > 0;
    rec[15] = 0;
    p2f_permute(s);
    if (a.outputs) {
#pragma unroll
      for (int i = 0; i < 12; i++) a.outputs[c * 12 + i] = s[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) a.digest[(size_t)ai * 4 + i] = s[i];
}

namespace {
// ---- cycles: the store layout of p2_trace.hip, a tile [COLS][32 cycles][16 rows + 1] ----
constexpr int P2C_TILE_CYCLES = 32;
constexpr int P2C_TILE_STRIDE = P2C_CYCLE + 1;
constexpr int P2C_TILE_COL = P2C_TILE_CYCLES * P2C_TILE_STRIDE;
template <int PASS>
struct P2cPass {
  static constexpr int COLS = PASS == 0 ? 15 : 13;             // state 12 + witnesses 3 | cube registers 13
  static constexpr int COL0 = PASS == 0 ? P2C_COL_STATE : P2C_COL_CUBE;
};

struct P2cSink {
  u64* tile;  // + lane * P2C_TILE_STRIDE
  __device__ __forceinline__ void put(int col, int r, u64 v) { tile[(size_t)col * P2C_TILE_COL + r] = v; }
};

// x^7 as p2_sbox computes it, and x^3 on the way
__device__ __forceinline__ u64 p2c_sbox(u64 x, u64& cube) {
  const u64 x2 = gl_sqr(x);
  cube = gl_mul(x2, x);
  return gl_mul(cube, gl_sqr(x2));
}

// row r: the state (pass 0, with the witnesses) -- the cube registers follow from the round that leaves the row
template <int PASS>
__device__ __forceinline__ void p2c_state_row(P2cSink& sink, int r, const u64 s[12], u64 w0, u64 w1, u64 w2) {
  if constexpr (PASS == 0) {
#pragma unroll
    for (int i = 0; i < 12; i++) sink.put(i, r, s[i]);
    sink.put(12, r, w0);
    sink.put(13, r, w1);
    sink.put(14, r, w2);
  }
}

// an external round whose 12 cubes stand on row r: registers 0..11, register 12 := c12
template <int PASS>
__device__ __forceinline__ void p2c_ext_round(P2cSink& sink, int r, u64 s[12], const unsigned long long* rc, u64 c12) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    u64 cube;
    s[i] = p2c_sbox(gl_add(s[i], rc[i]), cube);
    if constexpr (PASS == 1) sink.put(i, r, cube);
  }
  if constexpr (PASS == 1) sink.put(12, r, c12);
  p2_external_linear(s);
}

__device__ __forceinline__ u64 p2c_int_round(u64 s[12], int r, u64& cube) {
  const u64 w = p2c_sbox(gl_add(s[0], p2c::P2_ARK_INT[r]), cube);
  s[0] = w;
  p2_internal_linear(s);
  return w;
}

// write_cycle (trace.rs:300-420) = testing/precompile_trace.poseidon2_chiplet_trace; the row schedule of p2t_cycle plus the cubes
template <int PASS>
__device__ __forceinline__ void p2c_cycle(u64 s[12], P2cSink& sink) {
  p2c_state_row<PASS>(sink, 0, s, 0, 0, 0);
  p2_external_linear(s);
  p2c_ext_round<PASS>(sink, 0, s, p2c::P2_ARK_EXT_INITIAL, 0);
#pragma unroll
  for (int r = 1; r < 4; r++) {
    p2c_state_row<PASS>(sink, r, s, 0, 0, 0);
    p2c_ext_round<PASS>(sink, r, s, p2c::P2_ARK_EXT_INITIAL + 12 * r, 0);
  }
#pragma unroll 1
  for (int t = 0; t < 7; t++) {
    if constexpr (PASS == 0) {
#pragma unroll
      for (int i = 0; i < 12; i++) sink.put(i, 4 + t, s[i]);
    }
    u64 c0, c1, c2;
    const u64 w0 = p2c_int_round(s, 3 * t, c0), w1 = p2c_int_round(s, 3 * t + 1, c1), w2 = p2c_int_round(s, 3 * t + 2, c2);
    if constexpr (PASS == 0) {
      sink.put(12, 4 + t, w0);
      sink.put(13, 4 + t, w1);
      sink.put(14, 4 + t, w2);
    } else {
      sink.put(0, 4 + t, c0);
      sink.put(1, 4 + t, c1);
      sink.put(2, 4 + t, c2);
#pragma unroll
      for (int i = 3; i < 13; i++) sink.put(i, 4 + t, 0);
    }
  }
  if constexpr (PASS == 0) {
#pragma unroll
    for (int i = 0; i < 12; i++) sink.put(i, 11, s[i]);
  }
  u64 c12;
  const u64 w = p2c_int_round(s, 21, c12);
  if constexpr (PASS == 0) {
    sink.put(12, 11, w);
    sink.put(13, 11, 0);
    sink.put(14, 11, 0);
  }
  p2c_ext_round<PASS>(sink, 11, s, p2c::P2_ARK_EXT_TERMINAL, c12);
#pragma unroll
  for (int r = 1; r < 4; r++) {
    p2c_state_row<PASS>(sink, 11 + r, s, 0, 0, 0);
    p2c_ext_round<PASS>(sink, 11 + r, s, p2c::P2_ARK_EXT_TERMINAL + 12 * r, 0);
  }
  p2c_state_row<PASS>(sink, 15, s, 0, 0, 0);
  if constexpr (PASS == 1) {
#pragma unroll
    for (int i = 0; i < 13; i++) sink.put(i, 15, 0);
  }
}
}  // namespace

template <int PASS>
__global__ __launch_bounds__(P2C_TILE_CYCLES) void k_p2c_cycles(const u64* __restrict__ rec, u64 n_cycles, u64 cycles, u64 n, u64* __restrict__ out) {
  constexpr int COLS = P2cPass<PASS>::COLS, COL0 = P2cPass<PASS>::COL0;
  __shared__ u64 tile[COLS * P2C_TILE_COL];
  const u64 c0 = (u64)blockIdx.x * P2C_TILE_CYCLES, c = c0 + threadIdx.x;
  if (c < n_cycles) {
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = rec[c * P2C_REC + i];
    P2cSink sink{tile + threadIdx.x * P2C_TILE_STRIDE};
    p2c_cycle<PASS>(s, sink);
  }
  __syncthreads();
  const u64 live = (cycles - c0 < P2C_TILE_CYCLES ? cycles - c0 : P2C_TILE_CYCLES) * P2C_CYCLE;  // rows of this block
  u64* o = out + c0 * P2C_CYCLE;
  for (u32 e = threadIdx.x; e < live; e += P2C_TILE_CYCLES) {
    const u64 ce = c0 + e / P2C_CYCLE;
    const bool real = ce < n_cycles;  // a padding cycle never wrote the tile
    const u32 at = (e / P2C_CYCLE) * P2C_TILE_STRIDE + e % P2C_CYCLE;
#pragma unroll
    for (int col = 0; col < COLS; col++) o[(size_t)(COL0 + col) * n + e] = real ? tile[col * P2C_TILE_COL + at] : 0;
    if constexpr (PASS == 0) {
      o[e] = ce;
#pragma unroll
      for (int i = 0; i < 3; i++) o[(size_t)(P2C_COL_IN_MULT + i) * n + e] = real ? rec[ce * P2C_REC + 12 + i] : 0;
    }
  }
}

namespace {
size_t p2c_group_max_chains() {
  static const size_t v = [] {
    const char* e = getenv("MH_P2C_GROUP_MAX_CHAINS");  // experiments: the widest level the group form takes (0: the lane form always)
    return e ? (size_t)atol(e) : (size_t)8192;
  }();
  return v;
}

[[noreturn]] void p2c_refuse(mh_p2c_info* info, int kind, u64 index) {
  static const char* what[] = {"", "a null pointer where one is required", "an absorption with n_blocks = 0 (index: the absorption)",
                               "the n_blocks do not add up to n_cycles (index: the first absorption that runs past, n_abs when the list ends short)",
                               "a reference that is neither -1 nor an earlier absorption (index: 2 cycle + half)", "more than 2^20 cycles (2^24 rows)",
                               "the trace does not fit log_n (index: rows needed)"};
  info->defect_kind = kind;
  info->defect_index = index;
  char buf[320];
  snprintf(buf, sizeof buf, "mh_poseidon2_chiplet_trace_build: defect %d, index %llu: %s", kind, (unsigned long long)index, what[kind]);
  throw MhError(MH_ERR_INVALID, buf);
}
}  // namespace

extern "C" int mh_poseidon2_chiplet_trace_build(mh_ctx* c, const mh_p2c_absorption* abs, size_t n_abs, const uint64_t* blocks, const int64_t* refs,
                                                size_t n_cycles, int log_n, mh_trace** out, uint64_t* digests, uint64_t* outputs, mh_p2c_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_p2c_info local;
  if (!info) info = &local;
  try {
    *info = mh_p2c_info{};
    info->n_absorptions = n_abs;
    info->n_cycles = n_cycles;
    if (!out || (!abs && n_abs) || (!blocks && n_cycles)) p2c_refuse(info, 1, 0);
    MH_REQUIRE(log_n == -1 || (log_n >= 0 && log_n <= 24), "mh_poseidon2_chiplet_trace_build: log_n lies in 0..24, or is -1");
    std::vector<u64> start(n_abs);
    std::vector<u32> level(n_abs);
    if (mh_poseidon2_chiplet_plan(abs, n_abs, refs, n_cycles, start.data(), level.data(), info) != MH_OK) p2c_refuse(info, info->defect_kind, info->defect_index);
    if (log_n < 0) log_n = info->log_n;
    if (((u64)1 << log_n) < info->rows_needed) p2c_refuse(info, 6, info->rows_needed);
    info->log_n = log_n;
    const u64 height = (u64)1 << log_n, cycles = height / P2C_CYCLE;
    const u32 n_levels = (u32)info->n_levels;
    // the absorptions by level, longest first inside a level (the longest chain bounds the launch: it starts first)
    std::vector<u32> level_off(n_levels + 1, 0), order(n_abs);
    for (size_t i = 0; i < n_abs; i++) level_off[level[i] + 1]++;
    for (u32 l = 0; l < n_levels; l++) level_off[l + 1] += level_off[l];
    {
      std::vector<u32> at(level_off.begin(), level_off.end() - 1);
      for (size_t i = 0; i < n_abs; i++) order[at[level[i]]++] = (u32)i;
    }
    for (u32 l = 0; l < n_levels; l++) {
      u32* lo = order.data() + level_off[l];
      u32* hi = order.data() + level_off[l + 1];
      bool equal = true;
      for (u32* p = lo; p < hi && equal; p++) equal = abs[*p].n_blocks == abs[*lo].n_blocks;
      if (!equal) std::stable_sort(lo, hi, [&](u32 x, u32 y) { return abs[x].n_blocks > abs[y].n_blocks; });
    }
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf dabs(n_abs * sizeof(mh_p2c_absorption)), dstart(n_abs * 8), dorder(n_abs * 4), dlevel_off((size_t)(n_levels + 1) * 4), dblocks(n_cycles * 64),
        drefs(refs ? n_cycles * 16 : 0), rec(n_cycles * P2C_REC * 8), ddig(n_abs * 32), dout(outputs ? n_cycles * 96 : 0);
    std::unique_ptr<mh_trace> t = trace_new(c, log_n, P2C_WIDTH);
    if (n_abs) {
      c->h2d(dabs.p, abs, n_abs * sizeof(mh_p2c_absorption));
      c->h2d(dstart.p, start.data(), n_abs * 8);
      c->h2d(dorder.p, order.data(), n_abs * 4);
      c->h2d(dlevel_off.p, level_off.data(), (size_t)(n_levels + 1) * 4);
      c->h2d(dblocks.p, blocks, n_cycles * 64);
      if (refs) c->h2d(drefs.p, refs, n_cycles * 16);
      const P2cChains a{(const mh_p2c_absorption*)dabs.p, dstart.u(), (const u32*)dorder.p, (const u32*)dlevel_off.p, dblocks.u(),
                        refs ? (const long long*)drefs.p : nullptr, rec.u(), ddig.u(), outputs ? dout.u() : nullptr};
      ProfScope ps(c, "p2c_chains", (double)n_cycles * (64.0 + 8.0 * P2C_REC) + 88.0 * (double)n_abs);
      const size_t group_max = p2c_group_max_chains();
      for (u32 l = 0; l < n_levels;) {
        const u32 width = level_off[l + 1] - level_off[l];
        if (width > group_max) {
          MH_LAUNCH(k_p2c_chains_lane, dim3(sec_grid(width, P2C_LANE_BT)), dim3(P2C_LANE_BT), 0, c->stream, a, l);
          l++;
          continue;
        }
        u32 l1 = l + 1;  // a run of levels each within one block is one launch of one block
        if (width <= (u32)P2C_GROUP_CHAINS)
          while (l1 < n_levels && level_off[l1 + 1] - level_off[l1] <= (u32)P2C_GROUP_CHAINS) l1++;
        MH_LAUNCH(k_p2c_chains_group, dim3(sec_grid(width, P2C_GROUP_CHAINS)), dim3(P2C_GROUP_BT), 0, c->stream, a, l, l1);
        l = l1;
      }
    }
    {
      ProfScope ps(c, "p2c_cycles", 8.0 * P2C_WIDTH * (double)height + 2.0 * 8.0 * P2C_REC * (double)n_cycles);
      const unsigned grid = sec_grid(cycles, P2C_TILE_CYCLES);
      MH_LAUNCH(k_p2c_cycles<0>, dim3(grid), dim3(P2C_TILE_CYCLES), 0, c->stream, (const u64*)rec.u(), (u64)n_cycles, cycles, height, t->cols.u());
      MH_LAUNCH(k_p2c_cycles<1>, dim3(grid), dim3(P2C_TILE_CYCLES), 0, c->stream, (const u64*)rec.u(), (u64)n_cycles, cycles, height, t->cols.u());
    }
    if (digests && n_abs) c->d2h(digests, ddig.p, n_abs * 32);
    if (outputs && n_cycles) c->d2h(outputs, dout.p, n_cycles * 96);
    *out = t.release();
    return MH_OK;
  }
  SEC_CATCH
}
