// The precompile prover's Keccak round and sponge traces built on the device from messages (mh_keccak_traces_build) or from
// permutation inputs (mh_keccak_round_trace_build), gfx950.
//
// Replaces KeccakRoundAir's generate_trace_from_states_inner (hash/keccak/round/mod.rs:725-806) and the sponge's SpongeRequires /
// generate_trace (hash/keccak/sponge/trace.rs:176-262, 388-585).  The 128-slot round programme (round/program.rs `slots()`) and the
// 24 round constants are built here (kt_slots); the caller passes neither.
//   offsets          block_off[m] = blocks of the messages before m (len / 136 + 1 each): the tile scan of hs_scan.cuh, k_hs_carries
//                    between its two passes.
//   absorb_permute   a wave per message (or per state).  The wave holds the machine's address space of ONE permutation in LDS (3225
//                    words: the input at 0..24, RC[r] at 25 + 128 r, the value of programme row r at 25 + r; the dead round writes
//                    nothing and stays zero) and walks the message's blocks: absorb 17 lanes (pad10*1, 0x01 / 0x80), run the 24 rounds
//                    level by level -- a level's slots read only lower levels, other rounds, RC or the input, so they run a lane a
//                    slot: 10 dependent steps a round (widths 5 5 5 5 5 5 25 25 25 1) -- and copy the image out, 64 words a store.
//                    Per block it leaves what the sponge rows need: at_start[25], post_xorin[16], perm_out[25].
//   round_rows       a lane per (row, permutation lane): operands through the slot's back-offsets out of the image, the 34-column band
//                    (ip, 8 + 8 + 8 bytes, 8 limbs of (half + 2^32) 2^(shift mod 32), active), column-major, consecutive lanes on
//                    consecutive rows.  Every cell of the trace is written, pad rows and the odd count's idle lane included.
//   sponge_rows      a lane per row: the row's message by a wave-uniform binary search of block_off (a wave spans two blocks: one
//                    step on), the 67 cells in closed form from the message bytes and the per-block words; the padding rows too.
// Every cell has one writer and no kernel uses atomics.  The byte-pair table's multiplicities are not counted here
// (mh_fill_multiplicities_precompile_traces does that).
#include "section_out.cuh"
#include "hs_scan.cuh"
#include <cstring>

static_assert(sizeof(mh_keccak_msg) == 24, "mh_keccak_msg is 24 bytes");
static_assert(sizeof(mh_keccak_traces_info) == 48, "mh_keccak_traces_info is 48 bytes");

namespace {
constexpr int KT_PERIOD = 128, KT_ROUNDS = 24, KT_CYCLE = 25 * 128, KT_IP0 = 25, KT_WORDS = KT_IP0 + KT_CYCLE;
constexpr int KT_BAND = 34, KT_ROUND_WIDTH = 68, KT_SPONGE_WIDTH = 67, KT_LEVELS = 10, KT_LEVEL_STRIDE = 32;
constexpr int KT_RATE_LANES = 17, KT_RATE_BYTES = 136, KT_SPONGE_PERIOD = 32;
constexpr int KT_OUT0 = KT_IP0 + 23 * KT_PERIOD + 103;  // the 25 outputs of round 23: the iota slot, then the chi-XOR block
constexpr u64 KT_PAD_CONST = 0x8000000000000000ull;
constexpr u64 KT_P = 0xFFFFFFFF00000001ull;
constexpr u32 KT_IDLE = 0xFFFFFFFFu;
constexpr int KT_BT = 256;
enum { KT_NOP = 0, KT_XOR = 1, KT_ANDNOT = 2, KT_ROL = 3, KT_XORROL = 4 };

const u64 KT_RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                       0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                       0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                       0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                       0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

struct KtSlot {
  int op, shift, back_a, back_b, mult;
};

// `slots()` (round/program.rs:262-270).  A source is a slot of the same round (>= 0), lane (x, y) of the previous round's output
// (-1 - (x + 5 y)), or none (KT_NONE); `Source::back_off` turns it into a back-offset
constexpr int KT_NONE = -1000;
void kt_slots(KtSlot (&out)[KT_PERIOD]) {
  static const int RHO[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};  // [x][y]
  static const int SLOT_B[25] = {32, 34, 36, 37, 38, 39, 40, 41, 43, 46, 47, 48, 49, 50, 51, 52, 54, 55, 56, 58, 61, 63, 65, 67, 68};
  const int C0 = 2, DROL = 22, DXOR = 27, T0 = 69, CHI00 = 102, IOTA = 103, CHIX = 104, RC = 0;
  struct Raw {
    int op, shift, a, b, mult;
  } s[KT_PERIOD];
  for (auto& r : s) r = Raw{KT_NOP, 0, KT_NONE, KT_NONE, 0};
  auto lane = [](int x, int y) { return -1 - (x + 5 * y); };
  for (int x = 0; x < 5; x++) {  // theta C: five 4-XOR chains
    const int base = C0 + 4 * x;
    s[base] = Raw{KT_XOR, 0, lane(x, 0), lane(x, 1), 1};
    s[base + 1] = Raw{KT_XOR, 0, base, lane(x, 2), 1};
    s[base + 2] = Raw{KT_XOR, 0, base + 1, lane(x, 3), 1};
    s[base + 3] = Raw{KT_XOR, 0, base + 2, lane(x, 4), 2};
  }
  auto slot_c = [&](int x) { return C0 + 4 * x + 3; };
  for (int i = 0; i < 5; i++) s[DROL + i] = Raw{KT_ROL, 1, slot_c((i + 1) % 5), KT_NONE, 1};
  for (int i = 0; i < 5; i++) s[DXOR + i] = Raw{KT_XOR, 0, slot_c((i + 4) % 5), DROL + i, 5};
  for (int oy = 0; oy < 5; oy++)  // theta-apply + rho-pi
    for (int ox = 0; ox < 5; ox++) {
      const int ix = (3 * oy + ox) % 5, iy = ox, rho = RHO[ix][iy];
      const int a_src = lane(ix, iy), d_src = DXOR + ix;
      s[SLOT_B[ox + 5 * oy]] = Raw{rho ? KT_XORROL : KT_XOR, rho, iy == 0 ? d_src : a_src, iy == 0 ? a_src : d_src, 3};
    }
  for (int y = 0; y < 5; y++)
    for (int x = 0; x < 5; x++) s[T0 + x + 5 * y] = Raw{KT_ANDNOT, 0, SLOT_B[(x + 1) % 5 + 5 * y], SLOT_B[(x + 2) % 5 + 5 * y], 1};
  s[CHI00] = Raw{KT_XOR, 0, T0, SLOT_B[0], 1};
  s[IOTA] = Raw{KT_XOR, 0, CHI00, RC, 2};
  for (int idx = 1; idx < 25; idx++) s[CHIX + idx - 1] = Raw{KT_XOR, 0, T0 + idx, SLOT_B[idx], 2};
  auto back = [&](int src, int at) {
    if (src == KT_NONE) return 0;
    if (src >= 0) return at - src;
    const int l = -1 - src;
    return KT_PERIOD + at - (l == 0 ? IOTA : CHIX + l - 1);
  };
  for (int i = 0; i < KT_PERIOD; i++) out[i] = KtSlot{s[i].op, s[i].shift, back(s[i].a, i), back(s[i].b, i), s[i].mult};
}

inline bool kt_reads_b(int op) { return op == KT_XOR || op == KT_ANDNOT || op == KT_XORROL; }

// level 0: reads only the previous round's outputs, RC or the input; else one above the highest same-round slot read.  -1: NOP
void kt_levels(const KtSlot (&s)[KT_PERIOD], int (&level)[KT_PERIOD]) {
  for (int i = 0; i < KT_PERIOD; i++) {
    level[i] = -1;
    if (s[i].op == KT_NOP) continue;
    int l = 0;
    const int backs[2] = {s[i].back_a, kt_reads_b(s[i].op) ? s[i].back_b : 0};
    for (int b : backs)
      if (b > 0 && b <= i && level[i - b] + 1 > l) l = level[i - b] + 1;  // a NOP slot read (RC) is a constant: level -1 + 1
    level[i] = l;
  }
}

inline u32 kt_pack(int slot, const KtSlot& s) {
  return (u32)slot | (u32)s.op << 7 | (u32)s.shift << 10 | (u32)s.back_a << 16 | (u32)s.back_b << 24;
}

// what the kernels read: the schedule (level, lane) -> packed slot, KT_IDLE beyond the level's width; the programme by slot; RC
struct KtTab {
  u32 sched[KT_LEVELS][KT_LEVEL_STRIDE];
  u32 prog[KT_PERIOD];
  u64 rc[KT_ROUNDS];
};

void kt_table(KtTab& t) {
  KtSlot s[KT_PERIOD];
  int level[KT_PERIOD], width[KT_LEVELS] = {};
  kt_slots(s);
  kt_levels(s, level);
  memset(t.sched, 0xFF, sizeof t.sched);
  for (int i = 0; i < KT_PERIOD; i++) {
    MH_REQUIRE(s[i].back_a >= 0 && s[i].back_a < 256 && s[i].back_b >= 0 && s[i].back_b < 256 && s[i].shift < 64 && level[i] < KT_LEVELS,
               "keccak_traces: internal error, the round programme does not pack");
    t.prog[i] = kt_pack(i, s[i]);
    if (level[i] < 0) continue;
    MH_REQUIRE(width[level[i]] < KT_LEVEL_STRIDE, "keccak_traces: internal error, a level wider than 32 slots");
    t.sched[level[i]][width[level[i]]++] = t.prog[i];
  }
  memcpy(t.rc, KT_RC, sizeof t.rc);
}

struct KtRun {
  const KtTab* tab;
  const uint8_t* bytes;        // messages form
  const mh_keccak_msg* msgs;   // null: the stand-alone form, a wave per state
  const u32* block_off;        // [n_msgs + 1]
  const u64* states;           // stand-alone form: [n][25]
  u64* image;                  // [n_perms][KT_WORDS]
  u64* at_start;               // [n_perms][25]    messages form
  u64* post16;                 // [n_perms]        messages form
  u64* perm_out;               // [n_perms][25]    or null
  u64* digests;                // [n_msgs][4]      or null
};

struct KtSponge {
  const uint8_t* bytes;
  const mh_keccak_msg* msgs;
  const u32* block_off;
  u32 n_msgs, n_blocks;
  const u64 *at_start, *post16, *perm_out;
  long long pad_bytes_left;  // bytes_left and chunk_ptr as the last invocation leaves them
  u64 pad_chunk_ptr;
  u64* base;
  u64 height;
};

__device__ __forceinline__ u64 kt_rol(u64 x, u32 s) { return s ? (x << s) | (x >> (64 - s)) : x; }

// tape lane `pos` of a message: bytes [8 pos, 8 pos + 8) little-endian, zeros from `len` on
__device__ __forceinline__ u64 kt_tape(const uint8_t* __restrict__ bytes, u64 offset, u64 len, u64 pos) {
  u64 v = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u64 at = 8 * pos + i;
    if (at < len) v |= (u64)bytes[offset + at] << (8 * i);
  }
  return v;
}

// `value` as a lane half pair at column `half_at` and, when bytes_at >= 0, as eight bytes from column `bytes_at`
template <int HALF_AT, int BYTES_AT>
__device__ __forceinline__ void kt_put(u64* __restrict__ cell, u64 height, u64 value) {
  cell[(size_t)HALF_AT * height] = value & 0xffffffffull;
  cell[(size_t)(HALF_AT + 1) * height] = value >> 32;
  if (BYTES_AT >= 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) cell[(size_t)(BYTES_AT + i) * height] = (value >> (8 * i)) & 0xff;
  }
}
}  // namespace

// ---- offsets ----
__global__ __launch_bounds__(HS_BT) void k_kt_block_sums(const mh_keccak_msg* __restrict__ msgs, u32 n_msgs, u32* __restrict__ agg, u32 tiles) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 a[HS_PER_LANE], z[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    a[j] = i < n_msgs ? (u32)(msgs[i].len / KT_RATE_BYTES) + 1 : 0;
    z[j] = 0;
  }
  hs_tile_scan(a, z, 0, 0, ea, eb, ta, tb, s_wave);
  if (threadIdx.x == 0) {
    agg[blockIdx.x] = ta;
    agg[tiles + blockIdx.x] = 0;
  }
}

__global__ __launch_bounds__(HS_BT) void k_kt_offsets(const mh_keccak_msg* __restrict__ msgs, u32 n_msgs, const u32* __restrict__ agg,
                                                      u32* __restrict__ block_off) {
  __shared__ u32 s_wave[HS_WAVES][2];
  u32 a[HS_PER_LANE], z[HS_PER_LANE], ea[HS_PER_LANE], eb[HS_PER_LANE], ta, tb;
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    a[j] = i < n_msgs ? (u32)(msgs[i].len / KT_RATE_BYTES) + 1 : 0;
    z[j] = 0;
  }
  hs_tile_scan(a, z, agg[blockIdx.x], 0, ea, eb, ta, tb, s_wave);
#pragma unroll
  for (int j = 0; j < HS_PER_LANE; j++) {
    const u32 i = blockIdx.x * HS_TILE + threadIdx.x * HS_PER_LANE + j;
    if (i < n_msgs) block_off[i] = ea[j];
    if (i + 1 == n_msgs) block_off[n_msgs] = ea[j] + a[j];
  }
}

// ---- absorb_permute ----
__global__ __launch_bounds__(64) void k_kt_absorb_permute(KtRun r) {
  __shared__ u64 mem[KT_WORDS];
  const u32 lane = threadIdx.x, m = blockIdx.x;
  for (int i = lane; i < KT_WORDS; i += 64) mem[i] = 0;
  __syncthreads();
  if (lane < KT_ROUNDS) mem[KT_IP0 + KT_PERIOD * lane] = r.tab->rc[lane];  // no slot writes them: set once
  u32 e[KT_LEVELS];
#pragma unroll
  for (int l = 0; l < KT_LEVELS; l++) e[l] = lane < KT_LEVEL_STRIDE ? r.tab->sched[l][lane] : KT_IDLE;
  u64 offset = 0, len = 0;
  u32 g0 = m, n_blocks = 1;
  if (r.msgs) {
    offset = r.msgs[m].offset;
    len = r.msgs[m].len;
    g0 = r.block_off[m];
    n_blocks = r.block_off[m + 1] - g0;
  }
  const u64 last_bytes = len - (u64)KT_RATE_BYTES * (n_blocks - 1);  // 0 .. 135
  const u32 pad_lane = (u32)last_bytes >> 3, pad_byte = (u32)last_bytes & 7;
  u64 out = 0;
  for (u32 b = 0; b < n_blocks; b++) {
    const size_t g = (size_t)g0 + b;
    if (r.msgs) {
      const bool is_last = b + 1 == n_blocks;
      if (lane < 25) {
        const u64 at = mem[lane];
        r.at_start[g * 25 + lane] = at;
        if (lane < KT_RATE_LANES) {
          const u64 v = kt_tape(r.bytes, offset, len, (u64)KT_RATE_LANES * b + lane);
          u64 nv = at;
          if (!is_last || lane < pad_lane) {
            nv ^= v;
          } else if (lane == pad_lane) {
            const u64 cleared = ~(~0ull << (8 * pad_byte)) & v;  // ANDNOT(andnot_mask, lane)
            nv ^= cleared ^ (1ull << (8 * pad_byte));            // XOR(cleared, padding_mask)
          }
          if (lane == 16) {
            r.post16[g] = nv;
            if (is_last) nv ^= KT_PAD_CONST;
          }
          mem[lane] = nv;
        }
      }
    } else if (lane < 25) {
      mem[lane] = r.states[g * 25 + lane];
    }
    __syncthreads();
    for (int round = 0; round < KT_ROUNDS; round++) {
      const int base = KT_IP0 + KT_PERIOD * round;
#pragma unroll
      for (int l = 0; l < KT_LEVELS; l++) {
        if (e[l] != KT_IDLE) {
          const u32 op = (e[l] >> 7) & 7, at = base + (e[l] & 127);
          const u64 a = mem[at - ((e[l] >> 16) & 255)];
          const u64 bb = op == KT_ROL ? 0 : mem[at - (e[l] >> 24)];
          const u64 rv = op == KT_ANDNOT ? ~a & bb : a ^ bb;
          mem[at] = kt_rol(rv, (e[l] >> 10) & 63);
        }
        __syncthreads();
      }
    }
    u64* img = r.image + g * KT_WORDS;
    for (int i = lane; i < KT_WORDS; i += 64) img[i] = mem[i];
    if (lane < 25) out = mem[KT_OUT0 + lane];
    __syncthreads();
    if (lane < 25) {
      mem[lane] = out;
      if (r.perm_out) r.perm_out[g * 25 + lane] = out;
    }
    __syncthreads();
  }
  if (r.digests && lane < 4) r.digests[(size_t)m * 4 + lane] = out;
}

// ---- round_rows ----
__global__ __launch_bounds__(KT_BT) void k_kt_round_rows(const u64* __restrict__ image, const KtTab* __restrict__ tab, u64 n_perms, u64 ppl,
                                                         u64* __restrict__ base, u64 height) {
  __shared__ u32 s_prog[KT_PERIOD];
  if (threadIdx.x < KT_PERIOD) s_prog[threadIdx.x] = tab->prog[threadIdx.x];
  __syncthreads();
  const u64 t = (u64)blockIdx.x * KT_BT + threadIdx.x;
  if (t >= 2 * height) return;
  const u64 pl = t >= height, row = t - pl * height;
  const u64 first = pl * ppl, lane_perms = n_perms > first ? (n_perms - first < ppl ? n_perms - first : ppl) : 0;
  const u64 pi = row / KT_CYCLE;
  const u32 rr = (u32)(row - pi * KT_CYCLE);
  u64 a = 0, b = 0, rv = 0, lo = 0, hi = 0, act = 0;
  if (pi < lane_perms) {
    const u32 e = s_prog[rr & (KT_PERIOD - 1)], op = (e >> 7) & 7;
    const u64* at = image + (size_t)(first + pi) * KT_WORDS + KT_IP0 + rr;
    if (op != KT_NOP) a = at[-(int)((e >> 16) & 255)];
    if (op == KT_XOR || op == KT_ANDNOT || op == KT_XORROL) b = at[-(int)(e >> 24)];
    rv = op == KT_ANDNOT ? ~a & b : a ^ b;
    if (op == KT_ROL || op == KT_XORROL) {  // the half-swap takes rotations >= 32: the limbs are those of the shift mod 32
      const u32 k = (e >> 10) & 31;
      lo = ((rv & 0xffffffffull) + (1ull << 32)) << k;
      hi = ((rv >> 32) + (1ull << 32)) << k;
    }
    act = rr < KT_ROUNDS * KT_PERIOD;
  }
  u64* cell = base + (size_t)pl * KT_BAND * height + row;
  cell[0] = KT_IP0 + first * KT_CYCLE + row;  // ungated: runs over pad rows in both lanes
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cell[(size_t)(1 + i) * height] = (a >> (8 * i)) & 0xff;
    cell[(size_t)(9 + i) * height] = (b >> (8 * i)) & 0xff;
    cell[(size_t)(17 + i) * height] = (rv >> (8 * i)) & 0xff;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    cell[(size_t)(25 + i) * height] = (lo >> (16 * i)) & 0xffff;
    cell[(size_t)(29 + i) * height] = (hi >> (16 * i)) & 0xffff;
  }
  cell[(size_t)33 * height] = act;
}

// ---- sponge_rows ----
__global__ __launch_bounds__(KT_BT) void k_kt_sponge_rows(KtSponge s) {
  const u64 row = (u64)blockIdx.x * KT_BT + threadIdx.x;
  if (row >= s.height) return;
  const u64 g = row >> 5;
  const u32 slot = (u32)row & 31;
  const u32 rate_slots = slot < KT_RATE_LANES ? slot : KT_RATE_LANES;  // rate slots of this block above the row
  u64 act = 0, is_first = 0, is_zero = 0, avail = 0, chunk_ptr = s.pad_chunk_ptr;
  u64 chunk = 0, prev = 0, nw = 0, outv = 0, cleared = 0, padded = 0;
  u32 pad_byte = 8;  // no byte-offset flag
  long long bytes_left;
  if (g < s.n_blocks) {
    // the message of the wave's first row by binary search, the lane's own a step on (a message has a block at least)
    const u32 wave_first = (u32)((row & ~(u64)63) >> 5);
    u32 m = 0, top = s.n_msgs;
    while (top - m > 1) {
      const u32 mid = (m + top) >> 1;
      if (s.block_off[mid] <= wave_first) m = mid;
      else top = mid;
    }
    while (m + 1 < s.n_msgs && s.block_off[m + 1] <= (u32)g) m++;
    const mh_keccak_msg msg = s.msgs[m];
    const u32 b0 = s.block_off[m], b = (u32)g - b0, n_blocks = s.block_off[m + 1] - b0;
    const bool is_last = b + 1 == n_blocks;
    const u64 chunk_lanes = 4 * (msg.len ? (msg.len + 31) / 32 : 1);
    const u64 last_bytes = msg.len - (u64)KT_RATE_BYTES * (n_blocks - 1);
    const u32 pad_lane = (u32)last_bytes >> 3;
    const u32 in_block = is_last ? (u32)(chunk_lanes - (u64)KT_RATE_LANES * b) : KT_RATE_LANES;  // <= 20
    const u32 rate_avail = in_block < KT_RATE_LANES ? in_block : KT_RATE_LANES, overshoot = in_block - rate_avail;
    const bool is_rate = slot < KT_RATE_LANES, is_extra = slot >= 26 && slot < 29;
    const bool consume = (is_rate && slot < rate_avail) || (is_extra && slot - 26 < overshoot);
    const u32 extra_before = slot > 26 ? (slot - 26 < overshoot ? slot - 26 : overshoot) : 0;
    const u64 pos = (u64)KT_RATE_LANES * b + (slot < rate_avail ? slot : rate_avail) + extra_before;  // lanes consumed above the row
    act = 1;
    bytes_left = (long long)msg.len - 8 * ((long long)KT_RATE_LANES * b + rate_slots);
    chunk_ptr = 4 * msg.chunk_head + pos;
    is_first = b == 0;
    is_zero = is_last && slot > pad_lane;
    avail = slot < (overshoot ? 26 + overshoot : rate_avail);
    if (is_last) pad_byte = (u32)last_bytes & 7;
    if (consume) chunk = kt_tape(s.bytes, msg.offset, msg.len, pos);
    if (slot < 25) {
      prev = s.at_start[g * 25 + slot];
      if (is_last) outv = s.perm_out[g * 25 + slot];
      nw = prev;
      if (is_rate) {
        if (is_last && slot == pad_lane) {
          cleared = ~(~0ull << (8 * pad_byte)) & chunk;
          padded = cleared ^ (1ull << (8 * pad_byte));
          nw = prev ^ padded;
        } else if (!is_last || slot < pad_lane) {
          nw = prev ^ chunk;
        }
      }
    } else if (slot == 25) {
      prev = s.post16[g];
      nw = is_last ? prev ^ KT_PAD_CONST : prev;
    }
  } else {
    bytes_left = s.pad_bytes_left - 8 * ((long long)KT_RATE_LANES * (long long)(g - s.n_blocks) + rate_slots);
  }
  u64* cell = s.base + row;
  const u64 h = s.height;
  cell[0] = row;
  cell[1 * h] = act;
  cell[2 * h] = bytes_left < 0 ? KT_P + (u64)bytes_left : (u64)bytes_left;  // mod p
  cell[3 * h] = is_first;
  cell[4 * h] = chunk_ptr;
  cell[5 * h] = is_zero;
  cell[6 * h] = avail;
#pragma unroll
  for (u32 i = 0; i < 8; i++) cell[(size_t)(7 + i) * h] = i == pad_byte;
  kt_put<15, 27>(cell, h, chunk);
  kt_put<17, 35>(cell, h, prev);
  kt_put<19, 43>(cell, h, nw);
  kt_put<21, -1>(cell, h, outv);
  kt_put<23, 51>(cell, h, cleared);
  kt_put<25, 59>(cell, h, padded);
}

namespace {
inline u64 kt_pow2_at_least(u64 x) {
  u64 h = 1;
  while (h < x) h <<= 1;
  return h;
}
inline int kt_log2(u64 pow2) {
  int l = 0;
  while (((u64)1 << l) < pow2) l++;
  return l;
}
inline u64 kt_round_height(u64 n_perms) {  // max(2, next_pow2(ceil(max(n, 1) / 2) * 3200))
  const u64 ppl = ((n_perms ? n_perms : 1) + 1) / 2;
  return kt_pow2_at_least(ppl * KT_CYCLE);
}
inline u64 kt_sponge_height(u64 n_blocks) { return n_blocks ? kt_pow2_at_least(KT_SPONGE_PERIOD * n_blocks) : KT_SPONGE_PERIOD; }
constexpr u64 KT_MAX_PERMS = 2 * (SEC_MAX_ROWS / KT_CYCLE);  // the round trace of more permutations is above 2^24 rows

void kt_round_rows(mh_ctx* c, const u64* image, const KtTab* tab, u64 n_perms, mh_trace* t) {
  const u64 height = (u64)1 << t->log_n;
  ProfScope ps(c, "kt_round_rows", (16.0 + 8.0 * KT_BAND) * 2.0 * (double)height);
  MH_LAUNCH(k_kt_round_rows, dim3(sec_grid(2 * height, KT_BT)), dim3(KT_BT), 0, c->stream, image, tab, n_perms, ((n_perms ? n_perms : 1) + 1) / 2,
            t->cols.u(), height);
}

[[noreturn]] void kt_refuse(mh_keccak_traces_info* info, int kind, u64 index, const char* what) {
  info->defect_kind = kind;
  info->defect_index = index;
  char buf[256];
  snprintf(buf, sizeof buf, "mh_keccak_traces_build: defect %d, message %llu: %s", kind, (unsigned long long)index, what);
  throw MhError(MH_ERR_INVALID, buf);
}
}  // namespace

extern "C" int mh_keccak_round_program(int32_t* out) {
  if (!out) return MH_ERR_INVALID;
  KtSlot s[KT_PERIOD];
  kt_slots(s);
  for (int i = 0; i < KT_PERIOD; i++) {
    const int32_t row[5] = {s[i].op, s[i].shift, s[i].back_a, s[i].back_b, s[i].mult};
    memcpy(out + 5 * i, row, sizeof row);
  }
  return MH_OK;
}

extern "C" int mh_keccak_round_levels(int32_t* out) {
  if (!out) return MH_ERR_INVALID;
  KtSlot s[KT_PERIOD];
  int level[KT_PERIOD];
  kt_slots(s);
  kt_levels(s, level);
  for (int i = 0; i < KT_PERIOD; i++) out[i] = level[i];
  return MH_OK;
}

extern "C" int mh_keccak_round_trace_build(mh_ctx* c, const uint64_t* states, size_t n_perms, int log_n, mh_trace** out, uint64_t* outputs) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  try {
    MH_REQUIRE(out && (states || !n_perms), "mh_keccak_round_trace_build: null argument");
    MH_REQUIRE(log_n == -1 || (log_n >= 1 && log_n <= 24), "mh_keccak_round_trace_build: log_n lies in 1..24, or is -1");
    MH_REQUIRE(n_perms <= KT_MAX_PERMS, "mh_keccak_round_trace_build: more than 2^24 rows");
    const u64 least = kt_round_height(n_perms);
    if (log_n < 0) log_n = kt_log2(least);
    if (((u64)1 << log_n) < least) {
      char buf[200];
      snprintf(buf, sizeof buf, "mh_keccak_round_trace_build: the trace does not fit: %llu rows needed, 2^%d at hand", (unsigned long long)least, log_n);
      throw MhError(MH_ERR_INVALID, buf);
    }
    HIP_CHECK(hipSetDevice(c->device));
    KtTab tab;
    kt_table(tab);
    DevBuf dtab(sizeof tab), dstates(n_perms * 200), image(n_perms * KT_WORDS * 8), dout(outputs ? n_perms * 200 : 0);
    c->h2d(dtab.p, &tab, sizeof tab);
    std::unique_ptr<mh_trace> t = trace_new(c, log_n, KT_ROUND_WIDTH);
    if (n_perms) {
      c->h2d(dstates.p, states, n_perms * 200);
      KtRun r{(const KtTab*)dtab.p, nullptr, nullptr, nullptr, dstates.u(), image.u(), nullptr, nullptr, dout.u(), nullptr};
      ProfScope ps(c, "kt_absorb_permute", (200.0 + 8.0 * KT_WORDS) * (double)n_perms);
      MH_LAUNCH(k_kt_absorb_permute, dim3((unsigned)n_perms), dim3(64), 0, c->stream, r);
    }
    kt_round_rows(c, image.u(), (const KtTab*)dtab.p, n_perms, t.get());
    if (outputs && n_perms) c->d2h(outputs, dout.p, n_perms * 200);
    *out = t.release();
    return MH_OK;
  }
  SEC_CATCH
}

extern "C" int mh_keccak_traces_build(mh_ctx* c, const uint8_t* bytes, size_t n_bytes, const mh_keccak_msg* msgs, size_t n_msgs, int log_round,
                                      int log_sponge, mh_trace** round_out, mh_trace** sponge_out, uint8_t* digests, mh_keccak_traces_info* info) {
  if (!c) return MH_ERR_INVALID;
  PoolScope _ps(c);
  mh_keccak_traces_info local;
  if (!info) info = &local;
  try {
    *info = mh_keccak_traces_info{};
    if (!round_out || !sponge_out || (!msgs && n_msgs) || (!bytes && n_bytes)) kt_refuse(info, 4, 0, "a null pointer where one is required");
    MH_REQUIRE((log_round == -1 || (log_round >= 1 && log_round <= 24)) && (log_sponge == -1 || (log_sponge >= 5 && log_sponge <= 24)),
               "mh_keccak_traces_build: log_round lies in 1..24, log_sponge in 5..24, or either is -1");
    u64 n_blocks = 0;
    for (size_t i = 0; i < n_msgs; i++) {
      const mh_keccak_msg& m = msgs[i];
      if (m.offset > n_bytes || m.len > n_bytes - m.offset) kt_refuse(info, 1, i, "offset + len lies past n_bytes");
      const u64 chunk_lanes = 4 * (m.len ? (m.len + 31) / 32 : 1);
      if (m.chunk_head >= ((u64)1 << 30) || 4 * m.chunk_head + chunk_lanes >= ((u64)1 << 32))
        kt_refuse(info, 2, i, "4 * chunk_head plus the message's lanes does not fit 32 bits");
      n_blocks += m.len / KT_RATE_BYTES + 1;
      if (n_blocks > KT_MAX_PERMS) kt_refuse(info, 3, i, "more than 2^24 rows in the round trace");  // the sponge's 32 rows a block stay below
    }
    info->n_perms = n_blocks;
    info->sponge_rows = KT_SPONGE_PERIOD * n_blocks;
    info->round_rows_needed = kt_round_height(n_blocks);
    info->sponge_rows_needed = kt_sponge_height(n_blocks);
    if (log_round < 0) log_round = kt_log2(info->round_rows_needed);
    if (log_sponge < 0) log_sponge = kt_log2(info->sponge_rows_needed);
    if (((u64)1 << log_round) < info->round_rows_needed) kt_refuse(info, 5, info->round_rows_needed, "the round trace does not fit log_round (index: rows needed)");
    if (((u64)1 << log_sponge) < info->sponge_rows_needed) kt_refuse(info, 6, info->sponge_rows_needed, "the sponge trace does not fit log_sponge (index: rows needed)");
    HIP_CHECK(hipSetDevice(c->device));
    KtTab tab;
    kt_table(tab);
    const u32 tiles = sec_grid(n_msgs, HS_TILE);
    DevBuf dtab(sizeof tab), dbytes(n_bytes), dmsgs(n_msgs * sizeof(mh_keccak_msg)), block_off((n_msgs + 1) * 4), agg((size_t)tiles * 8), totals(16);
    DevBuf image(n_blocks * KT_WORDS * 8), at_start(n_blocks * 200), post16(n_blocks * 8), perm_out(n_blocks * 200), ddig(digests ? n_msgs * 32 : 0);
    c->h2d(dtab.p, &tab, sizeof tab);
    std::unique_ptr<mh_trace> rt = trace_new(c, log_round, KT_ROUND_WIDTH), st = trace_new(c, log_sponge, KT_SPONGE_WIDTH);
    long long pad_bytes_left = 0;
    u64 pad_chunk_ptr = 0;
    if (n_msgs) {
      c->h2d(dbytes.p, bytes, n_bytes);
      c->h2d(dmsgs.p, msgs, n_msgs * sizeof(mh_keccak_msg));
      const mh_keccak_msg& last = msgs[n_msgs - 1];
      pad_bytes_left = (long long)last.len - (long long)KT_RATE_BYTES * (long long)(last.len / KT_RATE_BYTES + 1);
      pad_chunk_ptr = 4 * last.chunk_head + 4 * (last.len ? (last.len + 31) / 32 : 1);
      {
        ProfScope ps(c, "kt_offsets", 56.0 * (double)n_msgs);
        MH_LAUNCH(k_kt_block_sums, dim3(tiles), dim3(HS_BT), 0, c->stream, (const mh_keccak_msg*)dmsgs.p, (u32)n_msgs, (u32*)agg.p, tiles);
        MH_LAUNCH(k_hs_carries, dim3(1), dim3(64), 0, c->stream, (u32*)agg.p, tiles, (unsigned long long*)totals.p, (unsigned long long*)totals.p + 1);
        MH_LAUNCH(k_kt_offsets, dim3(tiles), dim3(HS_BT), 0, c->stream, (const mh_keccak_msg*)dmsgs.p, (u32)n_msgs, (const u32*)agg.p, (u32*)block_off.p);
      }
      KtRun r{(const KtTab*)dtab.p, (const uint8_t*)dbytes.p, (const mh_keccak_msg*)dmsgs.p, (const u32*)block_off.p, nullptr, image.u(),
              at_start.u(), post16.u(), perm_out.u(), digests ? ddig.u() : nullptr};
      ProfScope ps(c, "kt_absorb_permute", (double)n_bytes + (408.0 + 8.0 * KT_WORDS) * (double)n_blocks);
      MH_LAUNCH(k_kt_absorb_permute, dim3((unsigned)n_msgs), dim3(64), 0, c->stream, r);
    }
    kt_round_rows(c, image.u(), (const KtTab*)dtab.p, n_blocks, rt.get());
    {
      const u64 height = (u64)1 << log_sponge;
      KtSponge s{(const uint8_t*)dbytes.p, (const mh_keccak_msg*)dmsgs.p, (const u32*)block_off.p, (u32)n_msgs, (u32)n_blocks, at_start.u(), post16.u(),
                 perm_out.u(), pad_bytes_left, pad_chunk_ptr, st->cols.u(), height};
      ProfScope ps(c, "kt_sponge_rows", (32.0 + 8.0 * KT_SPONGE_WIDTH) * (double)height);
      MH_LAUNCH(k_kt_sponge_rows, dim3(sec_grid(height, KT_BT)), dim3(KT_BT), 0, c->stream, s);
    }
    if (digests && n_msgs) c->d2h(digests, ddig.p, n_msgs * 32);
    *round_out = rt.release();
    *sponge_out = st.release();
    return MH_OK;
  }
  SEC_CATCH
}
