// The per-lane bodies of the uint traces' device stage (uint_traces.hip): the witness pass and the two row writers, as host-device
// functions (as gl.cuh's field arithmetic is).  The kernels of uint_traces.hip are their only callers in the library;
// tools/uint_traces_cpu.cpp runs the same bodies lane by lane on the host for tests/test_uint_traces_cpu.py.
//
// Column orders and the rule: uint/trace.rs:273-386, uint/mul/trace.rs:90-180 and 278-384, uint/store_mul/trace.rs:43-72,
// uint/add/trace.rs:104-215.
#pragma once
#include "../../include/midenhip.h"
#include "gl.cuh"
#include "ledger_stage.cuh"
#include "wave_count.cuh"

namespace {
constexpr int UT_USM_WIDTH = 44, UT_ADD_WIDTH = 30, UT_STORE_COLS = 18, UT_MUL_COLS = 26;
constexpr int UT_WITNESS_BT = 64, UT_ROWS_BT = 256;
constexpr u32 UT_ABSENT = 0xffffffffu;
// a multiply relation's record, in 32-bit words: the quotient (272 bits) 0..8, borrow 9, the 31 carries + 2^31 10..40 (as 16-bit halves:
// exactly the 62 cells of `gamma_slots`, in order), 41 zero, the row indices of a, b, c, r, bound 42..46, 47 zero
constexpr int UT_MREC = 48, UT_MREC_BORROW = 9, UT_MREC_GAMMA = 10, UT_MREC_INDEX = 42;
constexpr int UT_AREC = 8;  // an addition's: the row indices of a, b, c, bound (UT_ABSENT: no such operand), k, three zeros

struct UtLists {
  const mh_uint_row* rows;
  const u32* bound_index;  // [n_store]
  const mh_uint_mul_op* muls;
  const mh_uint_add_op* adds;
  u32 n_store, n_mul, n_add;
  u32* count;              // [n_store][2]: UintVal, UintLimbs reads by these two chiplets and the store itself
  u32* mrec;               // [n_mul][UT_MREC]
  u32* arec;               // [n_add][UT_AREC]
  unsigned long long* defect;
};

GL_HD u32 ut_find(const mh_uint_row* rows, u32 n, u32 ptr) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (rows[mid].ptr < ptr) lo = mid + 1; else hi = mid;
  }
  return lo < n && rows[lo].ptr == ptr ? lo : UT_ABSENT;
}

// One read of a store row: agreeing lanes of a wave add once (wave_count.cuh)
GL_HD void ut_count(u32* counter) { wave_count(counter); }

GL_HD void ut_load(u32 (&v)[8], const mh_uint_row* rows, u32 index) {
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = index == UT_ABSENT ? 0 : rows[index].value[j];
}

// 16-bit limb i of a value held in 32-bit limbs; i is a compile-time constant wherever this is used
#define UT_H16(x, i) (((x)[(i) >> 1] >> (16 * ((i) & 1))) & 0xffffu)

// every stored value reads its bound
GL_HD void ut_self(const UtLists& L, u32 i) { ut_count(&L.count[2 * (size_t)L.bound_index[i]]); }

GL_HD void ut_mul_witness(const UtLists& L, u32 i) {
  const mh_uint_mul_op op = L.muls[i];
  const u32 ia = ut_find(L.rows, L.n_store, op.a), ib = ut_find(L.rows, L.n_store, op.b), ic = ut_find(L.rows, L.n_store, op.c),
            ir = ut_find(L.rows, L.n_store, op.r), ip = ut_find(L.rows, L.n_store, op.bound);
  if (ia == UT_ABSENT || ib == UT_ABSENT || ic == UT_ABSENT || ir == UT_ABSENT || ip == UT_ABSENT) {
    ledger_report(L.defect, 8, 1, i, ia == UT_ABSENT ? 0 : ib == UT_ABSENT ? 1 : ic == UT_ABSENT ? 2 : ir == UT_ABSENT ? 3 : 4);
    return;
  }
  if (op.kappa_a >= 0x10000u || op.kappa_c >= 0x10000u) {
    ledger_report(L.defect, 9, 1, i, op.kappa_a >= 0x10000u ? 0 : 1);
    return;
  }
  const bool is_sub = op.is_sub != 0;
  u32 a[8], b[8], c[8], r[8], p[8];
  ut_load(a, L.rows, ia); ut_load(b, L.rows, ib); ut_load(c, L.rows, ic); ut_load(r, L.rows, ir); ut_load(p, L.rows, ip);

  // the numerator N = |kappa_a a b +- kappa_c c| in 17 limbs (< 2^529), `neg` its sign
  u32 N[17];
  {
    u32 ab[16];
#pragma unroll
    for (int k = 0; k < 16; k++) ab[k] = 0;
#pragma unroll
    for (int x = 0; x < 8; x++) {
      u64 carry = 0;
#pragma unroll
      for (int y = 0; y < 8; y++) {
        const u64 t = (u64)a[x] * b[y] + ab[x + y] + carry;  // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        ab[x + y] = (u32)t;
        carry = t >> 32;
      }
      ab[x + 8] = (u32)carry;
    }
    u64 carry = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u64 t = (u64)ab[k] * op.kappa_a + carry;
      N[k] = (u32)t;
      carry = t >> 32;
    }
    N[16] = (u32)carry;
  }
  bool neg = false;
  {
    u32 lin[9];
    u64 carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const u64 t = (u64)c[k] * op.kappa_c + carry;
      lin[k] = (u32)t;
      carry = t >> 32;
    }
    lin[8] = (u32)carry;
    if (!is_sub) {
      u64 cy = 0;
#pragma unroll
      for (int k = 0; k < 17; k++) {
        const u64 t = (u64)N[k] + (k < 9 ? lin[k] : 0u) + cy;
        N[k] = (u32)t;
        cy = t >> 32;
      }
    } else {
      u64 br = 0;
#pragma unroll
      for (int k = 0; k < 17; k++) {
        const u64 t = (u64)N[k] - (k < 9 ? lin[k] : 0u) - br;
        N[k] = (u32)t;
        br = (t >> 32) & 1;
      }
      neg = br != 0;
      if (neg) {  // the magnitude: two's complement of the 544-bit difference
        u64 cy = 1;
#pragma unroll
        for (int k = 0; k < 17; k++) {
          const u64 t = (u64)(~N[k]) + cy;
          N[k] = (u32)t;
          cy = t >> 32;
        }
      }
    }
  }

  // N = Q M + R, M = bound + 1 in nine limbs (2^256 when the bound is all ones).  Restoring division, a bit a step: R < M <= 2^256
  // before the shift, < 2^257 after it.
  u32 M[9], R[9], Q[17];
  {
    u64 cy = 1;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const u64 t = (u64)p[k] + cy;
      M[k] = (u32)t;
      cy = t >> 32;
    }
    M[8] = (u32)cy;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = 0;
#pragma unroll
  for (int w = 16; w >= 0; w--) {
    u32 x = N[w], qw = 0;
#pragma unroll 1
    for (int bit = 0; bit < 32; bit++) {
#pragma unroll
      for (int k = 8; k > 0; k--) R[k] = (R[k] << 1) | (R[k - 1] >> 31);
      R[0] = (R[0] << 1) | (x >> 31);
      x <<= 1;
      u32 T[9];
      u64 br = 0;
#pragma unroll
      for (int k = 0; k < 9; k++) {
        const u64 t = (u64)R[k] - M[k] - br;
        T[k] = (u32)t;
        br = (t >> 32) & 1;
      }
      const bool ge = br == 0;
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = ge ? T[k] : R[k];
      qw = (qw << 1) | (ge ? 1u : 0u);
    }
    Q[w] = qw;
  }

  // canonical_q: the quotient, the remainder the op must name, the borrow
  u32 borrow = 0;
  bool bad_r = false, bad_q = false, bad_under = false;
  if (!neg) {
#pragma unroll
    for (int k = 0; k < 8; k++) bad_r |= R[k] != r[k];
    bad_q = (Q[8] >> 16) != 0;
#pragma unroll
    for (int k = 9; k < 17; k++) bad_q |= Q[k] != 0;
  } else {
    bool rd_zero = true;
#pragma unroll
    for (int k = 0; k < 9; k++) rd_zero &= R[k] == 0;
    u64 br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {  // M - rd < 2^256 when rd != 0
      const u64 t = (u64)M[k] - R[k] - br;
      bad_r |= (rd_zero ? 0u : (u32)t) != r[k];
      br = (t >> 32) & 1;
    }
    bad_under = Q[0] >= 2;
#pragma unroll
    for (int k = 1; k < 17; k++) bad_under |= Q[k] != 0;
    borrow = Q[0] + (rd_zero ? 0u : 1u);
#pragma unroll
    for (int k = 0; k < 17; k++) Q[k] = 0;
  }
  if (bad_r || bad_q || bad_under) {
    ledger_report(L.defect, bad_r ? 10 : bad_q ? 11 : 12, 1, i, 0);
    return;
  }

  // gamma_halves: d_0..d_31 of kappa_a a(X) b(X) - q(X) (bound(X) + 1) + borrow (bound(X) + 1) +- kappa_c C(X^2) - R(X^2) over 16-bit limbs,
  // divided by X - 2^16.  A sum of 16 products below 2^32 times a 16-bit scale stays below 2^52.
  u32* rec = L.mrec + (size_t)i * UT_MREC;
  long long prev = 0;
  bool inexact = false, window = false;
#pragma unroll
  for (int k = 0; k < 32; k++) {
    u64 sab = 0, sqp = 0;
#pragma unroll
    for (int x = 0; x < 16; x++)
      if (k - x >= 0 && k - x < 16) sab += (u64)(UT_H16(a, x) * UT_H16(b, k - x));
#pragma unroll
    for (int x = 0; x < 17; x++)
      if (k - x >= 0 && k - x < 16) sqp += (u64)(UT_H16(Q, x) * UT_H16(p, k - x));
    long long d = (long long)(sab * op.kappa_a) - (long long)sqp;
    if (k < 17) d -= (long long)UT_H16(Q, k);
    if (k < 16) d += (long long)((u64)borrow * UT_H16(p, k));
    if (k == 0) d += (long long)borrow;
    if (k < 16 && (k & 1) == 0) {
      const long long lin = (long long)((u64)op.kappa_c * c[k >> 1]);
      d += (is_sub ? -lin : lin) - (long long)r[k >> 1];
    }
    const long long num = d + prev;
    if (k < 31) {
      inexact |= (num & 0xffff) != 0;
      const long long g = num >> 16;
      window |= g <= -((long long)1 << 31) || g >= ((long long)1 << 31);
      rec[UT_MREC_GAMMA + k] = (u32)(g + ((long long)1 << 31));
      prev = g;
    } else {
      inexact |= num != 0;
    }
  }
  if (inexact || window) {
    ledger_report(L.defect, inexact ? 10 : 13, 1, i, 0);
    return;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) rec[k] = Q[k];
  rec[UT_MREC_BORROW] = borrow;
  rec[41] = 0;
  rec[UT_MREC_INDEX + 0] = ia; rec[UT_MREC_INDEX + 1] = ib; rec[UT_MREC_INDEX + 2] = ic; rec[UT_MREC_INDEX + 3] = ir; rec[UT_MREC_INDEX + 4] = ip;
  rec[47] = 0;
  // the multiplier reads a, b and the bound over UintLimbs, c and r over UintVal
  ut_count(&L.count[2 * (size_t)ia + 1]);
  ut_count(&L.count[2 * (size_t)ib + 1]);
  ut_count(&L.count[2 * (size_t)ip + 1]);
  ut_count(&L.count[2 * (size_t)ic]);
  ut_count(&L.count[2 * (size_t)ir]);
}

GL_HD void ut_add_witness(const UtLists& L, u32 i) {
  const mh_uint_add_op op = L.adds[i];
  const u32 ia = ut_find(L.rows, L.n_store, op.a), ib = op.b ? ut_find(L.rows, L.n_store, op.b) : UT_ABSENT,
            ic = op.c ? ut_find(L.rows, L.n_store, op.c) : UT_ABSENT, ip = ut_find(L.rows, L.n_store, op.bound);
  if (ia == UT_ABSENT || (op.b && ib == UT_ABSENT) || (op.c && ic == UT_ABSENT) || ip == UT_ABSENT) {
    ledger_report(L.defect, 8, 2, i, ia == UT_ABSENT ? 0 : (op.b && ib == UT_ABSENT) ? 1 : (op.c && ic == UT_ABSENT) ? 2 : 3);
    return;
  }
  u32 a[8], b[8], c[8], p[8];
  ut_load(a, L.rows, ia); ut_load(b, L.rows, ib); ut_load(c, L.rows, ic); ut_load(p, L.rows, ip);
  // a + b against c (k = 0) and c + bound + 1 (k = 1), in nine limbs
  u32 S[9], C1[9];
  u64 cs = 0, cc = 1;
  bool b_zero = true;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 s = (u64)a[j] + b[j] + cs, t = (u64)c[j] + p[j] + cc;
    S[j] = (u32)s; cs = s >> 32;
    C1[j] = (u32)t; cc = t >> 32;
    b_zero &= b[j] == 0;
  }
  S[8] = (u32)cs; C1[8] = (u32)cc;
  bool k0 = S[8] == 0, k1 = true;
#pragma unroll
  for (int j = 0; j < 8; j++) k0 &= S[j] == c[j];
#pragma unroll
  for (int j = 0; j < 9; j++) k1 &= S[j] == C1[j];
  if (!k0 && !k1) {
    ledger_report(L.defect, 10, 2, i, 0);
    return;
  }
  if (op.nz && b_zero) {
    ledger_report(L.defect, 14, 2, i, 1);
    return;
  }
  u32* rec = L.arec + (size_t)i * UT_AREC;
  rec[0] = ia; rec[1] = ib; rec[2] = ic; rec[3] = ip; rec[4] = k0 ? 0u : 1u; rec[5] = 0; rec[6] = 0; rec[7] = 0;
  ut_count(&L.count[2 * (size_t)ia]);
  if (ib != UT_ABSENT) ut_count(&L.count[2 * (size_t)ib]);
  if (ic != UT_ABSENT) ut_count(&L.count[2 * (size_t)ic]);
  ut_count(&L.count[2 * (size_t)ip]);
}

// ---- rows ----
GL_HD void ut_usm_row(const UtLists& L, u64 n, u64* __restrict__ out, u64 t) {
  {  // the store's half: block t / 4, role t % 4
    const u64 i = t >> 2;
    const int role = (int)(t & 3);
    u64 s[UT_STORE_COLS];
#pragma unroll
    for (int k = 0; k < UT_STORE_COLS; k++) s[k] = 0;
    if (i < L.n_store) {
      const mh_uint_row* row = L.rows + i;
      const unsigned short* v16 = (const unsigned short*)row->value;
      if (role == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = v16[k];
      } else if (role == 1) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = v16[8 + k];
        s[8] = (u64)row->val_reads + L.count[2 * i];       // three 32-bit counts: far below p
        s[9] = (u64)row->limb_reads + L.count[2 * i + 1];
      } else {
        const u32* bound = L.rows[L.bound_index[i]].value;
        u32 comp[8], carry[8];
        u64 br = 0, cy = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const u64 d = (u64)bound[k] - row->value[k] - br;
          comp[k] = (u32)d;
          br = (d >> 32) & 1;
          cy = ((u64)row->value[k] + comp[k] + cy) >> 32;
          carry[k] = (u32)cy;
        }
        if (role == 2) {
#pragma unroll
          for (int k = 0; k < 16; k++) s[k] = UT_H16(comp, k);
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            s[k] = bound[k];
            s[4 + k] = carry[k];
            s[8 + k] = bound[4 + k];
            if (k < 3) s[12 + k] = carry[4 + k];
          }
          s[15] = i + 1 < L.n_store ? (u64)(row[1].ptr - row->ptr - 1) : 0;
        }
      }
      s[16] = row->ptr;
      s[17] = row->bound_ptr;
    } else {  // a padding block: its own bound, value 0, read once
      const u64 ptr = (L.n_store ? (u64)L.rows[L.n_store - 1].ptr + 1 : 1) + (i - L.n_store);
      if (role == 1) s[8] = 1;
      s[16] = ptr;
      s[17] = ptr;
    }
#pragma unroll
    for (int k = 0; k < UT_STORE_COLS; k++) out[(size_t)k * n + t] = s[k];
  }
  {  // the multiplier's half: relation t / 8, row t % 8
    const u64 i = t >> 3;
    const int role = (int)(t & 7);
    u64 m[UT_MUL_COLS];
#pragma unroll
    for (int k = 0; k < UT_MUL_COLS; k++) m[k] = 0;
    if (i < L.n_mul) {
      const mh_uint_mul_op op = L.muls[i];
      const u32* rec = L.mrec + (size_t)i * UT_MREC;
      const unsigned short* h = (const unsigned short*)(rec + UT_MREC_GAMMA);  // the 62 halves in gamma_slots order
      if (role < 3) {  // a, b, the bound: sixteen limbs and three halves
        const unsigned short* v16 = (const unsigned short*)L.rows[rec[UT_MREC_INDEX + (role == 0 ? 0 : role == 1 ? 1 : 4)]].value;
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = v16[k];
#pragma unroll
        for (int k = 0; k < 3; k++) m[16 + k] = h[34 + 3 * role + k];
      } else if (role == 3) {
        const unsigned short* q16 = (const unsigned short*)rec;
#pragma unroll
        for (int k = 0; k < 17; k++) m[k] = q16[k];
        m[17] = h[43];
        m[18] = h[44];
      } else if (role == 4) {
        const u32* v = L.rows[rec[UT_MREC_INDEX + 3]].value;
#pragma unroll
        for (int k = 0; k < 8; k++) m[k] = v[k];
#pragma unroll
        for (int k = 0; k < 11; k++) m[8 + k] = h[45 + k];
      } else if (role == 5) {
#pragma unroll
        for (int k = 0; k < 19; k++) m[k] = h[k];
      } else if (role == 6) {
#pragma unroll
        for (int k = 0; k < 15; k++) m[k] = h[19 + k];
      } else {
        const u32* v = L.rows[rec[UT_MREC_INDEX + 2]].value;
#pragma unroll
        for (int k = 0; k < 8; k++) m[k] = v[k];
        m[8] = gl_canon(op.mult);
        m[9] = op.c;
        m[10] = op.kappa_c;
        m[11] = op.is_sub ? 1 : 0;
        m[12] = op.is_sub ? gl_neg(op.kappa_c) : (u64)op.kappa_c;
#pragma unroll
        for (int k = 0; k < 6; k++) m[13 + k] = h[56 + k];
      }
      m[19] = op.a; m[20] = op.b; m[21] = op.r; m[22] = op.bound; m[23] = op.kappa_a; m[24] = 1; m[25] = rec[UT_MREC_BORROW];
    }
#pragma unroll
    for (int k = 0; k < UT_MUL_COLS; k++) out[(size_t)(UT_STORE_COLS + k) * n + t] = m[k];
  }
}

GL_HD void ut_add_row(const UtLists& L, u64 n, u64* __restrict__ out, u64 t) {
  const u64 i = t >> 1;
  const bool closing = (t & 1) != 0;
  u64 s[UT_ADD_WIDTH];
#pragma unroll
  for (int k = 0; k < UT_ADD_WIDTH; k++) s[k] = 0;
  if (i < L.n_add) {
    const mh_uint_add_op op = L.adds[i];
    const u32* rec = L.arec + (size_t)i * UT_AREC;
    const u32 ib = rec[1], ic = rec[2], kk = rec[4];
    u32 a[8], b[8], c[8], p[8];
    ut_load(a, L.rows, rec[0]); ut_load(b, L.rows, ib); ut_load(c, L.rows, ic); ut_load(p, L.rows, rec[3]);
    // gamma_j = the carry of a + b out of limb j minus that of c + k (bound + 1), mod p
    u64 gamma[7], pos = 0, negc = 0, sum_b = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (j < 7) {
        pos = ((u64)a[j] + b[j] + pos) >> 32;
        negc = ((u64)c[j] + (kk ? (u64)p[j] : 0) + (j == 0 ? kk : 0u) + negc) >> 32;
        gamma[j] = gl_sub(pos, negc);
      }
      sum_b += b[j];
    }
    if (!closing) {
#pragma unroll
      for (int j = 0; j < 8; j++) { s[j] = a[j]; s[8 + j] = b[j]; }
#pragma unroll
      for (int j = 0; j < 4; j++) s[16 + j] = gamma[j];
      s[20] = ib == UT_ABSENT ? 1 : 0;
      if (op.nz) {
        const u64 w = gl_inv(sum_b);
        s[21] = w;
        s[22] = gl_mul(w, sum_b);
      }
      s[23] = ib == UT_ABSENT ? 0 : 1;
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) { s[j] = c[j]; s[8 + j] = p[j]; }
#pragma unroll
      for (int j = 0; j < 3; j++) s[16 + j] = gamma[4 + j];
      s[20] = kk;
      s[21] = ic == UT_ABSENT ? 0 : 1;
      s[22] = gl_canon(op.mult);
      s[23] = ic == UT_ABSENT ? 1 : 0;
    }
    s[24] = op.a; s[25] = op.b; s[26] = op.c; s[27] = op.bound; s[28] = 1; s[29] = op.nz ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < UT_ADD_WIDTH; k++) out[(size_t)k * n + t] = s[k];
}

}  // namespace
