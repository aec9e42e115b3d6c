// The per-lane bodies of the EC traces' device stage (ec_traces.hip): the counting and checking pass and the four row writers, as
// host-device functions (as gl.cuh's field arithmetic is).  The kernels of ec_traces.hip are their only callers in the library;
// tools/ec_traces_cpu.cpp runs the same bodies lane by lane on the host for tests/test_ec_traces_cpu.py.
//
// Column orders: EcGroupsAir ec/groups.rs:59-74, EcPointStoreAir ec/mod.rs:153-197, EcGroupAddAir ec/add/mod.rs:190-277, EcMsmAir
// ec/msm/mod.rs:157-273; the rule ec/trace.rs:347-411, ec/add/trace.rs:146-251, ec/msm/trace.rs:390-500.
#pragma once
#include "../../include/midenhip.h"
#include "gl.cuh"
#include "ledger_stage.cuh"
#include "wave_count.cuh"

namespace {
constexpr int EC_GROUPS_WIDTH = 6, EC_POINTS_WIDTH = 14, EC_ADD_WIDTH = 21, EC_MSM_WIDTH = 38;

struct EcLists {
  const mh_ec_group* groups;
  const mh_ec_point* points;
  const mh_ec_add_op* adds;
  const mh_msm_expr* exprs;
  const mh_msm_term* terms;
  const u32* row_start;  // [n_exprs]: every expression's first term row (the planner's)
  u32 n_groups, n_points, n_add, n_exprs, n_terms;
  u32* gcount;           // [n_groups]: the reads of a group by these four chiplets
  u32* pcount;           // [n_points]
  u32* ecount;           // [n_exprs]: the uses of an expression as an operand
  unsigned long long* defect;
};

// the first of `n` terms whose base is not below `base` (n when there is none): the merge's cursor in front of `base`
GL_HD u32 ec_lower_bound(const mh_msm_term* terms, u32 n, u32 base) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (terms[mid].base < base) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the expression that holds term row t < n_terms: the last k with row_start[k] <= t
GL_HD u32 ec_expr_of(const EcLists& L, u32 t) {
  u32 lo = 0, hi = L.n_exprs;
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (L.row_start[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

GL_HD u64 ec_mult(u64 ext, u32 count) { return gl_add(gl_canon(ext), (u64)count); }

// ---- the counting and checking pass ----
// every stored point reads its group (the planner has ranged `group`)
GL_HD void ec_point_check(const EcLists& L, u32 i) { wave_count(&L.gcount[L.points[i].group - 1]); }

GL_HD void ec_add_check(const EcLists& L, u32 i) {
  const mh_ec_add_op op = L.adds[i];
  const bool bad_p = op.p == 0 || op.p > L.n_points, bad_q = op.q == 0 || op.q > L.n_points, bad_r = op.r == 0 || op.r > L.n_points,
             bad_g = op.group == 0 || op.group > L.n_groups;
  if (bad_p || bad_q || bad_r || bad_g) {
    ledger_report(L.defect, 8, 2, i, bad_p ? 0 : bad_q ? 1 : bad_r ? 2 : 3);
    return;
  }
  if (op.kind > 5 || op.mints > 1 || (op.mints && op.kind < 4)) {
    ledger_report(L.defect, 9, 2, i, op.kind > 5 ? 0 : 1);
    return;
  }
  const mh_ec_point p = L.points[op.p - 1], q = L.points[op.q - 1], r = L.points[op.r - 1];
  if (p.group != op.group || q.group != op.group || r.group != op.group) {
    ledger_report(L.defect, 10, 2, i, p.group != op.group ? 0 : q.group != op.group ? 1 : 2);
    return;
  }
  const bool pai_p = p.kind == 1, pai_q = q.kind == 1;
  if (!(pai_p && pai_q ? op.kind == 2 : pai_p ? op.kind == 0 : pai_q ? op.kind == 1 : op.kind >= 3)) {
    ledger_report(L.defect, 11, 2, i, 0);
    return;
  }
  if (op.mints && (op.r <= op.p || op.r <= op.q || r.kind != 2)) {
    ledger_report(L.defect, 12, 2, i, op.r <= op.p ? 0 : op.r <= op.q ? 1 : 2);
    return;
  }
  wave_count(&L.pcount[op.p - 1]);
  wave_count(&L.pcount[op.q - 1]);
  if (op.kind >= 3) {  // the live cases read the group and the result's row
    wave_count(&L.gcount[op.group - 1]);
    wave_count(&L.pcount[op.r - 1]);
  }
}

// the planner has ranged kind, n_rows and the operands: a_expr, b_expr name earlier expressions wherever the kind has them
GL_HD void ec_expr_check(const EcLists& L, u32 k) {
  const mh_msm_expr e = L.exprs[k];
  const bool bad_v = e.val == 0 || e.val > L.n_points, bad_g = e.group == 0 || e.group > L.n_groups;
  if (bad_v || bad_g) {
    ledger_report(L.defect, 8, 3, k, bad_v ? 0 : 1);
    return;
  }
  const u32 a_group = e.kind != 0 ? L.exprs[e.a_expr - 1].group : e.group, b_group = e.kind == 1 ? L.exprs[e.b_expr - 1].group : e.group;
  if (L.points[e.val - 1].group != e.group || a_group != e.group || b_group != e.group) {
    ledger_report(L.defect, 10, 3, k, L.points[e.val - 1].group != e.group ? 0 : a_group != e.group ? 1 : 2);
    return;
  }
  if (e.kind == 0) {
    if (L.terms[L.row_start[k]].base != e.val) ledger_report(L.defect, 15, 3, k, 0);
    return;
  }
  wave_count(&L.gcount[e.group - 1]);
  wave_count(&L.ecount[e.a_expr - 1]);
  if (e.kind == 1) {
    wave_count(&L.ecount[e.b_expr - 1]);
  } else {  // a neg reads its operand's value point and its own
    const u32 val_a = L.exprs[e.a_expr - 1].val;
    if (val_a != 0 && val_a <= L.n_points) wave_count(&L.pcount[val_a - 1]);  // else: that expression's lane reports kind 8
    wave_count(&L.pcount[e.val - 1]);
  }
}

// a combine row's cursors and takes: i, j = the lower bounds of `base` in the operands' term lists
struct EcMerge {
  u32 sa, la, sb, lb;  // the operands' first term rows and lengths
  u32 i, j;
  bool take_a, take_b;
};

GL_HD EcMerge ec_merge_at(const EcLists& L, const mh_msm_expr& e, u32 base) {
  EcMerge m;
  m.sa = L.row_start[e.a_expr - 1]; m.la = L.exprs[e.a_expr - 1].n_rows;
  m.sb = L.row_start[e.b_expr - 1]; m.lb = L.exprs[e.b_expr - 1].n_rows;
  m.i = ec_lower_bound(L.terms + m.sa, m.la, base);
  m.j = ec_lower_bound(L.terms + m.sb, m.lb, base);
  m.take_a = m.i < m.la && L.terms[m.sa + m.i].base == base;
  m.take_b = m.j < m.lb && L.terms[m.sb + m.j].base == base;
  return m;
}

GL_HD void ec_term_check(const EcLists& L, u32 t) {
  const u32 k = ec_expr_of(L, t);
  const mh_msm_expr e = L.exprs[k];
  const u32 idx = t - L.row_start[k], base = L.terms[t].base;
  if (idx > 0 && L.terms[t - 1].base >= base) {
    ledger_report(L.defect, 13, 3, t, 0);
    return;
  }
  const bool last = idx + 1 == e.n_rows;
  if (e.kind == 1) {
    const EcMerge m = ec_merge_at(L, e, base);
    if (!m.take_a && !m.take_b) {
      ledger_report(L.defect, 14, 3, t, 0);
      return;
    }
    u32 ni = m.la, nj = m.lb;  // where the walk stands after this row: the next row's cursors, or both lists' ends
    if (!last) {
      const u32 next = L.terms[t + 1].base;
      ni = ec_lower_bound(L.terms + m.sa, m.la, next);
      nj = ec_lower_bound(L.terms + m.sb, m.lb, next);
    }
    if ((idx == 0 && (m.i != 0 || m.j != 0)) || m.i + (m.take_a ? 1u : 0u) != ni || m.j + (m.take_b ? 1u : 0u) != nj) ledger_report(L.defect, 14, 3, t, 1);
  } else if (e.kind == 2) {
    const u32 sa = L.row_start[e.a_expr - 1], la = L.exprs[e.a_expr - 1].n_rows;
    if (idx >= la || L.terms[sa + idx].base != base || (last && e.n_rows != la)) ledger_report(L.defect, 14, 3, t, 2);
  }
}

// ---- rows: the pass above has been read back clean, every pointer below is in range ----
GL_HD void ec_groups_row(const EcLists& L, u64 n, u64* __restrict__ out, u64 t) {
  u64 s[EC_GROUPS_WIDTH];
#pragma unroll
  for (int c = 0; c < EC_GROUPS_WIDTH; c++) s[c] = 0;
  s[0] = t + 1;
  if (t < L.n_groups) {
    const mh_ec_group g = L.groups[t];
    s[1] = g.a_ptr; s[2] = g.b_ptr; s[3] = g.bound_ptr; s[4] = g.sbound_ptr;
    s[5] = ec_mult(g.ext_reads, L.gcount[t]);
  }
#pragma unroll
  for (int c = 0; c < EC_GROUPS_WIDTH; c++) out[(size_t)c * n + t] = s[c];
}

GL_HD void ec_points_row(const EcLists& L, u64 n, u64* __restrict__ out, u64 t) {
  u64 s[EC_POINTS_WIDTH];
#pragma unroll
  for (int c = 0; c < EC_POINTS_WIDTH; c++) s[c] = 0;
  if (t < L.n_points) {
    const mh_ec_point p = L.points[t];
    const mh_ec_group g = L.groups[p.group - 1];
    s[0] = t + 1; s[1] = p.group;
    s[2] = g.a_ptr; s[3] = g.b_ptr; s[4] = g.bound_ptr; s[5] = g.sbound_ptr;
    s[6] = p.x_ptr; s[7] = p.y_ptr; s[8] = p.u_ptr; s[9] = p.w_ptr;
    s[10] = p.kind == 1 ? 1 : 0;
    s[11] = ec_mult(p.ext_reads, L.pcount[t]);
    s[12] = 1;
    s[13] = p.kind == 2 ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c < EC_POINTS_WIDTH; c++) out[(size_t)c * n + t] = s[c];
}

// addition t / 4, role t % 4: slope, tail, result, term
GL_HD void ec_add_row(const EcLists& L, u64 n, u64* __restrict__ out, u64 t) {
  const u64 i = t >> 2;
  const int role = (int)(t & 3);
  u64 s[EC_ADD_WIDTH];
#pragma unroll
  for (int c = 0; c < EC_ADD_WIDTH; c++) s[c] = 0;
  if (i < L.n_add) {
    const mh_ec_add_op op = L.adds[i];
    const mh_ec_group g = L.groups[op.group - 1];
    const mh_ec_point p = L.points[op.p - 1], q = L.points[op.q - 1];
    if (role == 0) {
      s[0] = op.t[0]; s[1] = op.t[1]; s[2] = op.t[2];
    } else if (role == 1) {
      s[0] = op.t[3]; s[1] = op.t[4]; s[2] = op.t[5];
    } else if (role == 2) {
      s[0] = op.r; s[1] = g.sbound_ptr; s[2] = op.group;
    } else {
      s[0] = gl_canon(op.mult); s[1] = op.p; s[2] = op.q;
    }
    s[3] = p.x_ptr; s[4] = p.y_ptr; s[5] = q.x_ptr; s[6] = q.y_ptr;  // 0 on the point at infinity's row
    s[7] = g.a_ptr; s[8] = g.b_ptr; s[9] = g.bound_ptr;
    s[10] = op.kind == 0 || op.kind == 2 ? 1 : 0;  // pai_p
    s[11] = op.kind == 1 || op.kind == 2 ? 1 : 0;  // pai_q
    s[12] = op.kind == 3 ? 1 : 0;
    s[13] = op.kind == 4 ? 1 : 0;
    s[14] = op.kind == 5 ? 1 : 0;
    s[15] = 1;
    s[16] = op.mints;
    if (op.mints) {  // r > p, r > q: checked
      const u32 rp = op.r - op.p - 1, rq = op.r - op.q - 1;
      s[17] = rp & 0xffffu; s[18] = rp >> 16; s[19] = rq & 0xffffu; s[20] = rq >> 16;
    }
  }
#pragma unroll
  for (int c = 0; c < EC_ADD_WIDTH; c++) out[(size_t)c * n + t] = s[c];
}

GL_HD void ec_msm_row(const EcLists& L, u64 n, u64* __restrict__ out, u64 t) {
  u64 s[EC_MSM_WIDTH];
#pragma unroll
  for (int c = 0; c < EC_MSM_WIDTH; c++) s[c] = 0;
  if (t < L.n_terms) {
    const u32 k = ec_expr_of(L, (u32)t);
    const mh_msm_expr e = L.exprs[k];
    const mh_msm_term term = L.terms[t];
    const mh_ec_group g = L.groups[e.group - 1];
    const u32 idx = (u32)t - L.row_start[k];
    const bool boundary = idx + 1 == e.n_rows;
    s[0] = 1; s[1] = k + 1; s[2] = boundary ? 1 : 0; s[3] = e.group; s[4] = g.sbound_ptr; s[5] = idx;
    s[6] = term.base; s[7] = term.scalar; s[8] = e.val;
    s[9] = ec_mult(e.ext_mult, L.ecount[k]);
    s[10] = e.kind == 0 ? 1 : 0; s[11] = e.kind == 1 ? 1 : 0; s[32] = e.kind == 2 ? 1 : 0;
    s[34] = gl_canon(e.claim_mult);
    if (e.kind != 0) {
      const mh_msm_expr a = L.exprs[e.a_expr - 1];
      s[12] = e.a_expr; s[23] = a.val;
      s[25] = g.a_ptr; s[26] = g.b_ptr; s[27] = g.bound_ptr;
      if (e.kind == 1) {
        const EcMerge m = ec_merge_at(L, e, term.base);
        s[13] = e.b_expr; s[24] = L.exprs[e.b_expr - 1].val;
        s[14] = m.i; s[15] = m.j;
        s[16] = m.take_a && !m.take_b ? 1 : 0; s[17] = m.take_b && !m.take_a ? 1 : 0; s[18] = m.take_a && m.take_b ? 1 : 0;
        if (m.take_a) { s[19] = term.base; s[20] = L.terms[m.sa + m.i].scalar; }
        if (m.take_b) { s[21] = term.base; s[22] = L.terms[m.sb + m.j].scalar; }
      } else {
        s[14] = idx; s[19] = term.base; s[20] = L.terms[L.row_start[e.a_expr - 1] + idx].scalar;
      }
      if (boundary) {
        const u32 da = k - e.a_expr;  // expr - a_expr - 1 with expr = k + 1
        s[28] = da & 0xffffu; s[29] = da >> 16;
        if (e.kind == 1) {
          const u32 db = k - e.b_expr;
          s[30] = db & 0xffffu; s[31] = db >> 16;
        } else {
          const mh_ec_point va = L.points[a.val - 1];
          s[33] = va.x_ptr; s[35] = va.y_ptr; s[36] = L.points[e.val - 1].y_ptr; s[37] = e.neg_minted;
        }
      }
    }
  } else {  // pads keep the next pointer, idx counts on from 0
    s[1] = (u64)L.n_exprs + 1;
    s[5] = t - L.n_terms;
  }
#pragma unroll
  for (int c = 0; c < EC_MSM_WIDTH; c++) out[(size_t)c * n + t] = s[c];
}
}  // namespace
