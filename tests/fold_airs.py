"""The AIRs and traces of tests/test_gpu_constraint_fold.py (a helper module, not a test): small constraint systems whose gates receive
the corner operands of tests/jit_corner_operands.py row by row.  tests/test_jit_corner_operands.py checks on the CPU that each layout
shows every product gate every carry; the GPU tests run them through mh_constraint_fold."""
import functools
import numpy as np
from __graft_entry__ import load_package

load_package()
from miden_vm_amd import dag  # noqa: E402
import jit_corner_operands as J

P = dag.P
HEIGHTS = (8, 256)  # 2^3: the interpreter fallback under a fused program; 2^8: one full 256-row tile, compiled


def _col(n, shift, which):
    return np.array(J.column_values(n, shift, which), dtype=np.uint64)


class Case:
    """An AIR with everything mh_constraint_fold wants for it at one height."""

    def __init__(self, air, main, aux=None, publics=(), rnd=(), avs=()):
        self.air, self.main, self.aux, self.publics, self.rnd, self.avs = air, main, aux, list(publics), list(rnd), list(avs)

    def kwargs(self):
        return dict(aux=self.aux, publics=self.publics, randomness=self.rnd, aux_values=self.avs)


# ---- 1. product lattice ------------------------------------------------------------------------------------------------------------
LATTICE_PAIRS = 6
LATTICE_SHIFT = 23  # pair i starts 23 entries further into the table: the gates of one row see different entries


def single_product_air():
    """K = 1: C = x * y - z.  With z = 0 and alpha = (1, 0) the fold IS the product."""
    b = dag.AirBuilder(3)
    b.assert_zero(b.main(0) * b.main(1) - b.main(2))
    return dag.Air(b, name="one_product")


def lattice_air(levels=3):
    """Columns (x_i, y_i, z_i), i < 6.  C_i = x_i y_i - z_i; a second level multiplies products (any-representative operands):
    (x0 y0)(x1 y1), (x2 y2) x3, (x4 y4)(x5 y5), (x1 y1) x0, (x3 y3) x2, and a third level on top of two of those -- thirteen products,
    which MH_JIT_MULGROUP=4 emits as lz_mulN<4>, <4>, <3> and <2> (the third level is not ready before the second is defined)."""
    b = dag.AirBuilder(3 * LATTICE_PAIRS)
    x = [b.main(3 * i) for i in range(LATTICE_PAIRS)]
    y = [b.main(3 * i + 1) for i in range(LATTICE_PAIRS)]
    z = [b.main(3 * i + 2) for i in range(LATTICE_PAIRS)]
    p = [x[i] * y[i] for i in range(LATTICE_PAIRS)]
    for i in range(LATTICE_PAIRS):
        b.assert_zero(p[i] - z[i])
    if levels == 1:  # the satisfiable part alone (z = x y): the consistency test with the checker
        return dag.Air(b, name="lattice1")
    q45, q10 = p[4] * p[5], p[1] * x[0]
    b.assert_zero(p[0] * p[1])
    b.assert_zero(p[2] * x[3])
    b.assert_zero(q45)
    b.assert_zero(q10)
    b.assert_zero(p[3] * x[2])
    b.assert_zero(q45 * x[1])
    b.assert_zero(q10 * y[2])
    return dag.Air(b, name="lattice")


def lattice_trace(n, pairs=LATTICE_PAIRS):
    t = np.zeros((n, 3 * pairs), dtype=np.uint64)
    for i in range(pairs):
        t[:, 3 * i] = _col(n, i * LATTICE_SHIFT, 0)
        t[:, 3 * i + 1] = _col(n, i * LATTICE_SHIFT, 1)
    return t


def lattice_case(n):
    return Case(lattice_air(), lattice_trace(n))


def single_product_case(n):
    return Case(single_product_air(), lattice_trace(n, 1))


def cell_products(air, main):
    """-> {gate: [(a, b) per row]} for every MUL gate of `air` whose operands are both main-trace cells: the gates whose operands a
    trace dictates exactly."""
    import dag_eval
    _, nodes, _ = dag_eval.parse(air.blob)
    n = main.shape[0]
    out = {}
    for g, (op, a, b, _) in enumerate(nodes):
        if op == dag.OP_MUL and nodes[a][0] == dag.OP_MAIN and nodes[b][0] == dag.OP_MAIN:
            (_, ca, ra, _), (_, cb, rb, _) = nodes[a], nodes[b]
            out[g] = [(int(main[(r + ra) % n, ca]), int(main[(r + rb) % n, cb])) for r in range(n)]
    return out


# ---- 2. extension products ---------------------------------------------------------------------------------------------------------
EF_RND = [(P - 1, 0xFFFFFFFEFFFFFFFF), ((1 << 32) - 1, 1 << 32)]
EF_AVS = [(0xFFFFFFFEFFFFFFFF, P - 1), (1, 0)]


def ef_air():
    """EF x EF, EF x base, products of products, a uniform product (randomness x aux value) against a column."""
    b = dag.AirBuilder(2, aux_width=4, num_randomness=2, num_aux_values=2)
    e = [b.aux(i) for i in range(4)]
    m0, m1 = b.main(0), b.main(1)
    r0, r1, a0, a1 = b.randomness(0), b.randomness(1), b.aux_value(0), b.aux_value(1)
    ee = e[0] * e[1]
    em = e[2] * m0
    b.assert_zero_ext(ee)
    b.assert_zero_ext(em)
    b.assert_zero_ext(e[0] * r0 + e[3] * a0)
    b.assert_zero_ext(ee * e[2])
    b.assert_zero_ext(em * m1)
    b.assert_zero_ext(r1 * a0 * e[3] + a1 * m1)
    b.assert_zero(m0 * m1)
    return dag.Air(b, name="ef_products")


def ef_case(n):
    main = np.stack([_col(n, 5, 1), _col(n, 61, 1)], axis=1)
    aux = np.zeros((n, 8), dtype=np.uint64)
    # e0 = (a[r], a[r + 40]), e1 = (b[r], b[r + 40]): a0 b0 and a1 b1 of e0 * e1 are table pairs, the cross products mix two entries
    aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3] = _col(n, 0, 0), _col(n, 40, 0), _col(n, 0, 1), _col(n, 40, 1)
    # e2 = (a[r + 5], a[r + 77]) against the base operand m0 = b[r + 5]: the first product of e2 * m0 is a table pair
    aux[:, 4], aux[:, 5] = _col(n, 5, 0), _col(n, 77, 0)
    aux[:, 6], aux[:, 7] = _col(n, 99, 1), _col(n, 17, 0)
    return Case(ef_air(), main, aux, rnd=EF_RND, avs=EF_AVS)


# ---- 3. sums, differences, negations of lazy values -----------------------------------------------------------------------------------
# A product below 2^64 leaves lz_mul as the integer itself: these pairs put a value in [p, 2^64) behind a sum (chosen inputs; the
# expected values are field arithmetic as everywhere).  0xFFFFFFFF * 0x100000001 = 2^64 - 1, 2 * (2^63 - 1) = 2^64 - 2.
BIG_PAIRS = [(0xFFFFFFFF, 0x100000001), (2, (1 << 63) - 1), (0x100, (1 << 56) - 1)]
SUM_PERIODIC = [[1, P - 1, 0xFFFFFFFF, 0xFFFFFFFEFFFFFFFF]]


def sums_air():
    b = dag.AirBuilder(6, periodic=SUM_PERIODIC)
    x0, y0, x1, x2, y2, x3 = (b.main(i) for i in range(6))
    x3n = b.main(5, 1)
    per = b.periodic_value(0)
    p0, p2 = x0 * y0, x2 * y2
    b.assert_zero(p0 + x1)            # lz_add_c
    b.assert_zero(p0 - x1)            # lz_sub_c
    b.assert_zero(p0 + p2)            # lz_add_g
    b.assert_zero(p0 - p2)            # lz_sub_g
    b.assert_zero(p2 - p0)
    b.assert_zero(-p0)                # lz_neg<0>
    b.assert_zero(-x1 + p2)           # lz_neg<1>: p - cell
    b.assert_zero(x3n * y0 + per)     # next row (wraps to row 0 on the last row), periodic column shorter than the trace
    b.assert_zero((x0 + x1) * (x2 - x3))
    b.assert_zero(((p0 + x1) - p2) + (-(x3 * x1)) - per * x3n)
    return dag.Air(b, name="sums")


def sums_case(n):
    t = np.zeros((n, 6), dtype=np.uint64)
    t[:, 0], t[:, 1] = _col(n, 0, 0), _col(n, 0, 1)
    t[:, 2] = _col(n, 31, 1)
    t[:, 3], t[:, 4] = _col(n, 50, 0), _col(n, 50, 1)
    t[:, 5] = _col(n, 90, 0)
    # rows with chosen fix-ups: (p0, x1, p2) as integers
    big, small = BIG_PAIRS[0], (1, 1)
    rows = [(big, P - 1, big),         # add_c wraps once; add_g: (2^64 - 1) + (2^64 - 1) wraps twice
            (small, P - 1, big),       # sub_c borrows; sub_g: 1 - (2^64 - 1) = 2 < eps borrows twice
            (big, 0xFFFFFFFF, small),  # p2 - p0 borrows twice the other way round
            (BIG_PAIRS[1], 2, BIG_PAIRS[2]), ((0, 0), 1, BIG_PAIRS[1])]
    for k, (pa, c, pb) in enumerate(rows):
        r = (n - 1 - k) if k < 2 else k  # the last two rows too: the next-row read there wraps
        t[r, 0], t[r, 1], t[r, 2], t[r, 3], t[r, 4] = pa[0], pa[1], c, pb[0], pb[1]
    return Case(sums_air(), t)


# ---- 4. the alpha fold ----------------------------------------------------------------------------------------------------------------
ALPHAS = [(1, 0), (P - 1, 0), (0xFFFFFFFEFFFFFFFF, 0xFFFFFFFEFFFFFFFF), ((1 << 22) - 1, 1 << 44), (0x9E3779B97F4A7C15 % P, 0xC2B2AE3D27D4EB4F % P)]
# (cell, cell) whose plain sum -- what lz_add_c hands the fold -- has both 32-bit halves at their maxima, and other corners
FOLD_SUMS = [(0xFFFFFFFF00000000, 0xFFFFFFFF), (0xFFFFFFFEFFFFFFFF, 0), (0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF), (P - 1, P - 1), (0, 0), (1, P - 1),
             (0xFFFFFFFF, 0xFFFFFFFF00000000), (1 << 63, (1 << 63) - 1)]


def fold_air(K):
    """K constraints C_k = main(2k) + main(2k+1) -- the sum reaches the fold unreduced --, the last two of K = 7 extension-valued."""
    n_ext = 2 if K >= 7 else 0
    b = dag.AirBuilder(2 * (K - n_ext), aux_width=2 * n_ext)
    for k in range(K - n_ext):
        b.assert_zero(b.main(2 * k) + b.main(2 * k + 1))
    for k in range(n_ext):
        b.assert_zero_ext(b.aux(2 * k) + b.aux(2 * k + 1))
    return dag.Air(b, name=f"fold{K}")


def fold_case(K, n):
    air = fold_air(K)
    w = air.main_width // 2
    t = np.zeros((n, 2 * w), dtype=np.uint64)
    for k in range(w):
        for r in range(n):
            t[r, 2 * k], t[r, 2 * k + 1] = FOLD_SUMS[(r + 3 * k) % len(FOLD_SUMS)]
    aux = None
    if air.aux_width:
        aux = np.zeros((n, 2 * air.aux_width), dtype=np.uint64)
        for k in range(air.aux_width // 2):
            for r in range(n):
                s0, s1 = FOLD_SUMS[(r + k) % len(FOLD_SUMS)], FOLD_SUMS[(r + 5 + k) % len(FOLD_SUMS)]
                aux[r, 4 * k], aux[r, 4 * k + 1], aux[r, 4 * k + 2], aux[r, 4 * k + 3] = s0[0], s1[0], s0[1], s1[1]
    return Case(air, t, aux)


# ---- 5. dot gates -----------------------------------------------------------------------------------------------------------------------
DOT_TERMS = (2, 3, 400, 401)  # 3: MH_JIT_DOT's threshold; 400: the largest dot; 401: the ordinary path
DOT_COLS = 201               # cells: columns x {this row, next row}
DOT_MAX_CELL = 0xFFFFFFFEFFFFFFFF
# coefficients: canonical values with maximal 22-bit limbs (fold_limbs cuts bits 0-21, 22-43, 44-63).  The top limb of a canonical value
# is at most 0xFFFFF; with it at 0xFFFFF and the upper word below 0xFFFFFFFF the largest value is 0xFFFFFFFEFFFFFFFF (limbs 0xFFFFF,
# 0x3FFBFF, 0x3FFFFF); 0xFFFFF7FFFFFFFFFF trades one bit of the top limb for a full middle limb (0xFFFF7, 0x3FFFFF, 0x3FFFFF).
DOT_COEFFS = [(0xFFFFFFFEFFFFFFFF, 0xFFFFF7FFFFFFFFFF), (0xFFFFF7FFFFFFFFFF, 0xFFFFFFFEFFFFFFFF)]
DOT_MAX_ROWS = (0, 1, 5)  # rows whose cells are all DOT_MAX_CELL (row 1 reads row 2 as its next row: see dot_case)


def dot_air(terms):
    """One EF constraint sum_i rnd_(i mod 2) * cell_i + rnd_0 * rnd_1 + aux_0: distinct cells, so every MUL node is single-use."""
    b = dag.AirBuilder(DOT_COLS, aux_width=1, num_randomness=2)
    cells = [b.main(i // 2, i % 2) for i in range(terms)]
    acc = b.randomness(0) * cells[0]
    for i in range(1, terms):
        acc = acc + b.randomness(i % 2) * cells[i]
    b.assert_zero_ext(acc + b.aux(0) + b.randomness(0) * b.randomness(1))
    return dag.Air(b, name=f"dot{terms}")


def dot_case(terms, n):
    t = np.zeros((n, DOT_COLS), dtype=np.uint64)
    for c in range(DOT_COLS):
        t[:, c] = _col(n, 7 * c, c % 2)
    for r in DOT_MAX_ROWS + (2, 6):  # rows 0, 1, 5 and the rows they read as their next ones (1, 2, 6)
        t[r, :] = DOT_MAX_CELL
    aux = np.stack([_col(n, 3, 0), _col(n, 3, 1)], axis=1)
    return Case(dot_air(terms), t, aux, rnd=DOT_COEFFS)


def dot_accumulators(case, terms, r):
    """The exact integers fold_limbs sums into the six accumulators of each EF component of the dot, on row r."""
    n = case.main.shape[0]
    out = []
    for comp in (0, 1):
        w = [0] * 6
        for i in range(terms):
            alpha = case.rnd[i % 2][comp]
            x = int(case.main[(r + i % 2) % n, i // 2])
            x0, x1 = x & 0xFFFFFFFF, x >> 32
            a0, a1, a2 = alpha & 0x3FFFFF, (alpha >> 22) & 0x3FFFFF, alpha >> 44
            for j, v in enumerate((a0 * x0, a1 * x0, a2 * x0, a0 * x1, a1 * x1, a2 * x1)):
                w[j] += v
        out.append(w)
    return out


# ---- 6. selectors ----------------------------------------------------------------------------------------------------------------------
def selector_air():
    b = dag.AirBuilder(2)
    x, y = b.main(0), b.main(1)
    b.assert_zero(b.is_first_row() * x)
    b.assert_zero(b.is_last_row() * y)
    b.assert_zero(b.is_transition() * (x * y))
    b.assert_zero(b.is_first_row() + b.is_last_row() * 2 + b.is_transition() * x)
    return dag.Air(b, name="selectors")


def selector_case(n):
    return Case(selector_air(), lattice_trace(n, 1)[:, :2].copy())


@functools.lru_cache(maxsize=None)
def expected(name, n, *args):
    """The constraint values [n][K] of a case under the fold's selector values, computed once per (case, height)."""
    import dag_eval
    c = CASES[name](*args, n)
    return dag_eval.constraint_values(c.air, c.main, c.aux, None, c.publics, c.rnd, c.avs, selectors=dag_eval.screen_selectors)


CASES = dict(single=single_product_case, lattice=lattice_case, ef=ef_case, sums=sums_case, fold=fold_case, dot=dot_case,
             selectors=selector_case)
