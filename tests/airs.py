"""Small test AIRs (constraints as DAG blobs + trace/aux generators) exercising every builder input:
two-row windows, selectors, public values, periodic columns, EF aux columns, randomness, aux values,
base and extension constraints, and different per-AIR quotient degrees.  They play the role of the
reference's tiny test AIRs (crates/lifted-stark/src/testing/test_tiny_air.rs:177-410,
test_per_air_degree.rs, test_multi_aux_alignment.rs)."""
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import dag  # noqa: E402

P = dag.P


def emul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def eadd(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


# ------------------------------------------------------------------------------------------------
def fib_air():
    """2 main columns (a, b): a' = b, b' = a + b; boundary values are public inputs.
    Aux (1 EF column): running product p' = p * (r0 + a) with p[0] = 1; aux value = p_last*(r0+a_last)."""
    b = dag.AirBuilder(2, aux_width=1, num_randomness=1, num_aux_values=1, num_public=3)
    a0, b0, a1, b1 = b.main(0), b.main(1), b.main(0, 1), b.main(1, 1)
    tr = b.is_transition()
    b.assert_zero(tr * (a1 - b0))
    b.assert_zero(tr * (b1 - (a0 + b0)))
    b.assert_zero(b.is_first_row() * (a0 - b.public(0)))
    b.assert_zero(b.is_first_row() * (b0 - b.public(1)))
    b.assert_zero(b.is_last_row() * (b0 - b.public(2)))
    p0, p1, r = b.aux(0), b.aux(0, 1), b.randomness(0)
    b.assert_zero_ext(b.is_first_row() * (p0 - 1))
    b.assert_zero_ext(tr * (p1 - p0 * (r + a0)))
    b.assert_zero_ext(b.is_last_row() * (p0 * (r + a0) - b.aux_value(0)))

    def build_aux(main, randomness):
        n = main.shape[0]
        r = randomness[0]
        aux = np.zeros((n, 2), dtype=np.uint64)
        p = (1, 0)
        for i in range(n):
            aux[i] = p
            p = emul(p, eadd(r, (int(main[i, 0]), 0)))
        return aux, [p[0], p[1]]

    return dag.Air(b, build_aux, "fib")


def fib_trace(log_n, a=1, b_=1):
    n = 1 << log_n
    t = np.zeros((n, 2), dtype=np.uint64)
    x, y = a % P, b_ % P
    for i in range(n):
        t[i] = (x, y)
        x, y = y, (x + y) % P
    return t, [a % P, b_ % P, int(t[n - 1, 1])]


# ------------------------------------------------------------------------------------------------
PERIODIC_COLS = ([3, 5, 7, 11], [2, 9, 4, 6, 1, 8, 13, 12])


def periodic_air(num_public=3):
    """1 working column c (+ 2 free columns): c' = c^2 * k1 + k2 with periodic k1 (period 4), k2 (period 8).
    Degree 3 -> 2 quotient chunks.  2 EF aux columns: s' = s + r0*c (running sum), t = constant r1."""
    b = dag.AirBuilder(3, aux_width=2, num_randomness=2, num_aux_values=2, num_public=num_public, periodic=PERIODIC_COLS)
    c0, c1 = b.main(0), b.main(0, 1)
    tr = b.is_transition()
    b.assert_zero(tr * (c1 - (c0 * c0 * b.periodic_value(0) + b.periodic_value(1))))
    b.assert_zero(b.main(1) * b.main(2) - b.main(1) * b.main(2))  # trivially zero, keeps columns live
    s0, s1, t0, t1 = b.aux(0), b.aux(0, 1), b.aux(1), b.aux(1, 1)
    r0, r1 = b.randomness(0), b.randomness(1)
    b.assert_zero_ext(tr * (s1 - (s0 + r0 * c0)))
    b.assert_zero_ext(b.is_first_row() * s0)
    b.assert_zero_ext(t0 - r1)
    b.assert_zero_ext(tr * (t1 - t0))
    b.assert_zero_ext(b.is_last_row() * (s0 + r0 * c0 - b.aux_value(0)))
    b.assert_zero_ext(b.aux_value(1) - r1)

    def build_aux(main, randomness):
        n = main.shape[0]
        r0, r1 = randomness[0], randomness[1]
        aux = np.zeros((n, 4), dtype=np.uint64)
        s = (0, 0)
        for i in range(n):
            aux[i, 0:2] = s
            aux[i, 2:4] = r1
            s = eadd(s, emul(r0, (int(main[i, 0]), 0)))
        return aux, [s[0], s[1], r1[0], r1[1]]

    return dag.Air(b, build_aux, "periodic")


def periodic_trace(log_n, seed=5):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    t = rng.integers(0, P, (n, 3), dtype=np.uint64)
    c = 7
    for i in range(n):
        t[i, 0] = c
        c = (c * c * PERIODIC_COLS[0][i % 4] + PERIODIC_COLS[1][i % 8]) % P
    return t


# ------------------------------------------------------------------------------------------------
def dummy_trace(log_n, width, seed=1):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, P, (1 << log_n, width), dtype=np.uint64)
    t[:, 0] = 0
    return t


# ------------------------------------------------------------------------------------------------
def synthetic_big_air(width=51, aux_width=8, n_constraints=300, terms=3, seed=11, num_public=0):
    """A Miden-SIZED constraint system (thousands of gates, hundreds of constraints, degree <= 9, two-row
    window, aux columns + randomness) for exercising the DAG interpreter at the scale of the real AIRs
    (~5.2 k gates over the three Miden AIRs, air/src/snapshots/*relation_digest*.snap).  The constraints
    are random polynomials, so a random trace does NOT satisfy them: proofs are still deterministic and
    must be bit-identical between the oracle and the GPU, but no verifier accepts them."""
    rng = np.random.default_rng(seed)
    b = dag.AirBuilder(width, aux_width=aux_width, num_randomness=2, num_aux_values=aux_width, num_public=num_public)
    for k in range(n_constraints):
        acc = None
        for _ in range(terms):
            deg = int(rng.integers(2, 9))
            cols = rng.integers(0, width, deg)
            rows = rng.integers(0, 2, deg)
            t = b.main(int(cols[0]), int(rows[0]))
            for c, r in zip(cols[1:], rows[1:]):
                t = t * b.main(int(c), int(r)) if rng.random() < 0.7 else t * (b.main(int(c), int(r)) + int(rng.integers(1, 1000)))
            acc = t if acc is None else (acc + t if rng.random() < 0.5 else acc - t)
        if k % 5 == 0:  # every fifth constraint is extension-valued
            a = b.aux(int(rng.integers(0, aux_width)), int(rng.integers(0, 2)))
            e = a * (b.randomness(0) + b.main(int(rng.integers(0, width)))) - b.aux(int(rng.integers(0, aux_width)), 1) * b.randomness(1)
            b.assert_zero_ext(b.is_transition() * e + acc * 0 + acc)
        else:
            b.assert_zero(b.is_transition() * acc if rng.random() < 0.5 else acc)
    return dag.Air(b, build_aux=None, name=f"synthetic:{width}:{aux_width}:{n_constraints}")


# ------------------------------------------------------------------------------------------------
LOGUP_PERIODIC = ([1, 0, 0, 1, 1, 0, 1, 0],)


def logup_air():
    """A LogUp AIR in the reference's shape (air/src/lookup/aux_builder.rs): aux column 0 = running-sum accumulator,
    aux column 1 = a per-row fraction column, one aux value = the accumulator's final.  Main columns
    V, T, M, A, B, C, E, F:  bus 0 looks V up in table T with multiplicities M, bus 1 is a permutation A ~ B
    (B = A shuffled across rows); two pairs that cancel inside every row exercise next-row reads (E_next vs F,
    F[r] = E[r+1]) and a periodic multiplicity (zero on some rows: those fractions are skipped).
    Returns (Air, Lookup): the constraint DAG and the lookup program exported from the same definitions."""
    def denoms(b):
        r0, r1 = b.randomness(0), b.randomness(1)
        V, T, M, A_, B_, C_, F = b.main(0), b.main(1), b.main(2), b.main(3), b.main(4), b.main(5), b.main(7)
        E_next = b.main(6, 1)
        return dict(dV=r0 + V + r1 * 3, dT=r0 + T + r1 * 3, dA=r0 + r1 + A_, dB=r0 + r1 + B_, dC=r0 + r1 * 7 + C_,
                    dEn=r0 + r1 * 5 + E_next, dF=r0 + r1 * 5 + F, M=M)

    b = dag.AirBuilder(8, aux_width=2, num_randomness=2, num_aux_values=1, num_public=0, periodic=LOGUP_PERIODIC)
    d = denoms(b)
    acc, acc_next, f1 = b.aux(0), b.aux(0, 1), b.aux(1)
    b.assert_zero_ext(f1 * d["dA"] * d["dB"] - (d["dB"] - d["dA"]))
    own = d["dT"] - d["M"] * d["dV"]  # numerator of 1/dV - M/dT over dV*dT
    b.assert_zero_ext(b.is_transition() * ((acc_next - acc - f1) * d["dV"] * d["dT"] - own))
    b.assert_zero_ext(b.is_first_row() * acc)
    b.assert_zero_ext(b.is_last_row() * ((b.aux_value(0) - acc - f1) * d["dV"] * d["dT"] - own))

    lb = dag.LookupBuilder(8, num_cols=2, num_randomness=2, periodic=LOGUP_PERIODIC)
    d = denoms(lb)
    per = lb.periodic_value(0)
    lb.fraction(0, 1, d["dV"])
    lb.fraction(0, -d["M"], d["dT"])
    lb.fraction(0, 1, d["dEn"])
    lb.fraction(0, P - 1, d["dF"])
    lb.fraction(1, 1, d["dA"])
    lb.fraction(1, lb.const(P - 1), d["dB"])
    lb.fraction(1, per, d["dC"])
    lb.fraction(1, -per, d["dC"])
    lookup = dag.Lookup(lb, "logup")

    def build_aux(main, randomness):
        import oracle_binding as ob
        aux, fin = ob.lookup_build_aux(lookup, main, randomness)
        return aux, [int(fin[0]), int(fin[1])]

    return dag.Air(b, build_aux, "logup"), lookup


def logup_trace(log_n, seed=3, valid=True):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 8), dtype=np.uint64)
    table = rng.integers(0, P, n, dtype=np.uint64)
    picks = rng.integers(0, n, n)
    t[:, 0] = table[picks]
    t[:, 1] = table
    t[:, 2] = np.bincount(picks, minlength=n).astype(np.uint64)
    t[:, 3] = rng.integers(0, P, n, dtype=np.uint64)
    t[:, 4] = rng.permutation(t[:, 3])
    t[:, 5] = rng.integers(0, P, n, dtype=np.uint64)
    t[:, 6] = rng.integers(0, P, n, dtype=np.uint64)
    t[:, 7] = np.roll(t[:, 6], -1)
    if not valid:
        t[n // 2, 0] = (int(t[n // 2, 0]) + 1) % P  # a value that is not in the table: the buses no longer balance
    return t


# challenges with corner components for logup_corner_trace (tests/test_jit_corner_operands.py checks on the CPU that no denominator
# vanishes under them)
LOGUP_CORNER_CHALLENGES = [[(P - 1, 0xFFFFFFFEFFFFFFFF), ((1 << 32) - 1, 1 << 32)],
                           [(0xFFFFFFFEFFFFFFFF, 1), (P - 1, P - 1)],
                           [(1 << 32, (1 << 32) - 1), (0xFFFFFFFEFFFFFFFF, 0xFFFFFFFEFFFFFFFF)]]


def logup_corner_trace(log_n, valid=True):
    """logup_trace's structure (V looked up in T with multiplicities M, B a permutation of A, F[r] = E[r+1]) with every value column
    filled from the corner operand table of tests/jit_corner_operands.py: the compiled lookup program's products and sums see the
    operands that reach the rare carries of the asm product."""
    import jit_corner_operands as J
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    col = lambda shift, which: np.array(J.column_values(n, shift, which), dtype=np.uint64)
    t = np.zeros((n, 8), dtype=np.uint64)
    table = col(0, 0)
    picks = rng.integers(0, n, n)
    t[:, 0] = table[picks]
    t[:, 1] = table
    t[:, 2] = np.bincount(picks, minlength=n).astype(np.uint64)
    t[:, 3] = col(0, 1)
    t[:, 4] = rng.permutation(t[:, 3])
    t[:, 5] = col(37, 0)
    t[:, 6] = col(59, 1)
    t[:, 7] = np.roll(t[:, 6], -1)
    if not valid:
        t[n // 2, 0] = (int(t[n // 2, 0]) + 1) % P
    return t


# ------------------------------------------------------------------------------------------------
def prep_air(log_n, seed=13, num_public=0):
    """An AIR with PREPROCESSED columns (fixed circuit data committed at setup, crates/lifted-stark/src/preprocessed.rs):
    S (a 0/1 selector) and T (a table).  Main columns a, c, d:  a' = S ? a + T : a * c  (degree 3 with the selector),
    d = T_next (reads the preprocessed column's next row).  One all-zero EF aux column (the protocol wants one)."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    S = rng.integers(0, 2, n, dtype=np.uint64)
    T = rng.integers(0, P, n, dtype=np.uint64)
    b = dag.AirBuilder(3, aux_width=1, num_randomness=1, num_aux_values=0, num_public=num_public, preprocessed_width=2)
    a0, a1, c0, d0 = b.main(0), b.main(0, 1), b.main(1), b.main(2)
    s, t, t_next = b.preprocessed(0), b.preprocessed(1), b.preprocessed(1, 1)
    b.assert_zero(b.is_transition() * (s * (a1 - a0 - t) + (b.const(1) - s) * (a1 - a0 * c0)))
    b.assert_zero(d0 - t_next)
    b.assert_zero_ext(b.aux(0) * b.randomness(0))  # aux column is zero
    air = dag.Air(b, build_aux=None, name=f"prep:{log_n}", preprocessed=np.stack([S, T], axis=1))

    def trace(seed2=17):
        r2 = np.random.default_rng(seed2)
        m = np.zeros((n, 3), dtype=np.uint64)
        m[:, 1] = r2.integers(0, P, n, dtype=np.uint64)
        a = 5
        for r in range(n):
            m[r, 0] = a
            m[r, 2] = T[(r + 1) % n]
            a = (a + int(T[r])) % P if S[r] else (a * int(m[r, 1])) % P
        return m

    return air, trace


# ------------------------------------------------------------------------------------------------
def random_air(seed, width=6, aux_width=2, n_constraints=12, max_degree=4, with_preprocessed=False, log_n=None):
    """A random constraint system touching EVERY node kind in random base/extension mixtures (main / aux / periodic /
    public / selector / randomness / aux-value / preprocessed leaves; ADD, SUB, MUL, NEG over base-base, base-ext, ext-base
    and ext-ext operands).  Like synthetic_big_air the constraints are not satisfied by a random trace: proofs are
    deterministic and must be bit-identical between the oracle, the interpreter and the compiled kernels."""
    rng = np.random.default_rng(seed)
    pw = 2 if with_preprocessed else 0
    b = dag.AirBuilder(width, aux_width=aux_width, num_randomness=2, num_aux_values=2, num_public=2, periodic=PERIODIC_COLS,
                       preprocessed_width=pw)

    def leaf():
        k = int(rng.integers(0, 10 if with_preprocessed else 9))
        if k == 0:
            return b.main(int(rng.integers(0, width)), int(rng.integers(0, 2)))
        if k == 1:
            return b.aux(int(rng.integers(0, aux_width)), int(rng.integers(0, 2)))
        if k == 2:
            return b.periodic_value(int(rng.integers(0, 2)))
        if k == 3:
            return b.public(int(rng.integers(0, 2)))
        if k == 4:
            return [b.is_first_row, b.is_last_row, b.is_transition][int(rng.integers(0, 3))]()
        if k == 5:
            return b.randomness(int(rng.integers(0, 2)))
        if k == 6:
            return b.aux_value(int(rng.integers(0, 2)))
        if k == 7:
            return b.const(int(rng.integers(0, P, dtype=np.uint64)))
        if k == 8:
            return b.main(int(rng.integers(0, width)))
        return b.preprocessed(int(rng.integers(0, pw)), int(rng.integers(0, 2)))

    def expr(depth):
        if depth == 0 or rng.random() < 0.25:
            return leaf()
        op = int(rng.integers(0, 4))
        x = expr(depth - 1)
        if op == 3:
            return -x
        y = expr(depth - 1)
        if op == 0:
            return x + y
        if op == 1:
            return x - y
        return x * y if x.deg + y.deg <= max_degree else x + y

    for _ in range(n_constraints):
        e = expr(4)
        (b.assert_zero_ext if e.ext else b.assert_zero)(e)

    def build_aux(main, randomness):
        n = main.shape[0]
        r2 = np.random.default_rng(seed + 1000)
        return r2.integers(0, P, (n, 2 * aux_width), dtype=np.uint64), [int(x) for x in r2.integers(0, P, 4, dtype=np.uint64)]

    prep = None
    if with_preprocessed:
        prep = np.random.default_rng(seed + 2000).integers(0, P, (1 << log_n, pw), dtype=np.uint64)
    return dag.Air(b, build_aux, f"random:{seed}", preprocessed=prep)


# ------------------------------------------------------------------------------------------------
def range_air(log_n, seed=23):
    """A table lookup, the canonical LogUp + preprocessed pairing: the table T is a PREPROCESSED column (fixed circuit
    data), the main trace holds looked-up values V (each in T) and the multiplicities M; the bus
    sum_r 1/(alpha + V_r) - M_r/(alpha + T_r) balances iff every V is in the table.
    Returns (Air, Lookup, trace_fn): constraint DAG, lookup program (it reads the preprocessed column), trace builder."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    table = rng.permutation(np.arange(1, 4 * n, 4, dtype=np.uint64))[:n]  # n distinct values

    def denoms(b):
        r0, r1 = b.randomness(0), b.randomness(1)
        return r0 + b.main(0) + r1 * 2, r0 + b.preprocessed(0) + r1 * 2, b.main(1)

    b = dag.AirBuilder(2, aux_width=1, num_randomness=2, num_aux_values=1, preprocessed_width=1)
    dV, dT, M = denoms(b)
    acc, acc_next = b.aux(0), b.aux(0, 1)
    own = dT - M * dV
    b.assert_zero_ext(b.is_transition() * ((acc_next - acc) * dV * dT - own))
    b.assert_zero_ext(b.is_first_row() * acc)
    b.assert_zero_ext(b.is_last_row() * ((b.aux_value(0) - acc) * dV * dT - own))
    lb = dag.LookupBuilder(2, num_cols=1, num_randomness=2, preprocessed_width=1)
    dV, dT, M = denoms(lb)
    lb.fraction(0, 1, dV)
    lb.fraction(0, -M, dT)
    lookup = dag.Lookup(lb, "range")
    prep = table.reshape(n, 1)

    def build_aux(main, randomness):
        import oracle_binding as ob
        aux, fin = ob.lookup_build_aux(lookup, main, randomness, preprocessed=prep)
        return aux, [int(fin[0]), int(fin[1])]

    def trace(seed2=29, valid=True):
        r2 = np.random.default_rng(seed2)
        picks = r2.integers(0, n, n)
        m = np.zeros((n, 2), dtype=np.uint64)
        m[:, 0] = table[picks]
        m[:, 1] = np.bincount(picks, minlength=n).astype(np.uint64)
        if not valid:
            m[3, 0] = 2  # not in the table (all entries are 1 mod 4)
        return m

    return dag.Air(b, build_aux, f"range:{log_n}", preprocessed=prep), lookup, trace


# ------------------------------------------------------------------------------------------------
def bus_air(sign, extra_cols=0, tag=3):
    """One side of a CROSS-AIR LogUp bus (precompiles-prover/src/session/prove.rs: twelve chiplet AIRs whose sigma finals must
    sum to zero, closed by MultiAir::eval_external).  Main column 0 = the message; aux column 0 = the running sum of
    sign / (r0 + tag * r1 + V), its final the AIR's one aux value.  The per-row constraints hold for ANY trace; whether the
    senders' and receivers' multisets agree is visible only in the sum of the finals over the AIRs.
    Returns (Air, Lookup)."""
    w = 1 + extra_cols
    s = sign % P

    def denom(b):
        return b.randomness(0) + b.randomness(1) * tag + b.main(0)

    b = dag.AirBuilder(w, aux_width=1, num_randomness=2, num_aux_values=1, num_public=0)
    d = denom(b)
    acc, acc_next = b.aux(0), b.aux(0, 1)
    b.assert_zero_ext(b.is_transition() * ((acc_next - acc) * d - s))
    b.assert_zero_ext(b.is_first_row() * acc)
    b.assert_zero_ext(b.is_last_row() * ((b.aux_value(0) - acc) * d - s))
    for c in range(1, w):  # filler columns take part in a constraint so that they are live
        b.assert_zero(b.main(c) * b.main(c) - b.main(c) * b.main(c))
    lb = dag.LookupBuilder(w, num_cols=1, num_randomness=2)
    lb.fraction(0, lb.const(s), denom(lb))
    lookup = dag.Lookup(lb, f"bus{sign:+d}")

    def build_aux(main, randomness):
        import oracle_binding as ob
        aux, fin = ob.lookup_build_aux(lookup, main, randomness)
        return aux, [int(fin[0]), int(fin[1])]

    return dag.Air(b, build_aux, f"bus{sign:+d}:{w}"), lookup


def bus_traces(log_n, extra_cols=(0, 0, 0), seed=23, valid=True):
    """A sender of 2^log_n messages and two receivers of half of them each (in shuffled order)."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    msgs = rng.integers(0, P, n, dtype=np.uint64)
    perm = rng.permutation(n)
    out = []
    for k, part in enumerate((msgs, msgs[perm[:n // 2]], msgs[perm[n // 2:]])):
        t = rng.integers(0, P, (part.size, 1 + extra_cols[k]), dtype=np.uint64)
        t[:, 0] = part
        out.append(t)
    if not valid:
        out[2][3, 0] = (int(out[2][3, 0]) + 1) % P
    return out


def chiplet_stack_statement(log_bus=9):
    """Twelve heterogeneous instances in the shape of precompiles-prover/src/session/prove.rs (ChipletAir): a cross-AIR
    LogUp bus (sender + two receivers of half its height), three AIRs with preprocessed columns, three without aux columns,
    three wide DummyMidenAir fillers; heights 2^4 .. 2^log_bus.  Returns (airs, traces, {instance index: Lookup})."""
    import oracle_binding as ob  # noqa: F401
    from test_external_assertions import no_aux_air, no_aux_trace
    bus = [bus_air(+1), bus_air(-1, 1), bus_air(-1, 2)]
    preps = [prep_air(5, seed=31), prep_air(7, seed=32), prep_air(4, seed=33)]
    airs_ = [bus[0][0], preps[0][0], no_aux_air(), dag.dummy_miden_air(9, 1), bus[1][0], preps[1][0], no_aux_air(),
             dag.dummy_miden_air(21, 3), bus[2][0], preps[2][0], no_aux_air(), dag.dummy_miden_air(12, 2)]
    bt = bus_traces(log_bus, (0, 1, 2))
    traces = [bt[0], preps[0][1](), no_aux_trace(6), dummy_trace(8, 9), bt[1], preps[1][1](), no_aux_trace(4, seed=5),
              dummy_trace(5, 21), bt[2], preps[2][1](), no_aux_trace(log_bus, seed=6), dummy_trace(7, 12)]
    return airs_, traces, {0: bus[0][1], 4: bus[1][1], 8: bus[2][1]}
