"""CPU-only: the operand table of tests/jit_corner_operands.py reaches every carry of the constraint kernels' asm product, in the table
and in every layout the GPU tests use (tests/fold_airs.py).  The model of the 13 instructions only chooses inputs; what it returns is
held to the plain product here, and nothing on the GPU side takes an expected value from it."""
import pytest
import jit_corner_operands as J
import fold_airs as F
import dag_eval

P = J.P
REACHED = J.FLAGS + ("bw&c3",)
UNREACHED = J.NEVER + ("cm&k2",)


def test_the_model_is_congruent_to_the_product():
    for a, b in J.PAIRS:
        assert 0 <= a < P and 0 <= b < P
        r, _ = J.mul_model(a, b)
        assert 0 <= r < 1 << 64 and r % P == a * b % P, (hex(a), hex(b))
    # ... and for any-representative operands (what the second level of a product lattice hands it)
    for a in J.EDGE:
        for b in J.EDGE:
            assert J.mul_model(a, b)[0] % P == a * b % P, (hex(a), hex(b))


def test_the_issue_pairs_reach_the_rare_links():
    flags = [J.mul_model(a, b)[1] for a, b in J.SEED_PAIRS]
    assert flags[0]["k2"] == 1
    assert flags[1]["bw"] == 1 and flags[1]["mk"] == 1
    assert flags[2]["bw"] == 1 and flags[2]["c3"] == 1 and flags[2]["mk"] == 0
    assert all(p in J.PAIRS for p in J.SEED_PAIRS)


def test_table_reaches_every_carry_and_never_the_dropped_ones():
    cov = J.coverage(J.PAIRS)
    print("PAIRS:", len(J.PAIRS), "pairs;", cov)
    for k in REACHED:
        assert cov[k] >= 1, k
    for k in UNREACHED:
        assert cov[k] == 0, k  # the asm drops d4 / d5 and ORs cm with k2: it relies on this
    assert len(J.PAIRS) <= 256  # one 2^8-row trace shows a gate the whole table
    assert J.covers(J.small_cover(8))


def test_every_value_is_structured():
    """EDGE, 2^i + d or 2^i +- 2^j + d with d in {-1, 0, 1}: nothing in the table is an unexplained constant."""
    cand = set(J._candidates())
    for a, b in J.PAIRS:
        assert a in cand and b in cand, (hex(a), hex(b))


@pytest.mark.parametrize("n", F.HEIGHTS)
@pytest.mark.parametrize("name", ["single", "lattice"])
def test_every_cell_product_gate_of_a_layout_sees_every_carry(name, n):
    """The gates whose operands are both trace cells receive exactly what the trace holds.  (A product of products receives whichever
    representatives the first level returned; those gates are driven, but their carries cannot be dictated.)"""
    c = F.CASES[name](n)
    gates = F.cell_products(c.air, c.main)
    assert len(gates) == {"single": 1, "lattice": F.LATTICE_PAIRS}[name]
    for g, pairs in gates.items():
        cov = J.coverage(pairs)
        print(name, n, "gate", g, cov)
        for k in REACHED:
            assert cov[k] >= 1, (name, n, g, k)
        for k in UNREACHED:
            assert cov[k] == 0, (name, n, g, k)


@pytest.mark.parametrize("n", F.HEIGHTS)
def test_extension_layout_sees_every_carry_in_its_base_products(n):
    """e0 * e1: the products a0 b0 and a1 b1 are table pairs; e2 * m0: c0 * m0 is one."""
    c = F.ef_case(n)
    for ca, cb, src in ((0, 2, c.aux), (1, 3, c.aux)):
        assert J.covers([(int(src[r, ca]), int(src[r, cb])) for r in range(n)])
    assert J.covers([(int(c.aux[r, 4]), int(c.main[r, 0])) for r in range(n)])


@pytest.mark.parametrize("n", F.HEIGHTS)
def test_sums_layout_fires_single_and_double_fixups(n):
    """Integers, no model: a product below 2^64 is returned as it is (hi = 0: nothing to reduce), so rows holding BIG_PAIRS put values
    in [p, 2^64) behind the additions.  lz_add_g wraps twice iff a + b - 2^64 + eps >= 2^64; lz_sub_g iff a - b + 2^64 < eps."""
    c = F.sums_case(n)
    M, EPS = 1 << 64, 0xFFFFFFFF
    seen = set()
    for r in range(n):
        x0, y0, x1, x2, y2 = (int(c.main[r, i]) for i in range(5))
        if x0 * y0 >= M or x2 * y2 >= M:
            continue  # representative not known without a model: not counted
        p0, p2 = x0 * y0, x2 * y2
        if p0 + x1 >= M: seen.add("add_c")
        if p0 < x1: seen.add("sub_c")
        if p0 + p2 >= M:
            seen.add("add_g")
            if p0 + p2 - M + EPS >= M: seen.add("add_g twice")
        if p0 < p2:
            seen.add("sub_g")
            if p0 - p2 + M < EPS: seen.add("sub_g twice")
        if p2 < p0 and p2 - p0 + M < EPS: seen.add("sub_g twice, reversed")
        if p0 >= P: seen.add("neg of a value >= p")
    print(sorted(seen))
    assert seen == {"add_c", "sub_c", "add_g", "add_g twice", "sub_g", "sub_g twice", "sub_g twice, reversed", "neg of a value >= p"}
    assert len(F.SUM_PERIODIC[0]) < n


def test_fold_inputs_have_both_halves_at_their_maxima():
    """C_k = cell + cell reaches fold_limbs as the plain sum when it does not wrap: 0xFFFFFFFF00000000 + 0xFFFFFFFF = 2^64 - 1."""
    assert any(a + b == (1 << 64) - 1 for a, b in F.FOLD_SUMS)
    assert all(a < P and b < P for a, b in F.FOLD_SUMS)
    for K in (1, 2, 7):
        c = F.fold_case(K, 8)
        assert len(dag_eval.parse(c.air.blob)[2]) == K


def test_dot_accumulators_at_the_400_term_bound():
    """The generator keeps a dot to <= 400 terms because each of its six accumulators sums products below 2^54 in a plain u64.  The
    400-term case's inputs reach that bound: on the rows whose cells are all 0xFFFFFFFEFFFFFFFF the exact integer sums of w0, w1, w3, w4
    (limbs 0 and 1 of the coefficient against either half of the cell) exceed 2^62 and every sum stays below 2^64.
    w2 and w5 cannot exceed 2^62 for ANY admissible input: the top limb of a canonical coefficient is alpha >> 44 <= 0xFFFFF < 2^20
    (randomness is canonicalised on entry), a half is < 2^32, so 400 terms stay below 400 * 2^52 < 2^61.  They are held to that ceiling
    instead: with the largest top limb and the largest halves on every term they come within 2^-17 of it (the two coefficients' top limbs are 0xFFFFF and 0xFFFF7)."""
    terms = 400
    for n in F.HEIGHTS:
        c = F.dot_case(terms, n)
        for comp in (0, 1):
            assert all(v[comp] < P for v in c.rnd)
        for r in F.DOT_MAX_ROWS:
            for comp, w in enumerate(F.dot_accumulators(c, terms, r)):
                print(n, r, comp, [f"2^{v.bit_length() - 1}+" for v in w])
                assert all(v < 1 << 64 for v in w)
                for j in (0, 1, 3, 4):
                    assert w[j] > 1 << 62, (n, r, comp, j)
                ceiling = terms * 0xFFFFF * 0xFFFFFFFF
                for j in (2, 5):
                    assert ceiling * (1 - 2 ** -17) <= w[j] <= ceiling < 1 << 61, (n, r, comp, j)
    # one more term would still fit a u64 (401 * 2^54 < 2^64): the bound is the generator's, and 401 terms must not form one dot
    assert 401 * (1 << 54) < 1 << 64


@pytest.mark.parametrize("log_n", [4, 8])
def test_lookup_corner_challenges_leave_no_zero_denominator(log_n):
    """tests/test_gpu_lookup.py runs the compiled lookup program on a trace of corner operands under challenges with corner components:
    the CPU oracle must build that aux trace (it refuses a zero denominator), the buses balance on the valid variant, and no denominator
    of the program vanishes over Python integers either."""
    import airs as A
    import oracle_binding as ob
    _, lookup = A.logup_air()
    for valid in (True, False):
        main = A.logup_corner_trace(log_n, valid=valid)
        assert (main < P).all()
        for rnd in A.LOGUP_CORNER_CHALLENGES:
            assert all(0 <= x < P for c in rnd for x in c)
            _, fin = ob.lookup_build_aux(lookup, main, rnd)
            assert (int(fin[0]), int(fin[1])) == (0, 0) or not valid
            (r00, r01), (r10, r11) = rnd
            n = main.shape[0]
            for r in range(n):
                v, t, _, a, b, c, _, f = (int(x) for x in main[r])
                e_next = int(main[(r + 1) % n, 6])
                # dV, dT = r0 + x + 3 r1; dA, dB = r0 + r1 + x; dC = r0 + 7 r1 + x; dEn, dF = r0 + 5 r1 + x (tests/airs.py logup_air)
                for x, k in ((v, 3), (t, 3), (a, 1), (b, 1), (c, 7), (e_next, 5), (f, 5)):
                    assert ((r00 + x + k * r10) % P, (r01 + k * r11) % P) != (0, 0), (log_n, rnd, r)
