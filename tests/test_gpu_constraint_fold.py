"""GPU (run with -m gpu): the constraint programs on chosen operands, read back through mh_constraint_fold (csrc/check.hip).

The entry runs an AIR's own constraint program -- the compiled chunks of csrc/air_jit.cpp or the interpreter k_eval_quotient -- on the raw
trace, so a test dictates the operands of every gate: the rows hold the corner table of tests/jit_corner_operands.py, which reaches the
carries of the asm product that random field elements reach with probability ~2^-32 (k2, bw, c3, mk; tests/test_jit_corner_operands.py
proves the coverage on the CPU).  Expected values come from tests/dag_eval.py (the DAG over Python integers) and are compared for exact
equality of canonical felts, under MH_JIT=0 and MH_JIT=1, at 2^8 rows (one full 256-row tile) and 2^3 rows (below the height at which a
fused program runs compiled).

What these tests cannot do: the powers of a caller's alpha beyond the five chosen ones are not controllable, so SATURATING the fold's limb
accumulators stays with tests/test_jit_prelude_arith.py::test_fold_accumulators (400 terms of maximal operands, CPU build of the same
text); and the operands on the LDE domain of a proof are whatever the LDE makes them -- only the trace domain is dictated here."""
import os
import re
import numpy as np
import pytest
import dag_eval
import fold_airs as F
from __graft_entry__ import load_package
from test_gpu_check_constraints import device_air

pytestmark = pytest.mark.gpu
P = F.P
# generator switches (case 7): the stage-interleaved lz_mulN<2|3|4>, the canonicalising gl_mul, the limb-by-limb fold_value
SWITCHES = {"mulgroup4": {"MH_JIT_MULGROUP": "4"}, "lazyval0": {"MH_JIT_LAZYVAL": "0"}, "foldv0": {"MH_JIT_FLAGS": "-DMH_JIT_FOLDV=0"}}


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def fold_pairs(out):
    return [(int(a), int(b)) for a, b in out]


def check_case(ctx, name, args, n, alphas, jits=("0", "1")):
    """The fold of case `name` at height n equals the Python-integer fold for every alpha, under every MH_JIT setting in `jits`."""
    pkg = load_package()
    case = F.CASES[name](*args, n)
    values = F.expected(name, n, *args)
    for jit in jits:
        d = device_air(ctx, case.air, jit)
        assert (d.compiled_chunks > 0) == (jit == "1"), (name, args, n, jit)
        for alpha in alphas:
            got = fold_pairs(pkg.constraint_fold(ctx, d, case.main, alpha=alpha, **case.kwargs()))
            exp = dag_eval.alpha_fold(values, alpha)
            bad = [r for r in range(n) if got[r] != exp[r]]
            assert not bad, f"{name}{args} n={n} MH_JIT={jit} alpha={alpha}: row {bad[0]}: got {got[bad[0]]}, expected {exp[bad[0]]} ({len(bad)} rows differ)"
        d.free()


# ---- 1. product lattice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.HEIGHTS)
def test_one_product_read_back_unmixed(ctx, n):
    """K = 1, alpha = (1, 0), z = 0: F(r) is x * y itself, compared with a * b % p directly."""
    pkg = load_package()
    case = F.single_product_case(n)
    exp = [(int(case.main[r, 0]) * int(case.main[r, 1]) % P, 0) for r in range(n)]
    for jit in ("0", "1"):
        d = device_air(ctx, case.air, jit)
        assert fold_pairs(pkg.constraint_fold(ctx, d, case.main, alpha=(1, 0))) == exp, jit
    check_case(ctx, "single", (), n, F.ALPHAS)


@pytest.mark.parametrize("n", F.HEIGHTS)
def test_product_lattice(ctx, n):
    """Thirteen products on three levels (the upper ones take any-representative operands), every constraint mixed by corner alphas."""
    check_case(ctx, "lattice", (), n, F.ALPHAS)


# ---- 2. extension products -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.HEIGHTS)
def test_extension_products(ctx, n):
    """EF x EF (the interpreter's and gl-form's cross term multiplies sums of two corner components), EF x base, products of products,
    randomness and aux values with corner components."""
    check_case(ctx, "ef", (), n, F.ALPHAS[:3])


# ---- 3. sums, differences, negations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.HEIGHTS)
def test_sums_differences_negations_of_lazy_values(ctx, n):
    """lz_add_c / _g, lz_sub_c / _g, lz_neg<0|1> behind products in [p, 2^64) (single and double fix-ups: test_jit_corner_operands),
    a next-row read on the last row, a periodic column of length 4."""
    check_case(ctx, "sums", (), n, F.ALPHAS[:3])


# ---- 4. the alpha fold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 7])
def test_alpha_fold(ctx, K):
    """K constraints whose values reach fold_limbs with both 32-bit halves at 0xFFFFFFFF, folded with alpha in {(1, 0), (p-1, 0),
    (0xFFFFFFFEFFFFFFFF, 0xFFFFFFFEFFFFFFFF), (2^22 - 1, 2^44), a fixed arbitrary one}.  Only alpha itself is chosen: its powers are what
    they are, so the limb accumulators are not saturated here -- that is test_jit_prelude_arith.py::test_fold_accumulators' job (400 terms)."""
    for n in F.HEIGHTS:
        check_case(ctx, "fold", (K,), n, F.ALPHAS)


# ---- 5. dot gates ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", F.DOT_TERMS)
def test_dot_gates_at_their_bounds(ctx, terms):
    """sum_i rnd_i * cell_i + aux + rnd_0 rnd_1 with 2 terms (below MH_JIT_DOT's threshold: ordinary gates), 3 (the smallest dot), 400 (the
    largest: four of its six accumulators pass 2^62 on the rows of maximal cells, test_jit_corner_operands) and 401 (no single dot may
    take them: the generator makes a 400-term dot of the inner sum and adds the last term as an ordinary gate)."""
    for n in F.HEIGHTS:
        check_case(ctx, "dot", (terms,), n, F.ALPHAS[2:3])


# ---- 6. selectors ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.HEIGHTS)
def test_selector_values(ctx, n):
    """is_first = [r == 0], is_last = [r == n-1], is_transition = w_n^r - w_n^-1 (mh_constraint_fold's header comment)."""
    pkg = load_package()
    case = F.selector_case(n)
    w = pow(dag_eval.ROOT_2_32, (1 << 32) // n, P)
    w_inv = pow(w, n - 1, P)
    x = [int(v) for v in case.main[:, 0]]
    y = [int(v) for v in case.main[:, 1]]
    for jit in ("0", "1"):
        d = device_air(ctx, case.air, jit)
        got = fold_pairs(pkg.constraint_fold(ctx, d, case.main, alpha=(1 << 32, 0)))
        for r in (0, 1, n - 2, n - 1):
            first, last, trans = int(r == 0), int(r == n - 1), (pow(w, r, P) - w_inv) % P
            c = [first * x[r], last * y[r], trans * x[r] * y[r], first + 2 * last + trans * x[r]]
            f = sum(v * pow(1 << 32, 3 - k, P) for k, v in enumerate(c)) % P
            assert got[r] == (f, 0), (jit, r)
        assert (pow(w, n - 1, P) - w_inv) % P == 0  # is_transition vanishes on the last row, and only there
    check_case(ctx, "selectors", (), n, F.ALPHAS[1:3])


# ---- 7. generator switches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name,args", [("single", ()), ("lattice", ()), ("ef", ()), ("dot", (2,)), ("dot", (3,)), ("dot", (400,)), ("dot", (401,))])
def test_generator_switches(ctx, monkeypatch, tmp_path, switch, name, args):
    """Cases 1, 2 and 5 again with the products emitted as lz_mulN<2|3|4> groups, with the canonicalising arithmetic, and with the
    limb-by-limb fold_value.  Under MH_JIT_MULGROUP=4 the lattice's generated source must call all three group forms: a form that is
    never emitted is not tested."""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    dump = switch == "mulgroup4" and name == "lattice"
    if dump:
        monkeypatch.setenv("MH_JIT_DUMP", str(tmp_path))
    for n in F.HEIGHTS:
        check_case(ctx, name, args, n, F.ALPHAS[2:4], jits=("1",))
    if dump:
        src = "".join(open(os.path.join(tmp_path, f)).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip"))
        for form in (2, 3, 4):
            assert re.search(r"lz_mulN<%d>\(g\d+r, ga, gb\)" % form, src), f"the lattice AIR never calls lz_mulN<{form}>"


# ---- 8. consistency with the checker ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.HEIGHTS)
def test_nonzero_fold_rows_are_the_checkers_failing_rows(ctx, n):
    pkg = load_package()
    air = F.lattice_air(levels=1)
    main = F.lattice_trace(n)
    for i in range(F.LATTICE_PAIRS):
        for r in range(n):
            main[r, 3 * i + 2] = int(main[r, 3 * i]) * int(main[r, 3 * i + 1]) % P
    wrong = sorted({0, 1, n // 2, n - 2, n - 1})
    for j, r in enumerate(wrong):
        c = 3 * (j % F.LATTICE_PAIRS) + 2
        main[r, c] = (int(main[r, c]) + 1) % P
    for jit in ("0", "1"):
        d = device_air(ctx, air, jit)
        for alpha in F.ALPHAS[1:4]:
            got = fold_pairs(pkg.constraint_fold(ctx, d, main, alpha=alpha))
            assert [r for r in range(n) if got[r] != (0, 0)] == wrong, (jit, alpha)
        for exact in (False, True):
            entries, rows = pkg.check_constraints(ctx, d, main, exact=exact)
            assert rows == wrong and sum(e.rows for e in entries) == len(wrong), (jit, exact)


def test_malformed_calls(ctx):
    """The argument checks of mh_check_constraints: an error code and a message, never an exception across the C ABI."""
    import ctypes as C
    pkg = load_package()
    case = F.ef_case(8)
    d = device_air(ctx, case.air, "0")
    with pytest.raises(pkg.MidenHipError):  # width
        pkg.constraint_fold(ctx, d, case.main[:, :1], **case.kwargs())
    with pytest.raises(pkg.MidenHipError):  # no aux trace for an AIR with aux columns
        pkg.constraint_fold(ctx, d, case.main, randomness=case.rnd, aux_values=case.avs)
    with pytest.raises(pkg.MidenHipError):  # not enough randomness
        pkg.constraint_fold(ctx, d, case.main, aux=case.aux, randomness=case.rnd[:1], aux_values=case.avs)
    tm = pkg.Trace(ctx, case.main)
    out = np.zeros((8, 2), dtype=np.uint64)
    assert ctx.lib.mh_constraint_fold(ctx.h, d.h, tm.h, None, None, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0), None,
                                      pkg._ptr(out)) == 1  # null alpha: MH_ERR_INVALID
    assert ctx.lib.mh_constraint_fold(None, d.h, tm.h, None, None, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0), None,
                                      pkg._ptr(out)) == 1
