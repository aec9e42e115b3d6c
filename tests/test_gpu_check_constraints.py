"""GPU: the constraint checker (mh_check_constraints / mh_check_miden* / mh_check_precompile*, csrc/check.hip), run with -m gpu.

Per-constraint results are held to an independent evaluation of the DAG over Python integers and to the CPU oracle's
check_constraints (crates/lifted-stark/src/debug.rs); screen and exact mode must agree, under the interpreter and under the compiled
chunks alike."""
import os
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
import ref_traces as RT
from dag_eval import evaluate
from __graft_entry__ import load_package
from miden_vm_amd import dag, core_air as CO, precompile_airs as PA
from miden_vm_amd.testing import precompile_trace as PT

pytestmark = pytest.mark.gpu
P = dag.P
CASES = RT.load_cases()


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def device_air(ctx, air, jit):
    pkg = load_package()
    old = os.environ.get("MH_JIT")
    os.environ["MH_JIT"] = jit
    try:
        return pkg.DeviceAir(ctx, air)
    finally:
        if old is None:
            os.environ.pop("MH_JIT", None)
        else:
            os.environ["MH_JIT"] = old


# the independent evaluation (the blob's DAG over Python integers) lives in tests/dag_eval.py, shared with the fold tests


def as_dict(entries):
    return {e.constraint: (e.rows, e.first_row, (e.value[0], e.value[1])) for e in entries}


def oracle_pair(entries):
    """(sum of rows, first (row, constraint)) in the oracle's terms."""
    if not entries:
        return 0, None
    f = min(entries, key=lambda e: (e.first_row, e.constraint))
    return sum(e.rows for e in entries), (f.first_row, f.constraint)


RANDOM_CASES = [(seed, log_n) for seed, log_n in ((1, 3), (2, 5), (3, 6), (4, 8), (5, 10))]


@pytest.mark.parametrize("seed,log_n", RANDOM_CASES)
def test_random_constraint_systems_match_an_independent_evaluation(ctx, seed, log_n):
    pkg = load_package()
    air = A.random_air(seed, with_preprocessed=seed in (3, 5), log_n=log_n)
    rng = np.random.default_rng(100 + seed)
    n = 1 << log_n
    main = rng.integers(0, P, (n, 6), dtype=np.uint64)
    aux = rng.integers(0, P, (n, 4), dtype=np.uint64)
    # a few rows satisfied by construction would need a solver: instead zero a whole window so some constraints vanish there
    main[n // 2] = 0
    pub = [5, 7]
    rnd = [(11, 13), (17, 19)]
    avs = [(23, 29), (31, 37)]
    exp = evaluate(air, main, aux, air.preprocessed, pub, rnd, avs)
    cnt, first = ob.check_constraints(air, main, aux=aux, aux_values=[x for v in avs for x in v], publics=pub, randomness=rnd,
                                      preprocessed=air.preprocessed)
    results = []
    for jit in ("0", "1"):
        d = device_air(ctx, air, jit)
        prep = pkg.Trace(ctx, air.preprocessed) if air.preprocessed is not None else None
        for exact in (False, True):
            entries, rows = pkg.check_constraints(ctx, d, main, aux=aux, preprocessed=prep, publics=pub, randomness=rnd, aux_values=avs,
                                                  exact=exact)
            assert as_dict(entries) == exp, (jit, exact)
            assert oracle_pair(entries) == (cnt, first), (jit, exact)
            results.append((entries, rows))
    assert all(r == results[0] for r in results)


@pytest.mark.parametrize("log_n", [3, 6, 9])
def test_periodic_air_with_perturbations(ctx, log_n):
    """periodic_air: periodic columns shorter than the trace; satisfied, then one cell changed at row 0, n-1 and a periodic-gated row."""
    pkg = load_package()
    air = A.periodic_air()
    main = A.periodic_trace(log_n)
    rnd = [(3, 4), (5, 6)]
    aux, avs = air.build_aux(main, rnd)
    avs = [(avs[0], avs[1]), (avs[2], avs[3])]
    pub = [1, 2, 3]
    n = 1 << log_n
    for jit in ("0", "1"):
        d = device_air(ctx, air, jit)
        for exact in (False, True):
            assert pkg.check_constraints(ctx, d, main, aux=aux, publics=pub, randomness=rnd, aux_values=avs, exact=exact) == ([], [])
    for row in (0, n - 1, 5 % n):
        bad = main.copy()
        bad[row, 0] = (int(bad[row, 0]) + 1) % P
        exp = evaluate(air, bad, aux, None, pub, rnd, avs)
        cnt, first = ob.check_constraints(air, bad, aux=aux, aux_values=[x for v in avs for x in v], publics=pub, randomness=rnd)
        got = []
        for jit in ("0", "1"):
            d = device_air(ctx, air, jit)
            for exact in (False, True):
                entries, rows = pkg.check_constraints(ctx, d, bad, aux=aux, publics=pub, randomness=rnd, aux_values=avs, exact=exact)
                assert as_dict(entries) == exp
                assert oracle_pair(entries) == (cnt, first)
                got.append((entries, rows))
        assert all(g == got[0] for g in got)


def test_whole_column_error_counts_every_row(ctx):
    """2^18 rows with a wrong aux column: constraints failing on all n (or n-1) rows exercise the wave-aggregated atomics."""
    pkg = load_package()
    air = A.periodic_air()
    log_n = 18
    n = 1 << log_n
    main = A.periodic_trace(log_n)
    rnd = [(3, 4), (5, 6)]
    aux = np.random.default_rng(9).integers(1, P, (n, 4), dtype=np.uint64)
    avs = [(1, 2), rnd[1]]
    want = {2: n - 1, 3: 1, 4: n, 5: n - 1, 6: 1}
    for jit in ("0", "1"):
        d = device_air(ctx, air, jit)
        for exact in (False, True):
            entries, rows = pkg.check_constraints(ctx, d, main, aux=aux, publics=[1, 2, 3], randomness=rnd, aux_values=avs, exact=exact)
            assert {e.constraint: e.rows for e in entries} == want
            assert rows == list(range(n))


def statement(c):
    return [c["core"], c["chiplets"], c["poseidon2"]], RT.public_values(c), RT.aux_inputs(c)


def test_reference_snapshots_are_satisfied(ctx):
    pkg = load_package()
    m = pkg.Miden(ctx)
    for c in CASES:
        mats, pv, aux_in = statement(c)
        assert m.check(*mats, pv, aux_in) == [], c["case"]
        assert m.check(*[ctx.upload_trace(t) for t in mats], pv, aux_in, exact=True) == [], c["case"]


def test_perturbed_snapshot_matches_the_oracle(ctx):
    pkg = load_package()
    m = pkg.Miden(ctx)
    c = CASES[12]
    mats, pv, aux_in = statement(c)
    core = RT.statement_airs(ob.lookup_build_aux)["core"]
    for row in (0, 7, c["core"].shape[0] - 1):
        bad = mats[0].copy()
        bad[row, CO.STACK_TOP[1]] = (int(bad[row, CO.STACK_TOP[1]]) + 1) % P
        screen = m.check(bad, mats[1], mats[2], pv, aux_in)
        assert screen == m.check(bad, mats[1], mats[2], pv, aux_in, exact=True)
        local = [e for e in screen if e.instance >= 0]
        assert local and all(e.instance == 0 for e in local)
        # the oracle on the same perturbed matrix, aux rebuilt from it (the local verdicts do not depend on the challenges)
        rnd = [(123, 456), (789, 1011)]
        aux, fin = ob.lookup_build_aux(core[1], bad, rnd)
        cnt, first = ob.check_constraints(core[0], bad, aux=aux, aux_values=[int(fin[0]), int(fin[1])], publics=pv, randomness=rnd)
        assert oracle_pair(local) == (cnt, first), row


def test_wrong_program_hash_is_one_external_entry(ctx):
    pkg = load_package()
    m = pkg.Miden(ctx)
    mats, pv, aux_in = statement(CASES[12])
    bad = list(aux_in)
    bad[1] = (bad[1] + 1) % P
    got = m.check(*mats, pv, bad)
    assert len(got) == 1 and got[0].instance == -1 and got[0].constraint == 0 and got[0].rows == 1


@pytest.fixture(scope="module")
def session():
    pairs, traces, info = PT.precompile_session([b"", b"abc", bytes(range(200))], lambda *a: ob.lookup_build_aux(*a))
    return pairs, traces, info["public_root"]


def test_precompile_session(ctx, session):
    pkg = load_package()
    pairs, traces, root = session
    pc = pkg.Precompile(ctx)
    assert pc.check(traces, root) == []
    assert pc.check([ctx.upload_trace(t) for t in traces], root, exact=True) == []
    wrong = list(root)
    wrong[0] = (wrong[0] + 1) % P
    # the root is pinned by TranscriptEval's first row (a local constraint of instance 5), not by the session's external assertion
    got = pc.check(traces, wrong)
    assert len(got) == 1 and (got[0].instance, got[0].first_row, got[0].rows) == (5, 0, 1), got


def test_precompile_one_cell_per_chiplet(ctx, session):
    """One cell changed in each of the twelve AIRs: the local entries name that instance only and match the oracle on it."""
    pkg = load_package()
    pairs, traces, root = session
    pc = pkg.Precompile(ctx)
    rnd = [(3, 5), (7, 11), (13, 17), (19, 23)]
    for i, (air, lookup) in enumerate(pairs):
        n = traces[i].shape[0]
        for col in range(traces[i].shape[1]):  # the first column whose change some constraint sees
            bad = traces[i].copy()
            bad[n // 2, col] = (int(bad[n // 2, col]) + 1) % P
            prep = air.preprocessed
            aux, fin = ob.lookup_build_aux(lookup, bad, rnd[:lookup.num_randomness] if hasattr(lookup, "num_randomness") else rnd,
                                           preprocessed=prep)
            avs = [int(fin[0]), int(fin[1])] + [0, 0] * (air.num_aux_values - 1)
            cnt, first = ob.check_constraints(air, bad, aux=aux, aux_values=avs, publics=[int(x) for x in root],
                                              randomness=rnd[:air.num_randomness], preprocessed=prep)
            if cnt:
                break
        mains = list(traces)
        mains[i] = bad
        got = pc.check(mains, root)
        local = [e for e in got if e.instance >= 0]
        assert oracle_pair(local) == (cnt, first), i
        if cnt:
            assert all(e.instance == i for e in local), i
        else:  # BytePairLut's main columns are multiplicities: no local constraint sees them, only the bus balance does
            assert len(got) == 1 and got[0].instance == -1, (i, got)


def test_malformed_calls(ctx):
    import ctypes as C
    pkg = load_package()
    air = A.periodic_air()
    d = device_air(ctx, air, "0")
    main = A.periodic_trace(4)
    rnd = [(3, 4), (5, 6)]
    aux, avs = air.build_aux(main, rnd)
    avs = [(avs[0], avs[1]), (avs[2], avs[3])]
    with pytest.raises(pkg.MidenHipError):  # width
        pkg.check_constraints(ctx, d, main[:, :2], aux=aux, publics=[1, 2, 3], randomness=rnd, aux_values=avs)
    with pytest.raises(pkg.MidenHipError):  # height of the aux trace
        pkg.check_constraints(ctx, d, main, aux=aux[:8], publics=[1, 2, 3], randomness=rnd, aux_values=avs)
    with pytest.raises(pkg.MidenHipError):  # no aux trace for an AIR with aux columns
        pkg.check_constraints(ctx, d, main, publics=[1, 2, 3], randomness=rnd, aux_values=avs)
    lib = ctx.lib
    tm, ta = pkg.Trace(ctx, main), pkg.Trace(ctx, aux)
    pub, r, av = (np.array(x, dtype=np.uint64) for x in ([1, 2, 3], [3, 4, 5, 6], [x for v in avs for x in v]))
    bad = main.copy()
    bad[3, 0] = (int(bad[3, 0]) + 1) % P
    tb = pkg.Trace(ctx, bad)
    n = C.c_size_t(99)

    def call(t, flags, cap, out=None):
        return lib.mh_check_constraints(ctx.h, d.h, t.h, ta.h, None, pkg._ptr(pub), C.c_size_t(3), pkg._ptr(r), C.c_size_t(2), pkg._ptr(av),
                                        C.c_size_t(2), C.c_int(flags), out, C.c_size_t(cap), C.byref(n), None)

    assert call(tm, 0, 0) == 0 and n.value == 0
    assert call(tb, 0, 0) == pkg.MH_ERR_UNSATISFIED and n.value >= 1  # cap = 0: counted, nothing written
    assert b"row" in lib.mh_last_error(ctx.h)
    assert call(tb, 4, 0) == 1  # unknown flags: MH_ERR_INVALID
    assert lib.mh_check_constraints(ctx.h, d.h, tm.h, ta.h, None, pkg._ptr(pub), C.c_size_t(2), pkg._ptr(r), C.c_size_t(2), pkg._ptr(av),
                                    C.c_size_t(2), C.c_int(0), None, C.c_size_t(0), C.byref(n), None) == 1  # public count
    m = pkg.Miden(ctx)
    mats, pv, aux_in = statement(CASES[0])
    with pytest.raises(pkg.MidenHipError):
        m.check(*mats, pv[:31] + [0, 0], aux_in[:7])


def test_c_example(ctx, tmp_path):
    """examples/check_miden_c_abi.c, built with gcc -Wall -Werror: exit 0 on case 13, nonzero (and the cell named) when perturbed."""
    import subprocess
    from __graft_entry__ import ROOT
    exe = str(tmp_path / "check_miden")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "check_miden_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    mats, pv, aux_in = statement(CASES[12])

    def write(core, path):
        lh = [int(x.shape[0]).bit_length() - 1 for x in (core, mats[1], mats[2])]
        words = lh + [len(aux_in)] + list(pv) + list(aux_in)
        with open(path, "wb") as f:
            f.write(np.array(words, dtype=np.uint64).tobytes())
            for x in (core, mats[1], mats[2]):
                f.write(np.ascontiguousarray(x, dtype=np.uint64).tobytes())

    good, badf = str(tmp_path / "good.bin"), str(tmp_path / "bad.bin")
    write(mats[0], good)
    bad = mats[0].copy()
    bad[7, CO.STACK_TOP[1]] = (int(bad[7, CO.STACK_TOP[1]]) + 1) % P
    write(bad, badf)
    env = dict(os.environ)
    assert subprocess.run([exe, good], env=env, capture_output=True, timeout=120).returncode == 0
    r = subprocess.run([exe, badf], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "instance 0" in r.stdout, r.stdout + r.stderr
