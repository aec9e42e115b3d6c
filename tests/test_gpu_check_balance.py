"""GPU: the bus-balance checker (mh_check_balance*, csrc/balance.hip), run with -m gpu.

Every report is held to tests/balance_ref.py: an evaluation of the lookup blob over Python integers and a dict from denominator to net
multiplicity (the reference's HashMap walk, air/src/lookup/debug/trace/mod.rs:44-95), in the order the header specifies."""
import ctypes as C
import os
import subprocess
import time
import numpy as np
import pytest
import airs as A
import balance_ref as BR
import oracle_binding as ob
import ref_traces as RT
from __graft_entry__ import load_package, ROOT
from miden_vm_amd import dag, miden_statement as MS, precompile_airs as PA, protocol
from miden_vm_amd.testing import precompile_trace as PT

pytestmark = pytest.mark.gpu
P = dag.P
CASES = RT.load_cases()
RNDS = ([(3, 5), (7, 11)], [(1 << 40, 12345), (P - 2, 99)])


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def raw(entries):
    return b"".join(bytes(e) for e in entries), b"".join(bytes(p) for e in entries for p in e.push_list)


def both_modes(call):
    """call(exact) twice each: byte-identical; the screen (where it did not return early) and the exact mode agree."""
    s1, s2, x1, x2 = call(False), call(False), call(True), call(True)
    assert raw(s1) == raw(s2) and raw(x1) == raw(x2)
    assert raw(s1) == raw(x1)
    return x1


@pytest.mark.parametrize("log_n,rnd", [(4, 0), (4, 1), (10, 0), (10, 1), (16, 1)])
def test_logup_air(ctx, log_n, rnd):
    pkg = load_package()
    _, lookup = A.logup_air()
    dl = pkg.DeviceLookup(ctx, lookup)
    rnd = RNDS[rnd]
    good = A.logup_trace(log_n)
    assert both_modes(lambda exact: pkg.check_balance(ctx, [dl], [good], rnd, exact=exact)) == []
    bads = [A.logup_trace(log_n, valid=False)]
    rng = np.random.default_rng(log_n)
    for _ in range(0 if log_n == 16 else 3):  # random one-cell changes
        t = good.copy()
        r, c = int(rng.integers(0, 1 << log_n)), int(rng.integers(0, 8))
        t[r, c] = (int(t[r, c]) + 1 + int(rng.integers(0, 1000))) % P
        bads.append(t)
    for t in bads:
        exp = BR.balance([BR.fractions(lookup.blob, t, rnd)])
        got = both_modes(lambda exact: pkg.check_balance(ctx, [dl], [t], rnd, exact=exact))
        assert BR.as_report(got) == exp
        assert [e.pushes for e in got] == [len(p) for _, _, p in exp]


@pytest.mark.parametrize("log_n", [5, 12])
def test_range_air_with_preprocessed_table_and_boundary(ctx, log_n):
    pkg = load_package()
    air, lookup, trace = A.range_air(log_n)
    dl = pkg.DeviceLookup(ctx, lookup)
    prep = pkg.Trace(ctx, air.preprocessed)
    for rnd in RNDS:
        assert both_modes(lambda exact: pkg.check_balance(ctx, [dl], [trace()], rnd, preprocessed=[prep], exact=exact)) == []
        bad = trace(valid=False)
        fr = BR.fractions(lookup.blob, bad, rnd, prep=air.preprocessed)
        got = both_modes(lambda exact: pkg.check_balance(ctx, [dl], [bad], rnd, preprocessed=[prep], exact=exact))
        exp = BR.balance([fr])
        assert exp and BR.as_report(got) == exp
        # boundary pushes that cancel the two unmatched denominators: balanced again; one of them alone: the other stays
        fix = [(d, -1 if net == (1, 0) else 1) for d, net, _ in exp]
        if all(net in ((1, 0), (P - 1, 0)) for _, net, _ in exp):
            assert pkg.check_balance(ctx, [dl], [bad], rnd, boundary=fix, preprocessed=[prep], exact=True) == []
            got = pkg.check_balance(ctx, [dl], [bad], rnd, boundary=fix[:1], preprocessed=[prep], exact=True)
            assert BR.as_report(got) == BR.balance([fr], fix[:1])
        # a boundary push on a key of its own
        got = pkg.check_balance(ctx, [dl], [trace()], rnd, boundary=[((5, 6), -1)], preprocessed=[prep])
        assert BR.as_report(got) == [((5, 6), (P - 1, 0), [(-1, 0, 0, 0, (P - 1, 0))])]


def one_bus_lookup():
    """One fraction M / (r0 + V) per row: main columns V, M."""
    lb = dag.LookupBuilder(2, num_cols=1, num_randomness=1)
    lb.fraction(0, lb.main(1), lb.randomness(0) + lb.main(0))
    return dag.Lookup(lb, "one_bus")


def test_hot_key_single_key_and_wrapping_sums(ctx):
    """2^12 - 1 pushes on one key with multiplicities p - 1 (their integer sum passes 2^64 thousands of times before the reduction)
    and one push on a key of its own; then the same hot key netting to zero."""
    pkg = load_package()
    lookup = one_bus_lookup()
    dl = pkg.DeviceLookup(ctx, lookup)
    n = 1 << 12
    rnd = [(17, 19)]
    t = np.zeros((n, 2), dtype=np.uint64)
    t[:, 0], t[:, 1] = 5, P - 1
    t[77] = (9, 3)
    got = both_modes(lambda exact: pkg.check_balance(ctx, [dl], [t], rnd, exact=exact))
    exp = BR.balance([BR.fractions(lookup.blob, t, rnd)])
    assert BR.as_report(got) == exp
    assert sorted((e.pushes, e.net[0]) for e in got) == [(1, 3), (n - 1, P - (n - 1))]
    t[::2, 1] = 1       # the hot key now holds ones and p - 1 in turn ...
    t[77] = (9, 3)
    t[78] = (5, P - 2)
    t[79] = (5, 1)      # ... evened out to a zero net: only the single key is left
    got = both_modes(lambda exact: pkg.check_balance(ctx, [dl], [t], rnd, exact=exact))
    exp = BR.balance([BR.fractions(lookup.blob, t, rnd)])
    assert BR.as_report(got) == exp and len(exp) == 1 and exp[0][1] == (3, 0)


def test_caps_and_totals(ctx):
    pkg = load_package()
    _, lookup = A.logup_air()
    dl = pkg.DeviceLookup(ctx, lookup)
    rnd = RNDS[0]
    t = A.logup_trace(8)
    t[:, 0] = (t[:, 0] + np.uint64(1)) % np.uint64(P)  # every looked-up value wrong
    full = pkg.check_balance(ctx, [dl], [t], rnd)
    fe, fp = raw(full)
    n_e, n_p = len(full), sum(e.pushes for e in full)
    assert n_e > 100 and n_p > n_e
    tr = pkg.Trace(ctx, t)
    r = np.array([x for e in rnd for x in e], dtype=np.uint64)
    la, ta = (C.c_void_p * 1)(dl.h), (C.c_void_p * 1)(tr.h)
    for ecap, pcap in ((0, 0), (1, 2), (7, 1000), (1000, 3)):
        ent, psh = (pkg.BalanceEntry * max(1, ecap))(), (pkg.BalancePush * max(1, pcap))()
        ne, np_ = C.c_size_t(0), C.c_size_t(0)
        rc = ctx.lib.mh_check_balance(ctx.h, C.c_int(1), la, ta, None, pkg._ptr(r), C.c_size_t(2), None, None, C.c_size_t(0), C.c_int(0),
                                      ent if ecap else None, C.c_size_t(ecap), C.byref(ne), psh if pcap else None, C.c_size_t(pcap), C.byref(np_))
        assert rc == pkg.MH_ERR_UNSATISFIED and (ne.value, np_.value) == (n_e, n_p)
        we, wp = min(ecap, n_e), min(pcap, n_p)
        assert bytes(ent)[:48 * we] == fe[:48 * we] and bytes(psh)[:40 * wp] == fp[:40 * wp]
    assert b"unmatched" in ctx.lib.mh_last_error(ctx.h)


def test_malformed_calls(ctx):
    pkg = load_package()
    _, lookup = A.logup_air()
    dl = pkg.DeviceLookup(ctx, lookup)
    good = A.logup_trace(4)
    rnd = RNDS[0]
    with pytest.raises(pkg.MidenHipError):  # width
        pkg.check_balance(ctx, [dl], [good[:, :5]], rnd)
    with pytest.raises(pkg.MidenHipError):  # too few challenges
        pkg.check_balance(ctx, [dl], [good], rnd[:1])
    with pytest.raises(pkg.MidenHipError):  # a boundary sign
        pkg.check_balance(ctx, [dl], [good], rnd, boundary=[((1, 2), 2)])
    with pytest.raises(pkg.MidenHipError):  # a zero boundary denominator
        pkg.check_balance(ctx, [dl], [good], rnd, boundary=[((0, 0), 1)])
    other = pkg.Ctx(0)
    try:
        with pytest.raises(pkg.MidenHipError):  # a trace of another context
            pkg.check_balance(ctx, [dl], [pkg.Trace(other, good)], rnd)
    finally:
        other.close()
    tr = pkg.Trace(ctx, good)
    r = np.array([x for e in rnd for x in e], dtype=np.uint64)
    la, ta = (C.c_void_p * 1)(dl.h), (C.c_void_p * 1)(tr.h)
    ne, np_ = C.c_size_t(0), C.c_size_t(0)

    def call(flags=0, n_entries=C.byref(ne), lookups=la):
        return ctx.lib.mh_check_balance(ctx.h, C.c_int(1), lookups, ta, None, pkg._ptr(r), C.c_size_t(2), None, None, C.c_size_t(0), C.c_int(flags),
                                        None, C.c_size_t(0), n_entries, None, C.c_size_t(0), C.byref(np_))

    assert call() == 0
    assert call(flags=4) == 1            # unknown flags
    assert call(n_entries=None) == 1     # null argument
    assert call(lookups=None) == 1
    assert call(lookups=(C.c_void_p * 1)(None)) == 1
    # a live push whose denominator is zero
    lb = dag.LookupBuilder(2, num_cols=1, num_randomness=1)
    lb.fraction(0, lb.main(1), lb.main(0))
    dz = pkg.DeviceLookup(ctx, dag.Lookup(lb, "zero_denominator"))
    t = np.ones((8, 2), dtype=np.uint64)
    assert pkg.check_balance(ctx, [dz], [t], [(1, 1)], exact=True) != []
    t[3, 0] = 0
    for exact in (False, True):
        with pytest.raises(pkg.MidenHipError, match="zero"):
            pkg.check_balance(ctx, [dz], [t], [(1, 1)], exact=exact)
    t[3, 1] = 0  # not live: no push, no error
    assert len(pkg.check_balance(ctx, [dz], [t], [(1, 1)])) == 1
    m = pkg.Miden(ctx)
    mats, pv, aux_in = statement(CASES[0])
    with pytest.raises(pkg.MidenHipError):
        m.check_balance(*mats, pv, aux_in[:7])


# ---- the Miden statement ----
def statement(c):
    return [c["core"], c["chiplets"], c["poseidon2"]], RT.public_values(c), RT.aux_inputs(c)


def debug_challenges(state, pre, log_heights, count):
    """The challenges of mh_check_* (include/midenhip.h): state, pre-observe schedule, number of AIRs, log heights, then samples."""
    ch = ob.Challenger(state)
    ch.observe([int(x) for x in pre] + [len(log_heights)] + [int(x) for x in log_heights])
    return [ch.sample_ef() for _ in range(count)]


def miden_reference(mats, pv, aux_in):
    lookups = RT.statement_airs(ob.lookup_build_aux)
    state = np.zeros(12, dtype=np.uint64)
    load_package().load_library().mh_miden_challenger_state(ob.ptr(state))
    pre = MS.statement_pre_observe(protocol.PROD_PARAMS, pv, aux_in)
    rnd = debug_challenges([int(x) for x in state], pre, [int(m.shape[0]).bit_length() - 1 for m in mats], 2)
    ch = MS.Challenges(rnd[0], rnd[1])
    from miden_vm_amd import chiplets_air as CA
    bnd = [(ch.encode(CA.BUS_BLOCK_HASH_TABLE, list(aux_in[0:4]) + [0, 0, 0]), 1), (ch.encode(CA.BUS_LOG_DEFERRED_ROOT, [0, 0, 0, 0]), 1),
           (ch.encode(CA.BUS_LOG_DEFERRED_ROOT, list(aux_in[4:8])), -1)]
    bnd += [(ch.encode(CA.BUS_KERNEL_ROM_INIT, list(aux_in[i:i + 4])), 1) for i in range(8, len(aux_in), 4)]
    frs = [BR.fractions(lookups[k][1].blob, m, rnd) for k, m in zip(("core", "chiplets", "poseidon2"), mats)]
    return BR.balance(frs, bnd), lookups


def test_reference_snapshots_balance(ctx):
    pkg = load_package()
    m = pkg.Miden(ctx)
    for c in CASES:
        mats, pv, aux_in = statement(c)
        assert m.check_balance(*mats, pv, aux_in) == [], c["case"]
        assert m.check_balance(*[ctx.upload_trace(t) for t in mats], pv, aux_in, exact=True) == [], c["case"]


def test_wrong_program_hash_names_a_boundary_push(ctx):
    pkg = load_package()
    m = pkg.Miden(ctx)
    mats, pv, aux_in = statement(CASES[12])
    bad = list(aux_in)
    bad[1] = (bad[1] + 1) % P
    got = both_modes(lambda exact: m.check_balance(*mats, pv, bad, exact=exact))
    assert any(p.instance == -1 for e in got for p in e.push_list)
    exp, _ = miden_reference(mats, pv, bad)
    assert BR.as_report(got) == exp and len(exp) == 2


def test_changed_message_cells_match_the_reference(ctx):
    """One cell that a bus message reads, changed in each of the three AIRs at once: the report is the dict walk's, across the AIRs."""
    pkg = load_package()
    m = pkg.Miden(ctx)
    mats, pv, aux_in = statement(CASES[12])
    base, lookups = miden_reference(mats, pv, aux_in)
    assert base == []
    bad = [t.copy() for t in mats]
    for i, k in enumerate(("core", "chiplets", "poseidon2")):
        for col in BR.main_reads(lookups[k][1].blob):  # the first message cell of row 3 whose change unbalances a bus
            trial = [t.copy() for t in mats]
            trial[i][3, col] = (int(trial[i][3, col]) + 1) % P
            if miden_reference(trial, pv, aux_in)[0]:
                bad[i][3, col] = trial[i][3, col]
                break
    exp, _ = miden_reference(bad, pv, aux_in)
    got = both_modes(lambda exact: m.check_balance(*bad, pv, aux_in, exact=exact))
    assert BR.as_report(got) == exp
    assert len({p[0] for _, _, ps in exp for p in ps}) >= 2  # pushes of several instances


# ---- the precompile session ----
@pytest.fixture(scope="module")
def session():
    pairs, traces, info = PT.precompile_session([b"", b"abc", bytes(range(200))], lambda *a: ob.lookup_build_aux(*a))
    return pairs, traces, info["public_root"]


def session_fractions(pairs, traces, root, cache={}):
    """-> (per chiplet the reference's fractions, the verifier's boundary pushes) under the session's debug challenges"""
    root = [int(x) for x in root]
    pre = protocol.protocol_pre_observe(protocol.PROD_PARAMS, root, (), preprocessed_root=[0, 0, 0, 0])
    n_rnd = max(air.num_randomness for air, _ in pairs)
    rnd = debug_challenges([0] * 12, pre, [int(t.shape[0]).bit_length() - 1 for t in traces], n_rnd)
    msgs = [(PA.BUS_EC_GROUP, list(g)) for g in PA.FIXED_EC_GROUPS]
    msgs += [(PA.BUS_UINT_VAL, [ptr, bp] + [(v >> (32 * j)) & 0xffffffff for j in range(8)]) for ptr, bp, v in PA.FIXED_UINTS]
    bnd = [(PA._encode(rnd[0], rnd[1], bus, f), 1) for bus, f in msgs]
    frs = []
    for i, ((air, lookup), t) in enumerate(zip(pairs, traces)):
        key = (i, t.tobytes(), tuple(rnd))
        if key not in cache:
            cache[key] = BR.fractions(lookup.blob, t, rnd, prep=air.preprocessed)
        frs.append(cache[key])
    return frs, bnd


def session_reference(pairs, traces, root):
    return BR.balance(*session_fractions(pairs, traces, root))


def first_live_row(fr, start):
    """The first row from `start` on which one of the fractions `fr` is a live push: a chiplet's padding and idle rows push nothing, and
    a cell changed there changes no message."""
    n = len(fr[0][2])
    return next(r for r in range(start, n) if any((m0[r], m1[r]) != (0, 0) for _, _, m0, m1, _, _ in fr))


def test_precompile_session(ctx, session):
    pkg = load_package()
    pairs, traces, root = session
    pc = pkg.Precompile(ctx)
    assert pc.check_balance(traces, root) == []
    assert pc.check_balance([ctx.upload_trace(t) for t in traces], root, exact=True) == []
    assert session_reference(pairs, traces, root) == []
    frs, _ = session_fractions(pairs, traces, root)
    both = 0
    for i in (0, 2, 3, 6, 9):  # a message cell changed in several chiplets, one at a time, on a row that pushes
        r = first_live_row(frs[i], 1 if i != 3 else 0x0102)
        exp = []
        for col in BR.main_reads(pairs[i][1].blob):
            bad = list(traces)
            bad[i] = traces[i].copy()
            bad[i][r, col] = (int(bad[i][r, col]) + 1) % P
            exp = session_reference(pairs, bad, root)
            if exp:
                break
        assert exp, i
        got = both_modes(lambda exact: pc.check_balance(bad, root, exact=exact))
        assert BR.as_report(got) == exp, i
        both += len({p[0] for _, _, ps in exp for p in ps}) >= 2
    assert both  # some report names the providing and the consuming instance


def test_c_example(ctx, tmp_path):
    """examples/check_balance_c_abi.c, built with gcc -Wall -Werror: exit 0 on a snapshot, 1 (and a boundary push printed) with a wrong
    program hash."""
    exe = str(tmp_path / "check_balance")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "check_balance_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    mats, pv, aux_in = statement(CASES[12])

    def write(aux, path):
        lh = [int(x.shape[0]).bit_length() - 1 for x in mats]
        with open(path, "wb") as f:
            f.write(np.array(lh + [len(aux)] + list(pv) + list(aux), dtype=np.uint64).tobytes())
            for x in mats:
                f.write(np.ascontiguousarray(x, dtype=np.uint64).tobytes())

    good, badf = str(tmp_path / "good.bin"), str(tmp_path / "bad.bin")
    write(aux_in, good)
    bad = list(aux_in)
    bad[1] = (bad[1] + 1) % P
    write(bad, badf)
    r = subprocess.run([exe, good], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "balanced" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, badf, "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "instance -1" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.environ.get("MH_BALANCE_TIMING"), reason="timing case: set MH_BALANCE_TIMING=1 (profiles/r07_balance.txt)")
def test_timing_2_20_rows(ctx):
    """2^20 rows of logup_air: balanced (screen, exact), one damaged cell, a whole damaged column.  Prints the times; asserts only results."""
    pkg = load_package()
    _, lookup = A.logup_air()
    dl = pkg.DeviceLookup(ctx, lookup)
    rnd = RNDS[0]
    good = A.logup_trace(20)
    one = A.logup_trace(20, valid=False)
    col = good.copy()
    col[:, 0] = (col[:, 0] + np.uint64(1)) % np.uint64(P)
    for name, t, exact, want in (("balanced screen", good, False, 0), ("balanced exact", good, True, 0), ("one cell", one, False, 2),
                                 ("whole column", col, False, None)):
        tr = pkg.Trace(ctx, t)
        pkg.check_balance(ctx, [dl], [tr], rnd, exact=exact)
        t0 = time.perf_counter()
        got = pkg.check_balance(ctx, [dl], [tr], rnd, exact=exact)
        dt = time.perf_counter() - t0
        print(f"balance 2^20 logup_air {name}: {dt * 1e3:.2f} ms, {len(got)} entries, {sum(e.pushes for e in got)} pushes")
        assert want is None or len(got) == want
