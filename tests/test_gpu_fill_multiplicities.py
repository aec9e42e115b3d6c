"""GPU: multiplicity columns filled on the device (mh_fill_multiplicities*, csrc/multiplicity.hip), run with -m gpu.

Every filled trace and every report is held to tests/multiplicity_ref.py (the header's semantics over Python integers and dicts) or,
where the table's keys are unique, to the numpy ledger of the trace builder itself."""
import os
import subprocess
import numpy as np
import pytest
import airs as A
import balance_ref as BR
import multiplicity_ref as MR
import ref_traces as RT
from __graft_entry__ import load_package, ROOT
from miden_vm_amd import core_air as CO, dag, precompile_airs as PA, protocol
from miden_vm_amd.testing import precompile_trace as PT

pytestmark = pytest.mark.gpu
P = dag.P
RNDS = ([(3, 5), (7, 11)], [(1 << 40, 12345), (P - 2, 99)])  # tests/test_gpu_check_balance.py RNDS
JUNK = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def raw(entries):
    return b"".join(bytes(e) for e in entries), b"".join(bytes(p) for e in entries for p in e.push_list)


def fill_twice(ctx, lookups, mains, slots, rnd, boundary=(), preps=None):
    """Upload, fill, download; a second call on the filled traces leaves the same bytes and returns the same report.
    -> (cells written, filled matrices, report)"""
    pkg = load_package()
    dls = [pkg.DeviceLookup(ctx, lk) for lk in lookups]
    trs = [pkg.Trace(ctx, m) for m in mains]
    pr = None if preps is None else [None if p is None else pkg.Trace(ctx, p) for p in preps]
    w1, r1 = pkg.fill_multiplicities(ctx, dls, trs, slots, rnd, boundary=boundary, preprocessed=pr)
    out1 = [t.download() for t in trs]
    w2, r2 = pkg.fill_multiplicities(ctx, dls, trs, slots, rnd, boundary=boundary, preprocessed=pr)
    out2 = [t.download() for t in trs]
    assert w1 == w2 and raw(r1) == raw(r2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out1, out2))
    return w1, out1, r1


def against_reference(ctx, lookups, mains, slots, rnd, boundary=(), preps=None):
    """The library against multiplicity_ref.fill: cell for cell, the report entry for entry.  -> (written, filled, reference report)"""
    exp_w, exp_out, exp_rep = MR.fill([lk.blob for lk in lookups], mains, rnd, slots, boundary=boundary, preps=preps)
    w, out, rep = fill_twice(ctx, lookups, mains, slots, rnd, boundary=boundary, preps=preps)
    for a, b in zip(out, exp_out):
        assert (a == b).all(), np.argwhere(a != b)[:8]
    assert w == exp_w
    assert BR.as_report(rep) == exp_rep
    return w, out, exp_rep


# ---- 1, 2: the trace builders' own ledgers ----
@pytest.mark.parametrize("log_n,rnd", [(4, 0), (4, 1), (10, 0), (10, 1)])
def test_logup_air_equals_bincount(ctx, log_n, rnd):
    _, lookup = A.logup_air()
    good = A.logup_trace(log_n)
    slots = [(0,) + s for s in lookup.multiplicity_slots([2])]
    assert slots == [(0, 0, 1, 2)]
    for junk in (0, JUNK):
        t = good.copy()
        t[:, 2] = junk
        w, (out,), rep = fill_twice(ctx, [lookup], [t], slots, RNDS[rnd])
        assert (out == good).all() and rep == [] and w == 1 << log_n


@pytest.mark.parametrize("log_n", [5, 12])
def test_range_air_with_preprocessed_table(ctx, log_n):
    air, lookup, trace = A.range_air(log_n)
    good = trace()
    slots = [(0, 0, 1, 1)]
    for rnd in RNDS:
        for junk in (0, JUNK):
            t = good.copy()
            t[:, 1] = junk
            w, (out,), rep = fill_twice(ctx, [lookup], [t], slots, rnd, preps=[air.preprocessed])
            assert (out == good).all() and rep == [] and w == 1 << log_n
    # the value 2 is in no table row: reported; the column is the reference's
    bad = trace(valid=False)
    bad[:, 1] = JUNK
    if log_n == 5:
        _, _, exp = against_reference(ctx, [lookup], [bad], slots, RNDS[0], preps=[air.preprocessed])
    else:  # the reference's row-by-row walk is slow at 2^12 rows: the ledger minus the lost lookup, and the single unmatched push
        _, (out,), rep = fill_twice(ctx, [lookup], [bad], slots, RNDS[0], preps=[air.preprocessed])
        want = good[:, 1].copy()
        want[int(np.nonzero(air.preprocessed[:, 0] == good[3, 0])[0][0])] -= np.uint64(1)
        assert (out[:, 1] == want).all() and (out[:, 0] == bad[:, 0]).all()
        exp = BR.balance([BR.fractions(lookup.blob, out, RNDS[0], prep=air.preprocessed)])
        assert BR.as_report(rep) == exp
    assert len(exp) == 1 and exp[0][1] == (1, 0) and [p[1] for p in exp[0][2]] == [3]


# ---- 3 .. 5: small programs of the test's own ----
def provider(flagged=False, coeff=None, second_bus=False):
    """Main columns T, M (, F): -M / (r0 + T), or F * (0 - M) / (r0 + T), or coeff * M / (r0 + T); second_bus: also -M / (r1 + T)."""
    lb = dag.LookupBuilder(3 if flagged else 2, num_cols=1, num_randomness=2)
    T, M = lb.main(0), lb.main(1)
    m = lb.main(2) * (lb.const(0) - M) if flagged else (M * coeff if coeff is not None else -M)
    lb.fraction(0, m, lb.randomness(0) + T)
    if second_bus:
        lb.fraction(0, -M, lb.randomness(1) + T)
    return dag.Lookup(lb, "provider")


def consumer(second_bus=False):
    """Main columns V, S (, V2): S / (r0 + V); second_bus: also S / (r1 + V2)."""
    lb = dag.LookupBuilder(3 if second_bus else 2, num_cols=1, num_randomness=2)
    lb.fraction(0, lb.main(1), lb.randomness(0) + lb.main(0))
    if second_bus:
        lb.fraction(0, lb.main(1), lb.randomness(1) + lb.main(2))
    return dag.Lookup(lb, "consumer")


def key(rnd, i, v):
    return ((rnd[i][0] + int(v)) % P, rnd[i][1])


def test_cross_instance_mixed_heights_and_a_boundary_push(ctx):
    rng = np.random.default_rng(41)
    np_, nc = 1 << 6, 1 << 9
    table = rng.permutation(np.arange(100, 100 + 3 * np_, 3, dtype=np.uint64))
    prov = np.stack([table, np.full(np_, JUNK, dtype=np.uint64)], axis=1)
    picks = rng.integers(0, np_, nc)
    cons = np.stack([table[picks], rng.integers(0, 3, nc).astype(np.uint64)], axis=1)  # multiplicities 0, 1, 2
    for rnd in RNDS:
        boundary = [(key(rnd, 0, table[5]), 1)]
        # the consumer first, then the provider: the instance order is the caller's
        w, (c_out, p_out), rep = against_reference(ctx, [consumer(), provider()], [cons, prov], [(1, 0, 0, 1)], rnd, boundary=boundary)
        assert rep == [] and w == np_ and (c_out == cons).all()
        want = np.bincount(picks, weights=cons[:, 1].astype(np.float64), minlength=np_).astype(np.uint64)
        want[5] += np.uint64(1)
        assert (p_out[:, 1] == want).all()


def test_duplicate_provider_keys_and_a_hot_key(ctx):
    """One AIR: V, S consume; T, M provide.  The table repeats values (the lowest row gets the sum, the others 0); 2^12 - 1 consumers with
    multiplicity p - 1 sit on one key, so the low word of its sum wraps thousands of times before the reduction."""
    lb = dag.LookupBuilder(4, num_cols=1, num_randomness=1)
    lb.fraction(0, lb.main(1), lb.randomness(0) + lb.main(0))
    lb.fraction(0, -lb.main(3), lb.randomness(0) + lb.main(2))
    lookup = dag.Lookup(lb, "hot")
    n = 1 << 12
    t = np.zeros((n, 4), dtype=np.uint64)
    t[:, 0], t[:, 1] = 5, P - 1
    t[n - 1, 0:2] = (9, 3)
    t[:, 2] = np.arange(1000, 1000 + n, dtype=np.uint64)
    t[[7, 100, 4000], 2] = 5        # three rows carry the hot key
    t[[50, 51], 2] = 9
    t[:, 3] = JUNK
    w, (out,), rep = against_reference(ctx, [lookup], [t], [(0, 0, 1, 3)], [(17, 19)])
    assert rep == [] and w == n
    assert int(out[7, 3]) == (n - 1) * (P - 1) % P and int(out[100, 3]) == 0 and int(out[4000, 3]) == 0
    assert int(out[50, 3]) == 3 and int(out[51, 3]) == 0 and int(out[:, 3].astype(object).sum()) == int(out[7, 3]) + 3


def test_coefficients_flagged_scaled_and_shared_cells(ctx):
    rng = np.random.default_rng(43)
    n = 1 << 7
    table = np.arange(10, 10 + n, dtype=np.uint64)
    table[n // 2:] = table[:n // 2]                   # every value on two rows
    picks = rng.integers(0, n // 2, n)
    cons = np.stack([table[picks], np.ones(n, dtype=np.uint64)], axis=1)
    rnd = RNDS[1]
    # m = flag * (0 - M): rows with flag 0 keep their cells; their keys come from the other row that carries the value, or are reported
    flag = np.ones(n, dtype=np.uint64)
    flag[[0, 3, 9]] = 0                               # the second copy (rows n/2 + ...) provides
    flag[[5, n // 2 + 5]] = 0                         # nobody provides table[5]
    prov = np.stack([table, np.full(n, JUNK, dtype=np.uint64), flag], axis=1)
    w, (_, p_out), rep = against_reference(ctx, [consumer(), provider(flagged=True)], [cons, prov], [(1, 0, 0, 1)], rnd)
    assert w == n - 5 and (p_out[flag == 0, 1] == JUNK).all()
    looked_up_5 = int((picks == 5).sum())
    assert looked_up_5 > 0 and len(rep) == 1 and rep[0][1] == (looked_up_5, 0)
    counts = np.bincount(picks, minlength=n // 2)
    assert int(p_out[n // 2 + 3, 1]) == counts[3] and int(p_out[1, 1]) == counts[1] and int(p_out[n // 2 + 1, 1]) == 0
    # m = 3 * M: the cell is -net / 3
    prov = np.stack([table, np.full(n, JUNK, dtype=np.uint64)], axis=1)
    w, (_, p_out), rep = against_reference(ctx, [consumer(), provider(coeff=3)], [cons, prov], [(1, 0, 0, 1)], rnd)
    assert rep == [] and w == n and int(p_out[1, 1]) == (-int(counts[1]) * pow(3, P - 2, P)) % P
    # one cell feeding two fractions: the first slot decides; the second bus agrees (balanced) or does not (reported, not mis-filled)
    slots = [(1, 0, 0, 1), (1, 0, 1, 1)]
    agree = np.stack([cons[:, 0], cons[:, 1], cons[:, 0]], axis=1)
    w, (_, p_out), rep = against_reference(ctx, [consumer(second_bus=True), provider(second_bus=True)], [agree, prov], slots, rnd)
    assert rep == [] and w == n and (p_out[:n // 2, 1] == counts.astype(np.uint64)).all()
    differ = agree.copy()
    differ[0, 2] = table[(int(picks[0]) + 1) % (n // 2)]
    w, (_, p_out2), rep = against_reference(ctx, [consumer(second_bus=True), provider(second_bus=True)], [differ, prov], slots, rnd)
    assert len(rep) == 2 and (p_out2 == p_out).all()  # the first bus decided; both keys of the second are unmatched


# ---- 6: refusals ----
def test_refusals_leave_the_traces_unchanged(ctx):
    pkg = load_package()
    _, lookup = A.logup_air()
    good = A.logup_trace(4)
    rnd = RNDS[0]
    lb = dag.LookupBuilder(2, num_cols=1, num_randomness=1)
    lb.fraction(0, lb.randomness(0) * lb.main(1), lb.randomness(0) + lb.main(0))
    ef = dag.Lookup(lb, "ef_coefficient")
    lb = dag.LookupBuilder(2, num_cols=1, num_randomness=1)
    lb.fraction(0, -lb.main(1), lb.main(0))
    zd = dag.Lookup(lb, "zero_denominator")
    two = np.stack([np.arange(8, dtype=np.uint64), np.full(8, JUNK, dtype=np.uint64)], axis=1)  # row 0: denominator 0
    cases = [(lookup, good, [(0, 0, 0, 0)], "denominator reads a declared column.*instance 0 column 0 fraction 0|instance 0 column 0 fraction 0.*denominator"),
             (lookup, good, [(0, 0, 1, 0)], "undeclared reader.*instance 0 column 0 fraction 0"),
             (ef, two + np.uint64(1), [(0, 0, 0, 1)], "instance 0 column 0 fraction 0.*EF-valued"),
             (lookup, good, [(0, 0, 1, 8)], "out of range"), (lookup, good, [(0, 0, 4, 2)], "out of range"),
             (lookup, good, [(0, 2, 0, 2)], "out of range"), (lookup, good, [(1, 0, 1, 2)], "out of range"),
             (lookup, good, [(-1, 0, 1, 2)], "out of range"),
             (lookup, good, [(0, 0, 1, 2), (0, 0, 1, 3)], "two multiplicity slots.*instance 0 column 0 fraction 1"),
             (zd, two, [(0, 0, 0, 1)], "zero")]
    for lk, t, slots, reason in cases:
        dl, tr = pkg.DeviceLookup(ctx, lk), pkg.Trace(ctx, t)
        with pytest.raises(pkg.MidenHipError, match=reason):
            pkg.fill_multiplicities(ctx, [dl], [tr], slots, rnd)
        assert (tr.download() == t).all(), reason
        with pytest.raises(MR.Refused):
            MR.fill([lk.blob], [t], rnd, slots)
    with pytest.raises(pkg.MidenHipError):  # host matrices are not filled
        pkg.fill_multiplicities(ctx, [pkg.DeviceLookup(ctx, lookup)], [good], [(0, 0, 1, 2)], rnd)


# ---- 7: no slots = the exact balance check ----
def test_no_slots_is_the_exact_balance_check(ctx):
    pkg = load_package()
    _, lookup = A.logup_air()
    dl = pkg.DeviceLookup(ctx, lookup)
    for t in (A.logup_trace(8), A.logup_trace(8, valid=False)):
        tr = pkg.Trace(ctx, t)
        exp = pkg.check_balance(ctx, [dl], [tr], RNDS[0], exact=True)
        w, got = pkg.fill_multiplicities(ctx, [dl], [tr], [], RNDS[0])
        assert w == 0 and raw(got) == raw(exp) and (tr.download() == t).all()
    assert len(exp) == 2


# ---- 8: the shipped statements ----
def test_keccak_session_byte_pair_table(ctx):
    """The byte-pair table's three multiplicity columns from the consumers' pushes: the builder's ledger cell for cell (the table's keys
    are unique), then the session checks, proves and verifies."""
    pkg = load_package()
    pairs, traces, info = PT.precompile_session([b"abc"])
    root = info["public_root"]
    assert traces[3].shape == (PA.BPL_TRACE_HEIGHT, 3) and all((traces[3][:, c] != 0).any() for c in range(3))
    zeroed = [t.copy() for t in traces]
    zeroed[3][:] = 0
    pc = pkg.Precompile(ctx)
    trs = [ctx.upload_trace(t) for t in zeroed]
    assert pc.check_balance(trs, root, exact=True) != []
    slots = [(3,) + s for s in PA.BYTE_PAIR_LUT_MULT_SLOTS]
    w, rep = pc.fill_multiplicities(trs, root, slots)
    assert rep == [] and w == 3 * PA.BPL_TRACE_HEIGHT
    assert (trs[3].download() == traces[3]).all()
    assert all((tr.download() == t).all() for i, (tr, t) in enumerate(zip(trs, traces)) if i != 3)
    assert pc.check_balance(trs, root, exact=True) == [] and pc.check(trs, root) == []
    proof = pc.prove(trs, root)
    ok, dig = pkg.verify_precompile(pc.preprocessed_root(), root, proof.bytes)
    assert ok and (dig == proof.digest).all()


@pytest.mark.parametrize("case", [0, 12, 20])
def test_reference_snapshots_range_multiplicities(ctx, case):
    """RANGE_M of a reference snapshot, zeroed and filled: balanced, the constraints hold, every value's count is the original's; the
    cell equals the original's wherever its value sits on one row only (value 0 repeats above the table: the lowest row takes its count)."""
    pkg = load_package()
    c = RT.load_cases()[case]
    mats, pv, aux_in = [c["core"], c["chiplets"], c["poseidon2"]], RT.public_values(c), RT.aux_inputs(c)
    core = mats[0].copy()
    core[:, CO.RANGE_M] = JUNK
    m = pkg.Miden(ctx)
    trs = [ctx.upload_trace(t) for t in (core, mats[1], mats[2])]
    slots = [(0,) + s for s in CO.RANGE_M_MULT_SLOTS]
    w, rep = m.fill_multiplicities(trs, pv, aux_in, slots)
    assert rep == [] and w == core.shape[0]
    assert m.check(*trs, pv, aux_in) == []
    out = trs[0].download()
    keep = [k for k in range(core.shape[1]) if k != CO.RANGE_M]
    assert (out[:, keep] == mats[0][:, keep]).all()
    v, was, now = mats[0][:, CO.RANGE_V], mats[0][:, CO.RANGE_M], out[:, CO.RANGE_M]
    for val in np.unique(v):
        rows = np.nonzero(v == val)[0]
        assert int(now[rows].astype(object).sum()) == int(was[rows].astype(object).sum()), int(val)
        if len(rows) == 1:
            assert now[rows[0]] == was[rows[0]]
        else:
            assert (now[rows[1:]] == 0).all()


# ---- the C example ----
def table_air(log_n, seed=31):
    """tests/airs.py range_air with the table in the main trace: columns V (looked up), T (table), M (multiplicities); one bus
    sum_r 1 / (r0 + V_r + 2 r1) - M_r / (r0 + T_r + 2 r1).  -> (Air, Lookup, trace with M junk, the ledger's M)"""
    n = 1 << log_n

    def denoms(b):
        r0, r1 = b.randomness(0), b.randomness(1)
        return r0 + b.main(0) + r1 * 2, r0 + b.main(1) + r1 * 2, b.main(2)

    b = dag.AirBuilder(3, aux_width=1, num_randomness=2, num_aux_values=1)
    dV, dT, M = denoms(b)
    acc, acc_next = b.aux(0), b.aux(0, 1)
    own = dT - M * dV
    b.assert_zero_ext(b.is_transition() * ((acc_next - acc) * dV * dT - own))
    b.assert_zero_ext(b.is_first_row() * acc)
    b.assert_zero_ext(b.is_last_row() * ((b.aux_value(0) - acc) * dV * dT - own))
    lb = dag.LookupBuilder(3, num_cols=1, num_randomness=2)
    dV, dT, M = denoms(lb)
    lb.fraction(0, 1, dV)
    lb.fraction(0, -M, dT)
    rng = np.random.default_rng(seed)
    table = rng.permutation(np.arange(1, 4 * n, 4, dtype=np.uint64))[:n]
    picks = rng.integers(0, n, n)
    t = np.stack([table[picks], table, np.full(n, JUNK, dtype=np.uint64)], axis=1)
    return dag.Air(b, None, "table"), dag.Lookup(lb, "table"), t, np.bincount(picks, minlength=n).astype(np.uint64)


def test_c_example(ctx, tmp_path):
    """examples/fill_multiplicities_c_abi.c, built with gcc -Wall -Werror: fills, proves and verifies a table lookup (exit 0); with a
    looked-up value that is in no table row it prints the unmatched denominator and exits 1."""
    exe = str(tmp_path / "fill_multiplicities")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "fill_multiplicities_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    log_n = 6
    air, lookup, t, ledger = table_air(log_n)
    assert lookup.multiplicity_slots([2]) == [(0, 1, 2)]
    params = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=2, deep_pow_bits=3, num_queries=6, query_pow_bits=4)
    st, pre = protocol.challenger_state(), protocol.protocol_pre_observe(params, [])
    order = ("log_blowup", "log_folding_arity", "log_final_degree", "folding_pow_bits", "deep_pow_bits", "num_queries", "query_pow_bits")

    def write(trace, path):
        words = [log_n, 3, 0, 1, 2, len(air.blob), len(lookup.blob), len(pre)] + [params[k] for k in order] + [int(x) for x in st] + [int(x) for x in pre]
        with open(path, "wb") as f:
            f.write(np.array(words, dtype="<u8").tobytes())
            f.write(np.asarray(air.blob, dtype="<u8").tobytes())
            f.write(np.asarray(lookup.blob, dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(trace, dtype="<u8").tobytes())

    good, bad = str(tmp_path / "good.bin"), str(tmp_path / "bad.bin")
    write(t, good)
    wrong = t.copy()
    wrong[3, 0] = 2  # every table entry is 1 mod 4
    write(wrong, bad)
    r = subprocess.run([exe, good], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "balanced" in r.stdout and "verified" in r.stdout, r.stdout + r.stderr
    assert f"written {1 << log_n} cells of column 2, their sum {int(ledger.sum())}" in r.stdout, r.stdout
    r = subprocess.run([exe, bad], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "1 unmatched denominators" in r.stdout and f"their sum {int(ledger.sum()) - 1}" in r.stdout, r.stdout + r.stderr
