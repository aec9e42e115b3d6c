"""GPU: the range-check table laid on the device (mh_fill_range_table*, csrc/range_table.hip), run with -m gpu.

The Miden statement is held to the reference processor's snapshots and to the host generator of testing/core_trace.py, cell for cell;
the generic entry to tests/range_table_ref.py (the header's semantics over Python integers) on a three-column test AIR."""
import numpy as np
import pytest
import balance_ref as BR
import range_airs as RA
import range_table_ref as RR
import ref_traces as RT
from __graft_entry__ import load_package
from miden_vm_amd import core_air as CO
from miden_vm_amd.testing import core_trace as CV

pytestmark = pytest.mark.gpu
pkg = load_package()
CASES = RT.load_cases()
N = 1 << 7


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def info_dict(info):
    return dict(n_values=info.n_values, rows_needed=info.rows_needed, rows_available=info.rows_available)


def against_reference(ctx, lookups, mains, boundary=(), slot=RA.SLOT):
    """The library against range_table_ref.fill: every cell of every trace, the info, the report entry for entry.  -> (filled, report)"""
    exp_info, exp_out, exp_rep = RR.fill([lk.blob for lk in lookups], mains, RA.RND, slot, boundary=boundary)
    dls = [pkg.DeviceLookup(ctx, lk) for lk in lookups]
    trs = [pkg.Trace(ctx, m) for m in mains]
    rep, info = pkg.fill_range_table(ctx, dls, trs, slot, RA.RND, boundary=boundary)
    out = [t.download() for t in trs]
    for a, b in zip(out, exp_out):
        assert (a == b).all(), np.argwhere(a != b)[:8]
    assert info_dict(info) == exp_info
    assert BR.as_report(rep) == exp_rep
    return out, exp_rep


# ---- the Miden statement ----
@pytest.mark.parametrize("c", CASES, ids=[str(c["case"]) for c in CASES])
def test_reference_snapshots_cell_for_cell(ctx, c):
    """Both range columns junked: after the call the core trace is the reference processor's in every cell."""
    m = pkg.Miden(ctx)
    pv, aux_in = RT.public_values(c), RT.aux_inputs(c)
    trs = [ctx.upload_trace(t) for t in (RA.junked(c["core"]), c["chiplets"], c["poseidon2"])]
    rep, info = m.fill_range_table(trs, pv, aux_in)
    assert rep == []
    out = trs[0].download()
    assert (out == c["core"]).all(), np.argwhere(out != c["core"])[:8]
    assert (trs[1].download() == c["chiplets"]).all() and (trs[2].download() == c["poseidon2"]).all()
    assert info.rows_available == c["core"].shape[0] and info.rows_needed <= info.rows_available
    assert m.check(*trs, pv, aux_in) == []


PROGRAMS = [("u32mem", 1, 6), ("u32mem", 2, 7), ("u32mem", 5, 8), ("u32mem", 8, 9), ("bench", 8, 10)]


@pytest.mark.parametrize("kind,iters,log_core", PROGRAMS)
def test_executed_programs_equal_the_host_generator(ctx, kind, iters, log_core):
    """u32 operations and memory traffic on the test VM: the device's two columns are the host ledger's (range_table(range_lookups))."""
    vm = CV.CoreVM(stack_inputs=tuple(range(16)))
    r = CV.prove_inputs(vm, RA.u32_memory_program(iters) if kind == "u32mem" else CV.bench_program(iters))
    core, pv, aux_in = r["core"], r["public_values"], r["aux_inputs"]
    assert core.shape[0] == 1 << log_core
    m = pkg.Miden(ctx)
    trs = [pkg.Trace(ctx, t) for t in (RA.junked(core), r["chiplets"], r["poseidon2"])]
    rep, info = m.fill_range_table(trs, pv, aux_in)
    out = trs[0].download()
    assert rep == [] and (out == core).all(), np.argwhere(out != core)[:8]
    assert info_dict(info) == dict(n_values=len(vm.range_lookups), rows_needed=len(CV.range_table(vm.range_lookups)), rows_available=core.shape[0])
    if log_core == 6:  # the proof over the filled traces is the proof over the host-built ones
        got = m.prove(*trs, pv, aux_in)
        exp = m.prove(*[pkg.Trace(ctx, t) for t in (core, r["chiplets"], r["poseidon2"])], pv, aux_in)
        assert got.bytes == exp.bytes
        ok, dig = pkg.verify_miden(pv, aux_in, got.bytes)
        assert ok and (dig == got.digest).all()


def test_miden_info_and_host_matrices(ctx):
    """The info of the Miden entry is the snapshot's table (a looked-up value has a count; 0 and 65535 are present without one); host
    matrices are not filled."""
    c = CASES[0]
    m = pkg.Miden(ctx)
    trs = [ctx.upload_trace(t) for t in (RA.junked(c["core"]), c["chiplets"], c["poseidon2"])]
    _, info = m.fill_range_table(trs, RT.public_values(c), RT.aux_inputs(c))
    v, cnt = c["core"][:, CO.RANGE_V], c["core"][:, CO.RANGE_M]
    present = {int(x) for x in v[np.nonzero(cnt)[0]]} | {0, 65535}
    assert info_dict(info) == dict(n_values=len(present), rows_needed=RR.rows_needed(present), rows_available=len(v))
    with pytest.raises(pkg.MidenHipError):
        m.fill_range_table([c["core"], c["chiplets"], c["poseidon2"]], RT.public_values(c), RT.aux_inputs(c))  # host matrices are not filled


# ---- gap corners through the generic entry ----
CORNERS = {
    "zero": [0], "max": [65535], "one_two_three": [1, 2, 3],
    "around_3^7": [2186, 2187, 2188], "twice_3^7": [4374],
    "word_seam": [63, 64], "wave_seam": [4095, 4096], "workgroup_seam": [16383, 16384],
    "last_word": [65471, 65472, 65534],
}


@pytest.mark.parametrize("name", list(CORNERS))
def test_gap_corners(ctx, name):
    (out,), rep = against_reference(ctx, [RA.table_lookup()], [RA.table_trace(CORNERS[name], N)])
    assert rep == []
    present = set(CORNERS[name]) | {0, 65535}
    need = RR.rows_needed(present)
    assert [int(x) for x in out[N - need:, RA.V]] == RR.table_values(present)
    assert int(out[:, RA.M].astype(object).sum()) == N


def test_one_value_from_two_instances_and_the_boundary(ctx):
    """Value 300 is looked up by the table's own instance, by a second instance and by a boundary push; 77 by the boundary alone."""
    main = RA.table_trace([300, 5], N)
    other = np.array([[300], [9], [300], [65535]] * 16, dtype=np.uint64)
    boundary = [(RA.e_key(300), 1), (RA.e_key(77), 1)]
    (out, _), rep = against_reference(ctx, [RA.table_lookup(), RA.consumer_lookup()], [main, other], boundary=boundary)
    assert rep == []
    count = {int(v): int(m) for v, m in zip(out[:, RA.V], out[:, RA.M]) if m}
    assert count == {300: N // 2 + 32 + 1, 5: N // 2, 9: 16, 65535: 16, 77: 1}
    # the table may sit in the second instance of the statement as well
    (_, out2), rep = against_reference(ctx, [RA.consumer_lookup(), RA.table_lookup()], [other, main], boundary=boundary, slot=(1,) + RA.SLOT[1:])
    assert rep == [] and (out2 == out).all()


def test_dense_table(ctx):
    """2^12 distinct values in a 2^13-row trace: every lane of the rows kernel's first waves has values, gaps 1, 3 and 9 need no bridge."""
    rng = np.random.default_rng(7)
    values = np.cumsum(rng.choice([1, 3, 9], 1 << 12))
    assert len(set(values)) == 1 << 12 and values[-1] < 1 << 16
    main = RA.table_trace(rng.permutation(values), 1 << 13)
    (out,), rep = against_reference(ctx, [RA.table_lookup()], [main])
    assert rep == [] and len(np.unique(out[:, RA.V])) > 1 << 12


# ---- refusals ----
def test_refused_when_the_table_does_not_fit(ctx):
    values = np.arange(0, 2 * N, 2)
    main = RA.table_trace(values, N)
    dl, tr = pkg.DeviceLookup(ctx, RA.table_lookup()), pkg.Trace(ctx, main)
    with pytest.raises(pkg.MidenHipError, match="range table needs") as e:
        pkg.fill_range_table(ctx, [dl], [tr], RA.SLOT, RA.RND)
    present = set(int(x) for x in values) | {65535}
    assert info_dict(e.value.info) == dict(n_values=len(present), rows_needed=RR.rows_needed(present), rows_available=N)
    assert e.value.info.rows_needed > N
    assert tr.download().tobytes() == main.tobytes()
    with pytest.raises(RR.Refused):
        RR.fill([RA.table_lookup().blob], [main], RA.RND, RA.SLOT)
    # the caller sizes the trace by the info and calls again
    tall = RA.table_trace(values, 1 << int(e.value.info.rows_needed - 1).bit_length())
    against_reference(ctx, [RA.table_lookup()], [tall])


def test_a_lookup_of_65536_is_an_unmatched_push(ctx):
    main = RA.table_trace([5, 6], N)
    main[9, RA.C] = 65536
    (out,), rep = against_reference(ctx, [RA.table_lookup()], [main])
    assert len(rep) == 1 and rep[0][0] == RA.e_key(65536) and [p[:2] for p in rep[0][2]] == [(0, 9)]
    assert 65536 not in set(int(x) for x in out[:, RA.V])
    assert [int(x) for x in out[N - RR.rows_needed({0, 5, 6, 65535}):, RA.V]] == RR.table_values({0, 5, 6, 65535})


@pytest.mark.parametrize("kind,reason,where", [("rowwise_g", "denominator is not", "fraction 1"), ("rowwise_d0", "denominator is not", "fraction 1"),
                                               ("reader", "undeclared reader", "fraction 0"), ("mult", "multiplicity reads the value column", "fraction 1")])
def test_refused_declarations_write_nothing(ctx, kind, reason, where):
    lk = RA.table_lookup(kind)
    main = RA.table_trace([5, 6, 7, 2000], N)
    dl, tr = pkg.DeviceLookup(ctx, lk), pkg.Trace(ctx, main)
    with pytest.raises(pkg.MidenHipError, match=reason) as e:
        pkg.fill_range_table(ctx, [dl], [tr], RA.SLOT, RA.RND)
    assert "instance 0 column 0 " + where in str(e.value)
    assert tr.download().tobytes() == main.tobytes()
    with pytest.raises(RR.Refused):
        RR.fill([lk.blob], [main], RA.RND, RA.SLOT)


def test_slots_out_of_range_are_refused(ctx):
    main = RA.table_trace([5], N)
    dl, tr = pkg.DeviceLookup(ctx, RA.table_lookup()), pkg.Trace(ctx, main)
    for slot in ((1, 0, 1, 0, 1), (-1, 0, 1, 0, 1), (0, 1, 0, 0, 1), (0, 0, 2, 0, 1), (0, 0, 1, 3, 1), (0, 0, 1, 0, 3), (0, 0, 1, 1, 1)):
        with pytest.raises(pkg.MidenHipError, match="range slot"):
            pkg.fill_range_table(ctx, [dl], [tr], slot, RA.RND)
        assert tr.download().tobytes() == main.tobytes()


# ---- determinism ----
def test_two_calls_leave_the_same_bytes(ctx):
    rng = np.random.default_rng(11)
    main = RA.table_trace(rng.integers(0, 1 << 16, 40), 1 << 11)
    main[:, :2] = rng.integers(0, RA.P, (1 << 11, 2), dtype=np.uint64)
    dl = pkg.DeviceLookup(ctx, RA.table_lookup())
    outs = []
    for _ in range(2):
        tr = pkg.Trace(ctx, main)
        rep, info = pkg.fill_range_table(ctx, [dl], [tr], RA.SLOT, RA.RND)
        assert rep == []
        outs.append(tr.download().tobytes())
        rep, _ = pkg.fill_range_table(ctx, [dl], [tr], RA.SLOT, RA.RND)   # and a call on its own output changes nothing
        assert rep == [] and tr.download().tobytes() == outs[-1]
    assert outs[0] == outs[1]
