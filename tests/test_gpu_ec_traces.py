"""The precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces built on the device (run with -m gpu): mh_ec_traces_build
(csrc/ec_traces.hip) against the in-tree generators testing/precompile_trace.ec_store_traces / ec_group_add_trace / ec_msm_trace cell
for cell -- the three sessions, sub / neg ledgers, wave and block edges, two groups, padding, empty lists, multiplicities that wrap --
every device refusal by section, kind, index and operand, and a session whose traces 3..6 come from the device through to a byte-equal
proof.  Every build is made twice and must leave the same bytes.  The ledgers and defects are tests/ec_traces_cases.py's, shared with
the host-side run of the same row bodies (tests/test_ec_traces_cpu.py)."""
import ctypes as C
import numpy as np
import pytest
import oracle_binding as ob
import ec_traces_cases as EC

pkg = EC.pkg
from miden_vm_amd import protocol, precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu
P = pkg.P
UNTOUCHED = 0x1234


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def _vp(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


def builder(ctx):
    """-> build(lists, logs): mh_ec_traces_build on the ABI's own arguments, TWICE -> (rc, info, four matrices or None).  The out pointers
    of a refused call keep the value they had; an accepted call's second run leaves the same bytes."""
    lib = ctx.lib
    lib.mh_ec_traces_build.argtypes = [C.c_void_p] + [C.c_void_p, C.c_size_t] * 5 + [C.c_int] * 4 + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(pkg.EcTracesInfo)]

    def build(ls, logs):
        runs = []
        for _ in range(2):
            hs, info = [C.c_void_p(UNTOUCHED) for _ in range(4)], pkg.EcTracesInfo()
            rc = lib.mh_ec_traces_build(ctx.h, *[v for r in ls for v in (_vp(r), r.size)], *logs, *[C.byref(h) for h in hs], C.byref(info))
            if rc != 0:
                assert all(h.value == UNTOUCHED for h in hs), "a refusal leaves the out pointers alone"
                msg = lib.mh_last_error(ctx.h).decode()
                assert f"section {info.defect_section}, defect {info.defect_kind}, index {info.defect_index}, operand {info.defect_operand}" in msg, msg
                return rc, info, None
            rows = (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows)
            trs = [pkg.Trace.from_handle(ctx, h, int(n).bit_length() - 1, w) for h, n, w in zip(hs, rows, EC.WIDTHS)]
            runs.append([t.download() for t in trs])
            for t in trs:
                t.free()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), "a second call leaves the same bytes"
        return 0, info, runs[0]
    return build


@pytest.fixture(scope="module")
def sessions():
    return EC.session_cases()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["ec_store_session", "ec_add_session", "ec_msm_session"])
def test_session_ledgers_give_the_sessions_traces(ctx, sessions, which):
    """ec_store_session(5), ec_add_session([5, 6]) (double, generic, pai_p, pai_both, multiplicities of 2) and
    ec_msm_session([(5, 1), (3, 2)]) (four mints, all three take_* forms): the ledgers after the generators have run"""
    name, ls, exp = sessions[which]
    rc, info, got = builder(ctx)(ls, (-1, -1, -1, -1))
    assert rc == 0, info
    for what, g, e in zip(EC.NAMES, got, exp):
        if e is not None:
            EC.same(g, e, name + " " + what)
    if exp[2] is None:                                                  # no additions, no expressions: the all-padding forms
        assert got[2].shape == (4, 21) and not got[2].any()
        EC.same(got[3], PT.ec_msm_trace(PT.EcMsmRequires(None), None, None), "msm of no expression")


def test_sub_neg_and_msm_neg(ctx):
    """cancel, pai_q, a neg expression whose value point is minted and one that deduplicates onto a stored row"""
    EC.check(builder(ctx), EC.sub_neg_ledger())


def test_wave_and_block_edges(ctx):
    """65 minted additions chained past the stored points, more than 257 points, an expression of 300 terms over a balanced tree of
    combines (its rows cross a 256-lane block; 3196 term rows in all), combine(a, a)"""
    got, info = EC.check(builder(ctx), EC.edges_ledger())
    assert info.n_points > 257 and info.n_add >= 65 and info.n_points % 64 and info.n_add % 64 and info.n_terms % 256


def test_two_groups_with_points_interleaved(ctx):
    EC.check(builder(ctx), EC.two_groups_ledger())


def test_padding_and_empty_lists(ctx):
    build = builder(ctx)
    led = EC.sub_neg_ledger()
    EC.check(build, led, (3, 5, 6, 4))
    EC.check(build, led, (-1, 4, -1, 7))
    ls = EC.lists(led)
    for s, logs, need in ((0, (0, -1, -1, -1), 2), (1, (-1, 2, -1, -1), 8), (2, (-1, -1, 3, -1), 16), (3, (-1, -1, -1, 2), 8)):
        EC.refused(build, ls, s, 3, need, 0, logs)
    empty = EC.ledgers(k1_group=False)
    empty.ec.groups.clear()
    got, info = EC.check(build, empty)
    assert [g.shape[0] for g in got] == [2, 2, 4, 2] and (info.n_groups, info.n_points, info.n_add, info.n_exprs, info.n_terms) == (0,) * 5


def test_large_multiplicities_reduce_mod_p(ctx):
    """ext_reads, mult, ext_mult and claim_mult words just below 2^64, a mult of exactly p, and p - 1 outside reads plus one by an
    addition: the column holds 0"""
    led = EC.large_multiplicities_ledger()
    got, _ = EC.check(builder(ctx), led)
    wrap = len(led.ec.points)
    assert got[1][wrap - 1, PA.EP_COL_ECPOINT_MULT] == 0 and got[1][wrap - 1, PA.EP_COL_PTR] == wrap
    assert got[2][4 + PA.EA_ROW_TERM, 0] == 0                          # the addition whose mult is p


def test_every_device_refusal_names_section_kind_index_and_operand(ctx):
    build = builder(ctx)
    cases = EC.device_defects()
    assert {c[3] for c in cases} == set(range(8, 16))
    for what, ls, section, kind, index, operand in cases:
        EC.refused(build, ls, section, kind, index, operand)
    EC.check(build, EC.sub_neg_ledger())                               # the context goes on


def host_aux(lookup, main, randomness, preprocessed=None):
    return ob.lookup_build_aux(lookup, main, randomness, preprocessed)


def test_ec_msm_session_with_device_built_ec_traces_proves_the_same_bytes(ctx):
    import test_gpu_precompile as GP
    from test_precompile_ec_add import FAST
    pairs, traces, (_val, _acc, (_store, _adds, _muls, ec, ec_add, msm)) = PT.ec_msm_session([(5, 1), (3, 2)], host_aux)
    airs_, lookups = [p[0] for p in pairs], [p[1] for p in pairs]
    ls = PT.ec_lists(ec, ec_add, msm, own_reads_recorded=True)
    logs = [traces[i].shape[0].bit_length() - 1 for i in (3, 4, 5, 6)]
    built, info = ctx.ec_traces(*ls, *logs)
    for t, i in zip(built, (3, 4, 5, 6)):
        EC.same(t.download(), traces[i], EC.NAMES[i - 3])

    def prove(device_traces):
        dairs = [pkg.DeviceAir(ctx, x) for x in airs_]
        raw = ctx.upload_trace(airs_[0].preprocessed)
        com = pkg.commit_traces(ctx, [raw], FAST["log_blowup"])
        dairs[0].attach_preprocessed(com.tree(), 0, raw=raw)
        for d, lk in zip(dairs, lookups):
            d.attach_lookup(pkg.DeviceLookup(ctx, lk))
        st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
        pre = protocol.protocol_pre_observe(FAST, GP.ROOT, preprocessed_root=com.root())
        return pkg.prove(ctx, dairs, device_traces, GP.ROOT, FAST, st, pre, GP.never), com.root(), st, pre

    trs = [ctx.upload_trace(t) for t in traces]
    trs[3:7] = built
    got, root, st, pre = prove(trs)
    uploaded, _, _, _ = prove([ctx.upload_trace(t) for t in traces])
    assert bytes(got.bytes) == bytes(uploaded.bytes)
    ok, dig = pkg.verify(airs_, got.log_trace_heights, GP.ROOT, FAST, st, pre, got.fields, got.commitments, preprocessed_root=root,
                         external=PA.external_assertions(pkg, fixed_uints=True))
    assert ok and (dig == got.digest).all()
