"""Ledgers, expectations and defects shared by tests/test_ec_traces_cpu.py (the row bodies run lane by lane on the host) and
tests/test_gpu_ec_traces.py (mh_ec_traces_build on the device): both must give the generators' cells and the same refusals.  Not a test
module."""
import copy
import types
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

P = pkg.P
NAMES = ("groups", "points", "add", "msm")
WIDTHS = (6, 14, 21, 38)


def same(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert (got == exp).all(), (what, [(int(r), int(c), int(got[r, c]), int(exp[r, c])) for r, c in np.argwhere(got != exp)[:8]])


def ledgers(k1_group=True):
    """the session's EC and uint ledgers over the fixed environment, the secp256k1 group created (its point at infinity stored)"""
    led = types.SimpleNamespace(store=PT.UintStore().install_fixed_uints(), adds=PT.UintAddRequires(), muls=PT.UintMulRequires(), ec=PT.EcStore(),
                                ec_add=PT.EcAddRequires())
    led.req = PT.EcRequire(led.ec, led.store, led.muls, led.adds, led.ec_add)
    led.msm = PT.EcMsmRequires(led.req)
    if k1_group:
        led.group, led.pai = led.req.create_group(0, 7, PA.K1_BASE_BOUND_PTR)
    return led


def generator(led, heights=(0, 0, 0, 0)):
    """the three generators, in `Session.finish` order, on a copy of the ledgers (they route their demand into them)
    -> (groups, points, add, msm)"""
    c = copy.deepcopy(led)
    bpl = PT.BytePairLutRequires()
    msm = PT.ec_msm_trace(c.msm, c.store, bpl, min_height=heights[3])
    add = PT.ec_group_add_trace(c.ec_add, c.ec, bpl, min_height=heights[2])
    # one min_height for both stores: lay them twice where the two heights differ
    groups = PT.ec_store_traces(c.ec, min_height=heights[0])[0]
    points = PT.ec_store_traces(c.ec, min_height=heights[1])[1]
    return groups, points, add, msm


def lists(led):
    return PT.ec_lists(led.ec, led.ec_add, led.msm)


def check(build, led, logs=(-1, -1, -1, -1)):
    """build(lists, logs) -> (rc, info, four matrices); they must be the generators', cell for cell -> (matrices, info)"""
    exp = generator(led, tuple((1 << l) if l >= 0 else 0 for l in logs))
    ls = lists(led)
    rc, info, got = build(ls, logs)
    assert rc == 0, info
    for name, g, e in zip(NAMES, got, exp):
        same(g, e, name)
    assert (info.n_groups, info.n_points, info.n_add, info.n_exprs, info.n_terms, info.defect_kind) == tuple(x.size for x in ls) + (0,)
    assert (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows) == tuple(g.shape[0] for g in got)
    return got, info


def refused(build, ls, section, kind, index, operand, logs=(-1, -1, -1, -1)):
    rc, info, got = build(ls, logs)
    assert rc != 0 and got is None, "a defective ledger must be refused"
    assert (info.defect_section, info.defect_kind, info.defect_index, info.defect_operand) == (section, kind, index, operand), info
    return info


# ---- the sessions of the issue: their ledgers after the generators have run (own reads subtracted) ----
def session_cases():
    """-> [(name, lists, (groups, points, add or None, msm or None))] for ec_store_session(5), ec_add_session([5, 6]) and
    ec_msm_session([(5, 1), (3, 2)]), laid at the least heights"""
    out = []
    _, tr, (_store, _muls, ec) = PT.ec_store_session(5, min_height=0)
    out.append(("store", PT.ec_lists(ec, None, None, own_reads_recorded=True), (tr[1], tr[0], None, None)))
    _, tr, (_res, (_store, _adds, _muls, ec, ec_add)) = PT.ec_add_session([5, 6], min_height=0)
    assert {op["case"] for op, _ in ec_add.ops} >= {"double", "generic", "pai_p", "pai_both"} and any(m == 2 for _, m in ec_add.ops)
    out.append(("add", PT.ec_lists(ec, ec_add, None, own_reads_recorded=True), (tr[3], tr[4], tr[5], None)))
    _, tr, (_val, _acc, (_store, _adds, _muls, ec, ec_add, msm)) = PT.ec_msm_session([(5, 1), (3, 2)], min_height=0)
    rows = [r for e in msm.exprs for r in e["rows"]]
    assert (len(ec.points), len(ec_add.ops), sum(op["mints"] for op, _ in ec_add.ops), len(msm.exprs), len(rows)) == (7, 5, 4, 7, 11)
    assert any(r["take_a"] for r in rows) and any(r["take_b"] for r in rows) and any(r["take_both"] for r in rows)
    out.append(("msm", PT.ec_lists(ec, ec_add, msm, own_reads_recorded=True), (tr[3], tr[4], tr[5], tr[6])))
    return out


# ---- hand-built ledgers ----
def sub_neg_ledger():
    """EcRequire.sub (pai_q: R + PAI = P; a chord), EcRequire.neg (cancel, with its read of the point at infinity) and EcMsmRequires.neg
    twice: one whose value point is minted, one that deduplicates onto a stored point"""
    led = ledgers()
    mult = PT.k1_multiples(4)
    g1, g2, g3 = (led.req.add_point(led.group, *mult[i]) for i in range(3))
    assert led.req.sub(g1, led.pai, 1) == g1                            # pai_q
    assert led.req.sub(g3, g1, 2) == g2                                 # G2 + G1 = G3: a chord
    _, neg_g2, _ = led.req.neg(g2, 1)                                   # cancel; -G2 is stored from here on
    e1, e2 = led.msm.intro(g1), led.msm.intro(g2)
    c = led.msm.combine(e1, e2)
    n1 = led.msm.neg(e1)                                                # -G1 is minted
    n2 = led.msm.neg(e2)                                                # -G2 deduplicates onto the stored row
    led.msm.neg(c)
    led.msm.resolve(n1)
    assert {op["case"] for op, _ in led.ec_add.ops} >= {"cancel", "pai_q"}
    assert (led.msm.exprs[n1 - 1]["neg_minted"], led.msm.exprs[n2 - 1]["neg_minted"], led.msm.exprs[n2 - 1]["val"]) == (1, 0, neg_g2)
    led.ec.require_fixed_groups()
    return led


def edges_ledger(n_points=257, n_adds=65, n_terms=300):
    """wave and block edges: `n_points` stored points, `n_adds` additions, an expression of `n_terms` terms built by a balanced tree of
    combines over as many intros (its rows cross a 256-lane block, the binary searches run deep), and combine(a, a).  The points are
    multiples of G bound by value; the additions chain on from the last of them, every result minted."""
    led = ledgers()
    mult = PT.k1_multiples(n_terms)
    pts = [led.req.add_point(led.group, *xy) for xy in mult]
    acc = pts[-1]                                                       # past the stored multiples: every sum is minted
    for _ in range(n_adds):
        acc = led.req.add(acc, pts[0], 1)
    level = [led.msm.intro(p) for p in pts]
    while len(level) > 1:
        level = [led.msm.combine(level[i], level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    top = level[0]
    assert len(led.msm.terms(top)) == n_terms
    led.msm.combine(top, top)
    led.msm.resolve(top)
    assert len(led.ec.points) >= n_points and len(led.ec_add.ops) >= n_adds
    return led


def two_groups_ledger():
    """a second group over the same modulus (y^2 = x^3 + 5: its points are not checked by value here, only stored), points interleaved"""
    led = ledgers()
    g2, pai2 = led.req.create_group(0, 5, PA.K1_BASE_BOUND_PTR)
    led.req.constrain_scalar_bound(g2, PA.K1_SCALAR_BOUND_PTR)
    mult = PT.k1_multiples(4)
    bound = led.ec.group_params(g2)[2]
    a1 = led.req.add_point(led.group, *mult[0])
    b1 = led.ec.add_point_cert(g2, led.store.intern(11, bound), led.store.intern(12, bound))[0]
    a2 = led.req.add_point(led.group, *mult[1])
    b2 = led.ec.add_point_cert(g2, led.store.intern(13, bound), led.store.intern(14, bound))[0]
    led.req.add(a1, a2, 1)
    led.req.add(a1, a1, 3)
    led.req.add(pai2, b1, 1)                                            # pai_p in the second group
    led.req.add(b2, pai2, 1)                                            # pai_q
    e1, e2 = led.msm.intro(b1), led.msm.intro(b2)
    led.msm.intro(a1)
    assert led.ec.point_params(b1)[0] == g2 and e1 != e2
    led.ec.require_fixed_groups()
    led.ec.require_ecgroup(g2)
    return led


def large_multiplicities_ledger():
    """demand words just below 2^64 on a group, a point, an addition and an expression; a point whose outside reads are p - 1 with one
    more read by an addition (the sum wraps to 0)"""
    led = sub_neg_ledger()
    recorded = sum(1 for g, _ in led.ec.points if g == led.group) + sum(1 for e in led.msm.exprs if e["kind"] != "intro")
    led.ec.group_demand[led.group] = (1 << 64) - 1 + recorded            # ext_reads = 2^64 - 1: the recorders' own reads come on top
    led.ec_add.ops[0][1] = (1 << 64) - 1
    led.ec_add.ops[1][1] = P
    led.msm.exprs[0]["mult"] += (1 << 64) - 3
    led.msm.exprs[1]["claim_mult"] = (1 << 64) - 1
    wrap = led.req.add_point(led.group, *PT.k1_multiples(4)[3])         # read by exactly one addition below, as q
    led.req.add(led.pai, wrap, 1)
    led.ec.point_demand[wrap] = P - 1
    led.ec.point_demand[led.pai] = led.ec.point_demand.get(led.pai, 0) + (1 << 64) - 2
    return led




# ---- defects the device's checking pass finds (kinds 8..15) ----
def _bases():
    """A: sub_neg_ledger (additions 0 pai_q, 1 and 3 chords, 2 cancel, no mint; expressions 0, 1 intros of points 2, 3, 2 their
    combine, 3, 4 their negs, 5 the combine's neg over term rows 6, 7).  B: ec_msm_session([(5, 1), (3, 2)]) (points 1 at infinity,
    2, 3 members, 4..7 certified; additions 0 a double onto a stored row, 1, 2 minting doubles, 3 = 5 + 2 -> 6 and 4 = 6 + 3 -> 7 minting
    chords; expressions 0, 1 intros, 2..6 combines, 6 = combine(6, 2) over term rows 9, 10 with bases 2, 3).  C: two_groups_ledger
    (three intros nobody uses)."""
    return dict(A=lists(sub_neg_ledger()), B=session_cases()[2][1], C=lists(two_groups_ledger()))


def device_defects():
    """-> [(what, lists, section, kind, index, operand)]: every device kind, spoiled in copies of the record arrays"""
    bases, out = _bases(), []

    def spoil(what, base, expect, fn):
        g, p, a, e, t = (x.copy() for x in bases[base])
        out.append((what, fn(g, p, a, e, t) or (g, p, a, e, t)) + expect)

    def put(arr, i, **fields):
        for name, v in fields.items():
            arr[name][i] = v

    def second_group(g, p, a, e, t, **spoils):
        g2 = np.concatenate([g, g])
        for name, (arr, i) in dict(point=(p, spoils.get("point")), expr=(e, spoils.get("expr"))).items():
            if i is not None:
                arr["group"][i] = 2
        return g2, p, a, e, t
    spoil("8: an addition's q above n_points", "B", (2, 8, 1, 1), lambda g, p, a, e, t: put(a, 1, q=8))
    spoil("8: an addition's r 0, a later one's p too", "B", (2, 8, 0, 2), lambda g, p, a, e, t: (put(a, 0, r=0), put(a, 2, p=0)) and None)
    spoil("8: an addition's group above n_groups", "B", (2, 8, 2, 3), lambda g, p, a, e, t: put(a, 2, group=2))
    spoil("8: an expression's val 0", "B", (3, 8, 3, 0), lambda g, p, a, e, t: put(e, 3, val=0))
    spoil("8: an expression's group above n_groups", "B", (3, 8, 2, 1), lambda g, p, a, e, t: put(e, 2, group=9))
    spoil("8 in both sections: the additions first", "B", (2, 8, 1, 0), lambda g, p, a, e, t: (put(e, 0, group=9), put(a, 1, p=99)) and None)
    spoil("9: an addition kind 6", "B", (2, 9, 1, 0), lambda g, p, a, e, t: put(a, 1, kind=6))
    spoil("9: mints 2", "B", (2, 9, 1, 1), lambda g, p, a, e, t: put(a, 1, mints=2))
    spoil("9: mints on a pai_q", "A", (2, 9, 0, 1), lambda g, p, a, e, t: put(a, 0, mints=1))
    spoil("11 at a low index and 9 at a high one: 9", "A", (2, 9, 3, 0), lambda g, p, a, e, t: (put(a, 0, kind=5), put(a, 3, kind=7)) and None)
    spoil("10: a result stored under another group", "B", (2, 10, 1, 2), lambda g, p, a, e, t: second_group(g, p, a, e, t, point=3))
    spoil("10: an expression under another group than its val's", "B", (3, 10, 1, 0), lambda g, p, a, e, t: second_group(g, p, a, e, t, expr=1))
    spoil("11: a pai_q recorded as generic", "A", (2, 11, 0, 0), lambda g, p, a, e, t: put(a, 0, kind=5))
    spoil("11: a double recorded as pai_p", "B", (2, 11, 1, 0), lambda g, p, a, e, t: put(a, 1, kind=0, mints=0))
    spoil("12: mints with r <= p", "B", (2, 12, 1, 0), lambda g, p, a, e, t: put(a, 1, r=3))
    spoil("12: mints with r <= q", "B", (2, 12, 3, 1), lambda g, p, a, e, t: put(a, 3, q=6))
    spoil("12: mints onto a member row", "B", (2, 12, 0, 2), lambda g, p, a, e, t: put(a, 0, mints=1))
    spoil("13: bases 2, 2", "B", (3, 13, 4, 0), lambda g, p, a, e, t: put(t, 4, base=2))
    spoil("14: a first row neither operand holds", "B", (3, 14, 9, 0), lambda g, p, a, e, t: put(t, 9, base=1))
    spoil("14: the walk jumps an operand's term (the row before the foreign base)", "B", (3, 14, 9, 1), lambda g, p, a, e, t: put(t, 10, base=5))
    spoil("14: a neg row that is not its operand's", "A", (3, 14, 5, 2), lambda g, p, a, e, t: put(t, 5, base=2))
    spoil("15: an intro whose val is not its base", "C", (3, 15, 2, 0), lambda g, p, a, e, t: put(t, 2, base=1))
    return out
