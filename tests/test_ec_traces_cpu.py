"""No GPU: the planner of the EC traces (mh_ec_traces_plan, csrc/ec_traces_plan.cpp), testing.ec_lists, the ABI's four declarations of
the same records, and the device stage's per-lane bodies (csrc/ec_traces_rows.cuh) run lane by lane on the host
(tools/libec_traces_cpu.so, built by __graft_entry__.build()) against the generators cell for cell -- on the ledgers and defects
tests/test_gpu_ec_traces.py gives the device (tests/ec_traces_cases.py)."""
import copy
import ctypes as C
import os
import re
import numpy as np
import pytest
import ec_traces_cases as EC
from __graft_entry__ import ROOT

pkg = EC.pkg
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

P = pkg.P
LEAST = (-1, -1, -1, -1)


@pytest.fixture(scope="module")
def sessions():
    return EC.session_cases()


def _vp(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


@pytest.fixture(scope="module")
def build():
    """-> build(lists, logs) -> (rc, info, four matrices or None): the planner, then the row bodies on the host"""
    so = os.path.join(ROOT, "tools", "libec_traces_cpu.so")
    assert os.path.exists(so), "tools/libec_traces_cpu.so is missing: run __graft_entry__.build()"
    cpu = C.CDLL(so)
    cpu.ec_traces_cpu.argtypes = [C.c_void_p, C.c_size_t] * 5 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.POINTER(pkg.EcTracesInfo)]

    def run(ls, logs):
        try:
            _, plan = pkg.ec_traces_plan(*ls, *logs)
        except pkg.MidenHipError as e:
            return 4, e.info, None
        outs = [np.full((w, int(n)), 0xdead, dtype=np.uint64) for w, n in zip(EC.WIDTHS, (plan.groups_rows, plan.points_rows, plan.add_rows, plan.msm_rows))]
        info = pkg.EcTracesInfo()
        rc = cpu.ec_traces_cpu(*[v for r in ls for v in (_vp(r), r.size)], *logs, *[_vp(o) for o in outs], C.byref(info))
        return (rc, info, None) if rc else (0, info, [o.T for o in outs])
    return run


# ---- the planner ----
def test_planner_gives_the_generators_heights_and_the_first_rows(sessions):
    for name, ls, exp in sessions:
        row_start, info = pkg.ec_traces_plan(*ls)
        assert (info.n_groups, info.n_points, info.n_add, info.n_exprs, info.n_terms) == tuple(x.size for x in ls)
        needed = (info.groups_rows_needed, info.points_rows_needed, info.add_rows_needed, info.msm_rows_needed)
        assert needed == (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows)
        for n, e in zip(needed, exp):
            assert e is None or n == e.shape[0], (name, needed)
        assert list(row_start) == list(np.concatenate([[0], np.cumsum(ls[3]["n_rows"])])[:-1].astype(np.int64)) if ls[3].size else row_start.size == 0
    assert list(pkg.ec_traces_plan(*sessions[2][1])[0]) == [0, 1, 2, 3, 5, 7, 9]
    _, info = pkg.ec_traces_plan(*sessions[2][1], log_groups=3, log_points=3, log_add=7, log_msm=24)
    assert (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows, info.msm_rows_needed) == (8, 8, 128, 1 << 24, 16)
    _, info = pkg.ec_traces_plan([], [], [], [], [])
    assert (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows) == (2, 2, 4, 2)


def plan_refused(ls, expect, logs=LEAST):
    with pytest.raises(pkg.MidenHipError) as e:
        pkg.ec_traces_plan(*ls, *logs)
    i = e.value.info
    assert (i.defect_section, i.defect_kind, i.defect_index, i.defect_operand) == expect, i


def test_every_planner_refusal_names_section_kind_index_and_operand(sessions):
    base = sessions[2][1]                                               # points 1 at infinity, 2, 3 members, 4..7 certified; 7 expressions, 11 rows
    lib = pkg.load_library()
    lib.mh_ec_traces_plan.argtypes = [C.c_void_p, C.c_size_t] * 5 + [C.c_int] * 4 + [C.c_void_p, C.POINTER(pkg.EcTracesInfo)]
    # 1: a NULL list with a nonzero count, the lists in order
    for section, operand, slot in ((0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 3), (3, 1, 4)):
        args = [v for r in base for v in (_vp(r), r.size)]
        for s in range(slot, 5):
            args[2 * s] = None
        info = pkg.EcTracesInfo()
        assert lib.mh_ec_traces_plan(*args, -1, -1, -1, -1, None, C.byref(info)) != 0
        assert (info.defect_section, info.defect_kind, info.defect_index, info.defect_operand) == (section, 1, 0, operand)
    # 2: more than 2^24 rows (the count alone is read), or a log above 24
    for section, slot, n in ((0, 0, (1 << 24) + 1), (1, 1, (1 << 24) + 1), (2, 2, (1 << 22) + 1), (3, 4, (1 << 24) + 1)):
        args = [v for r in base for v in (_vp(r), r.size)]
        args[2 * slot + 1] = n
        info = pkg.EcTracesInfo()
        assert lib.mh_ec_traces_plan(*args, -1, -1, -1, -1, None, C.byref(info)) != 0
        assert (info.defect_section, info.defect_kind, info.defect_index) == (section, 2, n)
    plan_refused(base, (2, 2, 25, 0), (-1, -1, 25, -1))
    # 3: a log below the need
    plan_refused(base, (0, 3, 2, 0), (0, -1, -1, -1))
    plan_refused(base, (1, 3, 8, 0), (-1, 2, 4, 3))
    plan_refused(base, (2, 3, 32, 0), (-1, -1, 4, 3))
    plan_refused(base, (3, 3, 16, 0), (-1, -1, -1, 3))

    def spoiled(which, i, **fields):
        ls = [x.copy() for x in base]
        for name, v in fields.items():
            ls[which][name][i] = v
        return ls
    plan_refused(spoiled(1, 4, group=0), (1, 4, 4, 0))
    plan_refused(spoiled(1, 2, group=2), (1, 4, 2, 0))
    plan_refused(spoiled(1, 3, kind=3), (1, 5, 3, 0))
    plan_refused(spoiled(1, 0, y_ptr=9), (1, 5, 0, 2))
    plan_refused(spoiled(1, 0, w_ptr=9), (1, 5, 0, 4))
    plan_refused(spoiled(1, 5, u_ptr=9), (1, 5, 5, 3))
    plan_refused(spoiled(3, 2, kind=3), (3, 6, 2, 0))
    plan_refused(spoiled(3, 4, n_rows=0), (3, 6, 4, 1))
    plan_refused(spoiled(3, 1, n_rows=2), (3, 6, 1, 1))
    plan_refused(spoiled(3, 6, n_rows=3), (3, 6, 7, 2))
    plan_refused(spoiled(3, 3, a_expr=0), (3, 7, 3, 0))
    plan_refused(spoiled(3, 3, a_expr=4), (3, 7, 3, 0))                 # expression 3 is pointer 4: itself
    plan_refused(spoiled(3, 5, b_expr=7), (3, 7, 5, 1))
    plan_refused(spoiled(3, 0, b_expr=1), (3, 7, 0, 1))                 # an intro has no operand
    neg = spoiled(3, 6, kind=2)                                         # a neg names one operand
    plan_refused(neg, (3, 7, 6, 1))
    # one ledger, two defects: the lower kind
    two = spoiled(3, 3, a_expr=0)
    two[1]["group"][6] = 5
    plan_refused(two, (1, 4, 6, 0))
    two[3]["kind"][5] = 9
    plan_refused(two, (1, 4, 6, 0))
    two[1]["group"][6] = 1
    plan_refused(two, (3, 6, 5, 0))


# ---- ec_lists ----
def test_ec_lists_round_trip_and_the_demand_the_generators_recorded(sessions):
    name, (g, p, a, e, t), (groups, points, add, msm) = sessions[2]
    # the records are the ledgers'
    assert [tuple(int(x) for x in r) for r in g] == [tuple(PA.FIXED_EC_GROUPS[0][1:]) + (1,)]      # the verifier's boundary read
    assert [int(x) for x in p["kind"]] == [1, 0, 0, 2, 2, 2, 2] and int(p["ext_reads"].sum()) == 1 and int(p["ext_reads"][6]) == 1
    assert [int(x) for x in a["kind"]] == [4, 4, 4, 5, 5] and [int(x) for x in a["mints"]] == [0, 1, 1, 1, 1]
    assert [int(x) for x in e["kind"]] == [0, 0, 1, 1, 1, 1, 1] and int(e["ext_mult"].sum()) == 0 and [int(x) for x in e["claim_mult"]] == [0] * 6 + [1]
    assert [(int(b), int(s)) for b, s in t] == [(int(r[PA.MS_COL_BASE]), int(r[PA.MS_COL_SCALAR])) for r in msm[:11]]
    # ext_reads plus the implied demand is the generators' column
    live = a["kind"] >= 3
    implied_g = np.bincount(p["group"], minlength=2)[1:] + np.bincount(a["group"][live], minlength=2)[1:] + np.bincount(e["group"][e["kind"] != 0], minlength=2)[1:]
    assert [int(x) for x in (g["ext_reads"] + implied_g.astype(np.uint64))] == [int(x) for x in groups[:1, 5]]
    implied_p = np.bincount(np.concatenate([a["p"], a["q"], a["r"][live]]), minlength=8)[1:]
    assert [int(x) for x in (p["ext_reads"] + implied_p.astype(np.uint64))] == [int(x) for x in points[:7, PA.EP_COL_ECPOINT_MULT]]
    uses = np.bincount(np.concatenate([e["a_expr"], e["b_expr"]]), minlength=8)[1:]
    firsts = [int(x) for x in np.concatenate([[0], np.cumsum(e["n_rows"])])[:-1]]
    assert [int(x) for x in (e["ext_mult"] + uses.astype(np.uint64))] == [int(msm[r, PA.MS_COL_MULT]) for r in firsts]
    # before the generators have run, the same lists come from the ledgers as they stand
    led = EC.sub_neg_ledger()
    before = EC.lists(led)
    after = copy.deepcopy(led)
    bpl = PT.BytePairLutRequires()
    PT.ec_msm_trace(after.msm, after.store, bpl)
    PT.ec_group_add_trace(after.ec_add, after.ec, bpl)
    for x, y in zip(before, PT.ec_lists(after.ec, after.ec_add, after.msm, own_reads_recorded=True)):
        assert x.tobytes() == y.tobytes()
    assert int(before[1]["ext_reads"][0]) == 1                           # EcRequire.neg's read of the point at infinity


# ---- the ABI ----
def test_abi_agrees_across_header_rust_python_and_library():
    doc = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    lib = pkg.load_library()
    for f in ("mh_ec_traces_plan", "mh_ec_traces_build"):
        assert re.search(r"\bint\s+" + f + r"\s*\(", h) and re.search(r"pub fn " + f + r"\s*\(", rs) and f in pkg.EXPORTS and hasattr(lib, f), f
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    rust_c = {"u32": "uint32_t", "u64": "uint64_t", "i32": "int32_t", "[u32; 6]": "uint32_t"}

    def header(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name, h, flags=re.S).group(1)
        return [(d.split()[0], n.strip().split("[")[0]) for d in body.split(";") if d.strip() for n in d.split(None, 1)[1].split(",")]
    layouts = {"mh_ec_group": (pkg.EC_GROUP_DTYPE, 24), "mh_ec_point": (pkg.EC_POINT_DTYPE, 32), "mh_ec_add_op": (pkg.EC_ADD_OP_DTYPE, 56),
               "mh_msm_expr": (pkg.MSM_EXPR_DTYPE, 48), "mh_msm_term": (pkg.MSM_TERM_DTYPE, 8)}
    for name, (dt, size) in layouts.items():
        assert dt.itemsize == size and dt.isalignedstruct is False, name
        assert [n for n, _ in rust(name)] == list(dt.names) and [(rust_c[t], n) for n, t in rust(name)] == header(name), name
        offsets, at = [], 0
        for n, t in rust(name):                                        # the C layout: every field is naturally aligned without padding
            width = {"u32": 4, "u64": 8, "[u32; 6]": 24}[t]
            assert at % min(width, 8) == 0, (name, n)
            offsets.append(at)
            at += width
        assert [dt.fields[n][1] for n in dt.names] == offsets and at == size, name
    ctype = {C.c_uint64: ("u64", "uint64_t"), C.c_int32: ("i32", "int32_t")}
    assert rust("mh_ec_traces_info") == [(n, ctype[t][0]) for n, t in pkg.EcTracesInfo._fields_]
    assert header("mh_ec_traces_info") == [(ctype[t][1], n) for n, t in pkg.EcTracesInfo._fields_]
    assert C.sizeof(pkg.EcTracesInfo) == 128 and pkg.EcTracesInfo.defect_index.offset == 112
    args = lambda name: [x.split()[-1].lstrip("*") for x in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    common = ["groups", "n_groups", "points", "n_points", "adds", "n_add", "exprs", "n_exprs", "terms", "n_terms", "log_groups", "log_points", "log_add", "log_msm"]
    assert args("mh_ec_traces_plan") == rargs("mh_ec_traces_plan") == common + ["row_start", "info"]
    assert args("mh_ec_traces_build") == rargs("mh_ec_traces_build") == ["ctx"] + common + ["groups_out", "points_out", "add_out", "msm_out", "info"]
    assert callable(pkg.ec_traces_plan) and callable(pkg.ec_traces) and callable(pkg.Ctx.ec_traces) and callable(pkg.Precompile.ec_traces) and callable(PT.ec_lists)


# ---- the row bodies, lane by lane on the host ----
def test_row_bodies_give_the_sessions_traces(build, sessions):
    for name, ls, exp in sessions:
        rc, info, got = build(ls, LEAST)
        assert rc == 0, info
        for what, g, e in zip(EC.NAMES, got, exp):
            if e is not None:
                EC.same(g, e, name + " " + what)


@pytest.mark.parametrize("ledger", [EC.sub_neg_ledger, EC.edges_ledger, EC.two_groups_ledger, EC.large_multiplicities_ledger], ids=lambda f: f.__name__)
def test_row_bodies_give_the_generators_cells(build, ledger):
    EC.check(build, ledger())


def test_row_bodies_pad_and_lay_empty_lists(build):
    led = EC.sub_neg_ledger()
    EC.check(build, led, (3, 5, 6, 4))
    empty = EC.ledgers(k1_group=False)
    empty.ec.groups.clear()
    got, _ = EC.check(build, empty)
    assert [g.shape[0] for g in got] == [2, 2, 4, 2]


def test_checking_pass_refuses_every_device_kind(build):
    cases = EC.device_defects()
    assert {c[3] for c in cases} == set(range(8, 16))
    for what, ls, section, kind, index, operand in cases:
        EC.refused(build, ls, section, kind, index, operand)
