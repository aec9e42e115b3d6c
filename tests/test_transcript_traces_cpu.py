"""No GPU: the planners of the ChunkNode and TranscriptEval traces (mh_chunk_node_plan, mh_transcript_eval_plan,
csrc/transcript_traces_plan.cpp), testing.chunk_node_lists / transcript_lists, the ABI's declarations of the same records, and the device
stage's per-lane bodies (csrc/transcript_traces_rows.cuh) run lane by lane on the host (tools/libtranscript_traces_cpu.so, built by
__graft_entry__.build()) against the generators cell for cell -- on the ledgers and defects tests/test_gpu_transcript_traces.py gives the
device (tests/transcript_traces_cases.py).  The Poseidon2 trace is the generator's matrix in the device's layout."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import transcript_traces_cases as TC
from __graft_entry__ import ROOT

pkg = TC.pkg
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

P = pkg.P


def _vp(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


class HostBackend:
    """the planners, then the row bodies on the host, over the generator's Poseidon2 matrix"""

    def __init__(self):
        so = os.path.join(ROOT, "tools", "libtranscript_traces_cpu.so")
        assert os.path.exists(so), "tools/libtranscript_traces_cpu.so is missing: run __graft_entry__.build()"
        self.cpu = C.CDLL(so)
        self.cpu.chunk_node_cpu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                            C.POINTER(pkg.ChunkNodeInfo)]
        self.cpu.transcript_eval_cpu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.POINTER(pkg.TranscriptEvalInfo)]

    def p2(self, case):
        return TC.p2_host(case)

    def cn(self, p2, lists, log_n=-1):
        (cols, log_p2), (data, digests, rec) = p2, lists
        try:
            plan = pkg.chunk_node_plan(data, digests, rec, cols.shape[1] // 16, log_n)
        except pkg.MidenHipError as e:
            return 4, e.info, None
        out, info = np.full((42, int(plan.rows)), 0xdead, dtype=np.uint64), pkg.ChunkNodeInfo()
        rc = self.cpu.chunk_node_cpu(_vp(cols), log_p2, _vp(data), data.size, _vp(digests), _vp(rec), rec.size, log_n, _vp(out), C.byref(info))
        return (rc, info, None) if rc else (0, info, out.T)

    def te(self, p2, lists, log_n=-1):
        (cols, log_p2), (nodes, terms, limbs, root) = p2, lists
        try:
            _, plan = pkg.transcript_eval_plan(nodes, terms, limbs, root, cols.shape[1] // 16, log_n)
        except pkg.MidenHipError as e:
            return 4, e.info, None, None
        out, info, felts = np.full((39, int(plan.rows)), 0xdead, dtype=np.uint64), pkg.TranscriptEvalInfo(), np.zeros(4, dtype=np.uint64)
        rc = self.cpu.transcript_eval_cpu(_vp(cols), log_p2, _vp(nodes), nodes.size, _vp(terms), terms.size, _vp(limbs), limbs.shape[0], root, log_n,
                                          _vp(out), _vp(felts), C.byref(info))
        return (rc, info, None, None) if rc else (0, info, out.T, [int(x) for x in felts])


@pytest.fixture(scope="module")
def host():
    return HostBackend()


# ---- the lists ----
def test_lists_are_the_ledgers_of_the_session():
    c = TC.session_case()
    data, digests, rec = c.cn_lists
    assert bytes(data) == b"abc" + bytes(range(200)) and [int(x) for x in rec["len"]] == [0, 3, 200]
    assert [int(x) for x in rec["out_mult"]] == [1, 2, 1] and [int(x) for x in rec["chunk_head"]] == [0, 1, 2] and digests.shape == (3, 32)
    assert [bytes(d) for d in digests] == [r["keccak_digest"] for r in c.s.node.records]
    nodes, terms, limbs, root = c.te_lists
    assert nodes.size == 42 and set(int(k) for k in nodes["kind"]) == set(range(9)) - {pkg.TE_EC_PAI} and root == 41
    assert terms.size == 2 and limbs.shape == (int(((nodes["kind"] == pkg.TE_UINT_LEAF) | (nodes["kind"] == pkg.TE_UINT_PIN)).sum()), 8)
    ext = sorted(-1 - int(v) for f in ("lhs", "rhs") for v in nodes[f][nodes["kind"] == pkg.TE_AND] if v < 0)
    assert ext == sorted(int(rec["perm_keccak"][i]) for i in (0, 1, 1, 2))   # the four claims over three records: issued handles are cycles
    assert c.te_exp.shape == (64, 39) and c.cn_exp.shape == (16, 42)
    e = TC.edge_case()
    assert e.te_lists[0].size % 64 and e.cn_lists[2].size == 300 and e.te_exp.shape[1] == 39 and e.cn_exp.shape[0] == 2048


# ---- the planners ----
def test_planners_give_the_generators_heights_and_the_first_rows():
    for c in [TC.session_case(), TC.edge_case()] + TC.small_cases():
        info = pkg.chunk_node_plan(*c.cn_lists, c.p2_cycles)
        assert info.rows == info.rows_needed == c.cn_exp.shape[0] and info.n_records == c.cn_lists[2].size, c.name
        start, info = pkg.transcript_eval_plan(*c.te_lists, c.p2_cycles)
        active = int(c.te_exp[:, 0].sum())
        assert info.rows == info.rows_needed == max(2, 1 << (active - 1).bit_length()) and info.active_rows == active, c.name
        nodes, root = c.te_lists[0], c.te_lists[3]
        width = np.where(nodes["kind"] == pkg.TE_EC_MSM, nodes["rhs"], 1) * (nodes["kind"] != pkg.TE_ZERO)
        width[root] = 0
        assert list(start) == list(1 + np.concatenate([[0], np.cumsum(width)])[:-1]), c.name
    c = TC.session_case()
    assert pkg.chunk_node_plan(*c.cn_lists, c.p2_cycles, 24).rows == 1 << 24
    assert pkg.transcript_eval_plan(*c.te_lists, c.p2_cycles, 9)[1].rows == 512
    empty = pkg.chunk_node_plan(b"", np.zeros((0, 32), np.uint8), [], 1)
    assert (empty.rows, empty.n_chunks, empty.n_records) == (2, 0, 0)


def plan_refused(call, expect):
    with pytest.raises(pkg.MidenHipError) as e:
        call()
    i = e.value.info
    assert (i.defect_kind, i.defect_index, i.defect_operand) == expect, i


def test_every_chunk_node_planner_refusal_names_kind_index_and_operand():
    c = TC.session_case()
    data, digests, rec0 = c.cn_lists
    cyc = c.p2_cycles
    lib = pkg.load_library()
    lib.mh_chunk_node_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(pkg.ChunkNodeInfo)]
    for operand in range(3):                                             # 1: a NULL pointer, the pointers in order
        args = [_vp(data), data.size, _vp(digests), _vp(rec0), rec0.size]
        for slot in (0, 2, 3)[operand:]:
            args[slot] = None
        info = pkg.ChunkNodeInfo()
        assert lib.mh_chunk_node_plan(*args, cyc, -1, C.byref(info)) != 0
        assert (info.defect_kind, info.defect_index, info.defect_operand) == (1, 0, operand)
    assert lib.mh_chunk_node_plan(*[_vp(data), data.size, _vp(digests), _vp(rec0), rec0.size], cyc, -1, None) != 0

    def spoiled(i, **fields):
        rec = rec0.copy()
        for name, v in fields.items():
            rec[name][i] = v
        return lambda log_n=-1: pkg.chunk_node_plan(data, digests, rec, cyc, log_n)
    plan_refused(spoiled(2, len=201), (2, 2, 0))
    plan_refused(spoiled(1, offset=(1 << 64) - 1), (2, 1, 0))            # offset + len wraps
    plan_refused(spoiled(1, chunk_head=2), (3, 1, 0))
    plan_refused(spoiled(1, len=33, offset=0), (3, 2, 0))               # two chunks now: the next head is late
    plan_refused(spoiled(0, sponge_head=16), (4, 0, 0))
    plan_refused(spoiled(2, perm_chunks=cyc - 6), (5, 2, 0))             # 7 chunks from there run past the trace
    plan_refused(spoiled(2, perm_chunks=cyc), (5, 2, 0))
    plan_refused(spoiled(0, perm_digest_chunks=cyc), (5, 0, 1))
    plan_refused(spoiled(1, perm_keccak=1 << 63), (5, 1, 2))
    plan_refused(lambda: spoiled(0)(25), (6, 25, 0))
    plan_refused(lambda: spoiled(0)(3), (7, 16, 0))
    plan_refused(lambda: spoiled(0)(-2), (7, 16, 0))
    # more than 2^24 rows: 2^24 + 1 records of no bytes, chunk heads running
    n = (1 << 24) + 1
    many = np.zeros(n, dtype=pkg.KN_RECORD_DTYPE)
    many["chunk_head"] = np.arange(n)
    plan_refused(lambda: pkg.chunk_node_plan(b"", np.zeros((n, 32), np.uint8), many, 8), (6, n, 0))
    # one ledger, two defects: the lower kind, then the lower index
    rec = rec0.copy()
    rec["sponge_head"][0], rec["len"][2] = 1, 500
    plan_refused(lambda: pkg.chunk_node_plan(data, digests, rec, cyc), (2, 2, 0))
    rec["len"][2], rec["sponge_head"][1] = 200, 31
    plan_refused(lambda: pkg.chunk_node_plan(data, digests, rec, cyc), (4, 0, 0))


def test_every_transcript_planner_refusal_names_kind_index_and_operand():
    c = TC.session_case()
    nodes0, terms0, limbs, root = c.te_lists
    cyc, K = c.p2_cycles, pkg
    lib = pkg.load_library()
    lib.mh_transcript_eval_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int,
                                            C.c_void_p, C.POINTER(pkg.TranscriptEvalInfo)]
    for operand in range(3):
        args = [_vp(nodes0), nodes0.size, _vp(terms0), terms0.size, _vp(limbs), limbs.shape[0]]
        for slot in (0, 2, 4)[operand:]:
            args[slot] = None
        info = pkg.TranscriptEvalInfo()
        assert lib.mh_transcript_eval_plan(*args, root, cyc, -1, None, C.byref(info)) != 0
        assert (info.defect_kind, info.defect_index, info.defect_operand) == (1, 0, operand)

    def spoiled(i=0, terms=None, root_=root, **fields):
        nodes = nodes0.copy()
        for name, v in fields.items():
            nodes[name][i] = v
        return lambda log_n=-1: pkg.transcript_eval_plan(nodes, terms0 if terms is None else terms, limbs, root_, cyc, log_n)
    add, is_, leaf = TC._kind(nodes0, K.TE_UINT_OP, 1), TC._kind(nodes0, K.TE_UINT_OP, 4), TC._kind(nodes0, K.TE_UINT_LEAF)
    ec_add, msm, and_ = TC._kind(nodes0, K.TE_EC_OP, 1), TC._kind(nodes0, K.TE_EC_MSM), TC._kind(nodes0, K.TE_AND)
    plan_refused(spoiled(5, kind=9), (2, 5, 0))
    plan_refused(spoiled(add, op=0), (2, add, 1))
    plan_refused(spoiled(add, op=5), (2, add, 1))
    plan_refused(spoiled(ec_add, op=4), (2, ec_add, 1))
    plan_refused(spoiled(add, lhs=add), (3, add, 0))                    # itself
    plan_refused(spoiled(add, rhs=-1), (3, add, 1))                     # an external binding anywhere but under an AND
    plan_refused(spoiled(and_, lhs=and_ + 1), (3, and_, 0))
    plan_refused(spoiled(leaf, lhs=limbs.shape[0]), (3, leaf, 0))
    plan_refused(spoiled(ec_add, rhs=41), (3, ec_add, 1))
    plan_refused(spoiled(msm, rhs=0), (3, msm, 1))
    plan_refused(spoiled(msm, rhs=3), (3, msm, 0))
    plan_refused(spoiled(msm, lhs=-1), (3, msm, 0))
    t0 = int(nodes0["lhs"][msm])
    bad = terms0.copy()
    bad["scalar_node"][t0 + 1] = msm
    plan_refused(spoiled(terms=bad), (3, t0 + 1, 3))
    bad = terms0.copy()
    bad["base_node"][t0] = 0xffffffff
    plan_refused(spoiled(terms=bad), (3, t0, 2))
    plan_refused(spoiled(root_=42), (4, 42, 0))
    plan_refused(spoiled(root_=leaf), (4, leaf, 0))
    plan_refused(spoiled(root_=msm), (4, msm, 0))
    plan_refused(spoiled(leaf, perm=cyc), (5, leaf, 0))
    plan_refused(spoiled(msm, perm=cyc - 1), (5, msm, 0))                # its last cycle is past the trace
    ext_and, f = next((a, f) for a in range(nodes0.size) for f in ("lhs", "rhs") if nodes0["kind"][a] == K.TE_AND and nodes0[f][a] < 0)
    plan_refused(spoiled(ext_and, **{f: -1 - cyc}), (5, ext_and, 1 if f == "lhs" else 2))
    plan_refused(spoiled(ext_and, **{f: -(1 << 63)}), (5, ext_and, 1 if f == "lhs" else 2))
    plan_refused(lambda: spoiled()(25), (6, 25, 0))
    plan_refused(lambda: spoiled()(5), (7, 64, 0))
    # more than 2^24 rows: one MSM claim over 2^24 term rows, every term the same two nodes
    n = 1 << 24
    big = np.zeros(3, dtype=K.TE_NODE_DTYPE)
    big["kind"] = [K.TE_ZERO, K.TE_UINT_LEAF, K.TE_EC_MSM]
    big["rhs"][2] = n
    plan_refused(lambda: pkg.transcript_eval_plan(big, np.zeros(n, dtype=K.TE_TERM_DTYPE), np.zeros((1, 8), np.uint32), 0, n), (6, n + 2, 0))
    # two defects: the lower kind first
    two = nodes0.copy()
    two["perm"][leaf], two["op"][is_] = cyc, 9
    plan_refused(lambda: pkg.transcript_eval_plan(two, terms0, limbs, root, cyc), (2, is_, 1))


# ---- the ABI ----
def test_abi_agrees_across_header_rust_python_and_library():
    doc = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    lib = pkg.load_library()
    entries = ("mh_chunk_node_plan", "mh_chunk_node_trace_build", "mh_transcript_eval_plan", "mh_transcript_eval_trace_build")
    for f in entries:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h) and re.search(r"pub fn " + f + r"\s*\(", rs) and f in pkg.EXPORTS and hasattr(lib, f), f
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    rust_c = {"u32": "uint32_t", "u64": "uint64_t", "i32": "int32_t", "i64": "int64_t"}

    def header(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name, h, flags=re.S).group(1)
        return [(d.split()[0], n.strip()) for d in body.split(";") if d.strip() for n in d.split(None, 1)[1].split(",")]
    for name, (dt, size) in {"mh_kn_record": (pkg.KN_RECORD_DTYPE, 64), "mh_te_node": (pkg.TE_NODE_DTYPE, 64), "mh_te_term": (pkg.TE_TERM_DTYPE, 8)}.items():
        assert dt.itemsize == size and [n for n, _ in rust(name)] == list(dt.names), name
        assert [(rust_c[t], n) for n, t in rust(name)] == header(name), name
        at = 0
        for n, t in rust(name):                                         # the C layout: every field naturally aligned, no padding
            width = 4 if t.endswith("32") else 8
            assert at % width == 0 and dt.fields[n][1] == at and dt.fields[n][0].itemsize == width, (name, n)
            at += width
        assert at == size, name
    ctype = {C.c_uint64: ("u64", "uint64_t"), C.c_int32: ("i32", "int32_t")}
    for name, cls, size in (("mh_chunk_node_info", pkg.ChunkNodeInfo, 56), ("mh_transcript_eval_info", pkg.TranscriptEvalInfo, 80)):
        assert rust(name) == [(n, ctype[t][0]) for n, t in cls._fields_] and header(name) == [(ctype[t][1], n) for n, t in cls._fields_], name
        assert C.sizeof(cls) == size, name
    args = lambda name: [x.split()[-1].lstrip("*") for x in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    for f in entries:
        assert args(f) == rargs(f), f
    assert args("mh_chunk_node_trace_build") == ["ctx", "p2", "bytes", "n_bytes", "digests", "records", "n", "log_n", "out", "info"]
    assert args("mh_transcript_eval_trace_build") == ["ctx", "p2", "nodes", "n_nodes", "terms", "n_terms", "limbs", "n_lit", "root", "log_n", "out",
                                                      "root_felts", "info"]
    for f in ("chunk_node_trace", "transcript_eval_trace"):
        assert callable(getattr(pkg, f)) and callable(getattr(pkg, f[:-5] + "plan")) and callable(getattr(pkg.Ctx, f)) and callable(getattr(pkg.Precompile, f))
    assert callable(PT.chunk_node_lists) and callable(PT.transcript_lists)


# ---- the row bodies, lane by lane on the host ----
def test_row_bodies_give_the_sessions_traces(host):
    info = TC.check(host, TC.session_case())
    assert (info.n_nodes, info.n_terms, info.rows, info.n_zero) == (42, 2, 64, 1)


def test_row_bodies_give_the_edge_ledgers_cells(host):
    c = TC.edge_case()
    info = TC.check(host, c)
    assert info.n_nodes % 64 and info.active_rows % 64 and info.rows == 1024 and c.cn_lists[2].size == 300 and c.s.p2.next_seq % 64


@pytest.mark.parametrize("which", range(4), ids=["pinned_root", "zero_root", "zeros_merged", "ec_sub"])
def test_row_bodies_give_the_small_cases_cells(host, which):
    c = TC.small_cases()[which]
    TC.check(host, c)
    if which < 3:                                                        # no record: height 2, both counters from 0
        assert c.cn_exp.shape == (2, 42) and c.cn_lists[2].size == 0
    if which == 2:
        assert c.te_exp.shape == (4, 39) and c.te_exp[3, 14] == 1 and c.te_exp[3, 15] == 4      # three ANDs, then the merged ZERO row


def test_row_bodies_pad(host):
    TC.check(host, TC.session_case(), log_cn=6, log_te=8)
    TC.check(host, TC.small_cases()[0], log_cn=3, log_te=3)


def test_checking_pass_refuses_every_device_kind(host):
    c = TC.session_case()
    p2 = host.p2(c)
    te = TC.te_device_defects(c)
    assert {d[2] for d in te} == set(range(8, 16))
    for what, lists, kind, index, operand in te:
        TC.refused(host.te(p2, lists), kind, index, operand)
    cn = TC.cn_device_defects(c)
    assert {d[2] for d in cn} == {8, 9}
    for what, lists, kind, index, operand in cn:
        TC.refused(host.cn(p2, lists), kind, index, operand)
