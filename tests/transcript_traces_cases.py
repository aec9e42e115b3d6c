"""Ledgers, expectations and defects shared by tests/test_transcript_traces_cpu.py (the row bodies run lane by lane on the host, the
Poseidon2 trace the generator's) and tests/test_gpu_transcript_traces.py (mh_chunk_node_trace_build / mh_transcript_eval_trace_build on the
device, the Poseidon2 trace built there with digest references): both must give the generators' cells and the same refusals.  A backend
is an object with p2(case) -> its Poseidon2 trace, cn(p2, lists, log_n) -> (rc, info, matrix or None) and te(p2, lists, log_n) ->
(rc, info, matrix or None, root felts or None).  Not a test module."""
import functools
import types
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

P = pkg.P
FP, GROUP = PA.K1_BASE_BOUND_PTR, PA.K1_GROUP_PTR
M = PA.K1_BOUND + 1
SESSION_INPUTS = [b"", b"abc", b"abc", bytes(range(200))]


def same(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert (got == exp).all(), (what, [(int(r), int(c), int(got[r, c]), int(exp[r, c])) for r, c in np.argwhere(got != exp)[:8]])


def case(name, s, root, min_height=0):
    """a recorded `Session` and its root -> the lists both builders take, the generators' two matrices, the Poseidon2 ledger"""
    c = types.SimpleNamespace(name=name, s=s, root=root)
    c.te_exp, c.public_root = PT.transcript_eval_trace(s.eval, root, min_height=min_height)
    c.cn_exp = PT.chunk_node_trace(s.chunk, s.node)
    c.cn_lists = PT.chunk_node_lists(s.chunk, s.node)
    c.te_lists = PT.transcript_lists(s.eval, root)
    c.p2_cycles = max(1, 1 << max(0, (s.p2.next_seq - 1).bit_length())) if s.p2.next_seq else 1
    return c


def p2_host(c):
    """the generator's Poseidon2 chiplet matrix, column-major as the device holds it -> (uint64 [32, height], log height)"""
    if not hasattr(c, "_p2_host"):
        m, _ = PT.poseidon2_chiplet_trace(c.s.p2)
        c._p2_host = (np.ascontiguousarray(m.T), m.shape[0].bit_length() - 1)
    return c._p2_host


def p2_lists(c):
    """the Poseidon2 ledger as mh_poseidon2_chiplet_trace_build takes it, digests as REFERENCES: no permutation on the host"""
    absorptions, blocks, refs = c.s.p2.lists(refs=True)
    return np.array(absorptions, dtype=pkg.P2C_ABSORPTION_DTYPE).reshape(-1), blocks, refs


def point(s, mult, k):
    return s.ec_create(GROUP, s.uint_leaf(mult[k - 1][0], FP), s.uint_leaf(mult[k - 1][1], FP))


@functools.lru_cache(maxsize=None)
def session_case():
    """precompile_session(SESSION_INPUTS): 42 nodes of every kind but PAI, 3 node records (one read twice, one of 7 chunks and 2 sponge
    blocks); 64 x 39 and 16 x 42"""
    _, traces, out = PT.precompile_session(SESSION_INPUTS)
    s = out["session"]
    root = next(dict(id=n["id"], hash=n["hash"]) for n in reversed(s.eval.nodes) if n["id"] in s.eval.live)
    c = case("session", s, root, min_height=8)
    same(c.te_exp, traces[5], "the session's eval trace")
    same(c.cn_exp, traces[0], "the session's chunk/node trace")
    c.traces, c.out = traces, out
    return c


@functools.lru_cache(maxsize=None)
def edge_case():
    """300 Keccak claims of lengths 0..299 (across the 32-byte chunk and 136-byte block boundaries) and a repeated empty input, a 130-step
    uint_add chain closed by an `is`, 70 created points, P + pai is P, a 70-term MSM claimed in reversed order (its run crosses a wave), a
    pin: no size is a multiple of 64 or 256"""
    s = PT.Session()
    claims = [s.keccak(bytes((7 * i + j) & 0xff for j in range(i)))[1] for i in range(300)]
    claims.append(s.keccak(b"")[1])
    x = s.uint_leaf(PA.K1_G[0], FP)
    acc = x
    for _ in range(130):
        acc = s.uint_add(acc, x)
    claims.append(s.uint_is(acc, s.uint_leaf(131 * PA.K1_G[0] % M, FP)))
    mult = PT.k1_multiples(70)
    pts = [point(s, mult, k) for k in range(1, 71)]
    claims.append(s.ec_is(s.ec_add(pts[4], s.ec_pai(GROUP)), pts[4]))
    e = None
    for p in pts:
        intro = s.msm_intro(p)
        e = intro if e is None else s.msm_combine(e, intro)
    by_base = dict(s.msm.terms(e))
    msm_node = s.ec_msm(e, [(p, s.eval.uint_leaf(by_base[p["point"]])) for p in reversed(pts)])
    vx, vy = s.msm_value_coords(e)
    claims.append(s.ec_is(msm_node, s.ec_create(GROUP, s.uint_leaf(vx, FP), s.uint_leaf(vy, FP))))
    claims.append(s.pin_uint(100, (PA.K1_G[0] * 3 + 1) % M, FP))
    return case("edge", s, s.assert_and_fold(claims))


def small_cases():
    """a lone pinned root (no AND); a ZERO root; several zeros merged; ec_sub; an empty record list comes with all but the last"""
    out = []
    s = PT.Session()
    out.append(case("pinned root", s, s.pin_uint(100, 12345, FP)))
    s = PT.Session()
    out.append(case("zero root", s, s.zero()))
    s = PT.Session()
    z = [s.zero() for _ in range(4)]
    out.append(case("zeros merged", s, s.assert_and(s.assert_and(s.assert_and(z[0], z[1]), z[2]), z[3])))
    s = PT.Session()
    mult = PT.k1_multiples(12)
    sub = s.ec_is(s.ec_sub(point(s, mult, 12), point(s, mult, 7)), point(s, mult, 5))
    out.append(case("ec_sub", s, s.assert_and_fold([sub, s.keccak(b"sub")[1]])))
    return out


def check(backend, c, log_cn=-1, log_te=-1):
    """both builds of a case against the generators' matrices (padded by the generators' rule where a log is given)"""
    p2 = backend.p2(c)
    rc, info, got = backend.cn(p2, c.cn_lists, log_cn)
    assert rc == 0, (c.name, info)
    exp = c.cn_exp
    if log_cn >= 0:                                                      # the generator pads the chunk side to a least height
        chunk = PT.chunk_trace(c.s.chunk, 1 << log_cn)
        exp = np.zeros((chunk.shape[0], PA.CN_COLS), dtype=np.uint64)
        exp[:, :PA.CHUNK_COLS] = chunk
        exp[:c.cn_exp.shape[0], PA.CHUNK_COLS:] = c.cn_exp[:, PA.CHUNK_COLS:]
    same(got, exp, c.name + " chunk/node")
    rc, info, got, root = backend.te(p2, c.te_lists, log_te)
    assert rc == 0, (c.name, info)
    exp = c.te_exp if log_te < 0 else PT.transcript_eval_trace(c.s.eval, c.root, min_height=1 << log_te)[0]
    same(got, exp, c.name + " eval")
    assert root == c.public_root, c.name
    return info


def refused(result, kind, index, operand):
    rc, info = result[0], result[1]
    assert rc != 0 and result[2] is None, info
    assert (info.defect_kind, info.defect_index, info.defect_operand) == (kind, index, operand), info


# ---- defects the device's checking pass finds, on the session's lists ----
def _kind(nodes, kind, op=None, nth=0):
    hits = [i for i in range(nodes.size) if nodes["kind"][i] == kind and (op is None or nodes["op"][i] == op)]
    return hits[nth]


def session_marks(c):
    """cycles of the session's Poseidon2 ledger the defects point at: the 7-chunk chain's first cycle, a one-block absorption's"""
    rec = c.cn_lists[2]
    long_ = int(np.argmax(rec["len"]))
    return types.SimpleNamespace(long=long_, chain=int(rec["perm_chunks"][long_]), short=int(np.argmin(rec["len"] + (rec["len"] == 0) * 1000)))


def te_device_defects(c):
    """-> [(what, (nodes, terms, limbs, root), kind, index, operand)]"""
    nodes0, terms0, limbs, root = c.te_lists
    m = session_marks(c)
    out = []

    def spoil(what, kind, index, operand, root_=root, terms=None, append=None, **fields):
        nodes = nodes0.copy()
        for name, (i, v) in fields.items():
            nodes[name][i] = v
        if append is not None:
            nodes = np.concatenate([nodes, append])
        out.append((what, (nodes, terms0 if terms is None else terms, limbs, root_), kind, index, operand))
    K = pkg
    add, is_, leaf, pin = _kind(nodes0, K.TE_UINT_OP, 1), _kind(nodes0, K.TE_UINT_OP, 4), _kind(nodes0, K.TE_UINT_LEAF), _kind(nodes0, K.TE_UINT_PIN)
    create, ec_add, msm = _kind(nodes0, K.TE_EC_CREATE), _kind(nodes0, K.TE_EC_OP, 1), _kind(nodes0, K.TE_EC_MSM)
    ands = [i for i in range(nodes0.size) if nodes0["kind"][i] == K.TE_AND]
    first_and = ands[0]
    assert pin < create and leaf < add
    t0 = int(nodes0["lhs"][msm])
    # 8: the wrong class
    spoil("a value under an AND", 8, first_and, 1, rhs=(first_and, leaf))
    spoil("a truthy node under a create", 8, create, 0, lhs=(create, pin))
    spoil("a uint node under an EC op", 8, ec_add, 1, rhs=(ec_add, leaf))
    spoil("an EC node under a create", 8, _kind(nodes0, K.TE_EC_CREATE, nth=1), 0, lhs=(_kind(nodes0, K.TE_EC_CREATE, nth=1), create))
    bad = terms0.copy()
    bad["base_node"][t0 + 1] = leaf
    spoil("a uint node as an MSM base", 8, t0 + 1, 2, terms=bad)
    bad = terms0.copy()
    bad["scalar_node"][t0] = create
    spoil("an EC node as an MSM scalar", 8, t0, 3, terms=bad)
    # 9: different moduli
    spoil("a uint op under another modulus than its operands", 9, add, 0, bound_ptr=(add, int(nodes0["bound_ptr"][add]) + 1))
    spoil("a create under another modulus", 9, create, 0, bound_ptr=(create, 1))
    spoil("an MSM whose scalars lie under another bound", 9, t0, 3, bound_ptr=(msm, int(nodes0["bound_ptr"][msm]) + 1))
    # 10: `is` over distinct pointers (the operand it now names is a uint value under the same modulus, with another pointer)
    other = next(i for i in range(is_) if nodes0["kind"][i] == K.TE_UINT_LEAF and nodes0["bound_ptr"][i] == nodes0["bound_ptr"][is_]
                 and nodes0["ptr"][i] != nodes0["ptr"][int(nodes0["rhs"][is_])])
    spoil("a uint `is` over distinct pointers", 10, is_, 0, lhs=(is_, other))
    ec_is = _kind(nodes0, K.TE_EC_OP, 3)
    spoil("an EC `is` over distinct pointers", 10, ec_is, 0, rhs=(ec_is, create))
    # 11: linearity
    second = ands[1]
    inner = int(nodes0["lhs"][second])                                   # the AND below it
    ext = next(int(nodes0[f][a]) for a in ands for f in ("lhs", "rhs") if nodes0[f][a] < 0)
    spoil("a stray unasserted claim", 11, inner, 0, lhs=(second, ext))
    third = ands[2]
    assert nodes0["rhs"][third] < 0                                     # an issued handle gives way: no node goes unread
    spoil("Truthy consumed twice", 11, inner, 1, rhs=(third, inner))
    spoil("the root read", 11, inner, 2, root_=inner)
    # 12: a value node nobody reads
    extra = nodes0[leaf:leaf + 1].copy()
    spoil("a leaf nobody reads", 12, nodes0.size, 0, append=extra)
    # 13: a perm that is not a one-block absorption
    spoil("a perm inside a chain", 13, leaf, 0, perm=(leaf, m.chain + 3))
    spoil("a perm on a chain's head", 13, pin, 1, perm=(pin, m.chain))
    # 14: an MSM span that is not one absorption of n_terms blocks
    head = int(nodes0["perm"][msm])
    spoil("an MSM span that starts inside an absorption", 14, msm, 0, perm=(msm, m.chain + 1))
    spoil("an MSM span that starts one absorption early", 14, t0 + 1, 1, perm=(msm, head - 1))
    spoil("an MSM span shorter than its absorption", 14, msm, 2, perm=(msm, m.chain))
    # 15: an external cycle that does not end an absorption
    a_ext, f_ext = next((a, f) for a in ands for f in ("lhs", "rhs") if nodes0[f][a] < 0)
    spoil("an external binding inside a chain", 15, a_ext, 0 if f_ext == "lhs" else 1, **{f_ext: (a_ext, -1 - (m.chain + 2))})
    return out


def cn_device_defects(c):
    """-> [(what, (data, digests, records), kind, index, operand)]"""
    data, digests, rec0 = c.cn_lists
    m = session_marks(c)
    out = []

    def spoil(what, kind, index, operand, **fields):
        rec = rec0.copy()
        for name, (i, v) in fields.items():
            rec[name][i] = v
        out.append((what, (data, digests, rec), kind, index, operand))
    spoil("a chain that starts inside its absorption", 8, m.long, 0, perm_chunks=(m.long, m.chain + 1))
    spoil("a chain that starts one cycle early", 8, m.long, 1, perm_chunks=(m.long, m.chain - 1))
    spoil("a one-chunk chain on a longer absorption's head", 9, m.short, 0, perm_chunks=(m.short, m.chain))
    spoil("a digest-chunks cycle inside a chain", 9, 0, 1, perm_digest_chunks=(0, m.chain + 1))
    spoil("a node cycle inside a chain", 9, 1, 2, perm_keccak=(1, m.chain + 5))
    spoil("a node cycle in the padding", 9, 2, 2, perm_keccak=(2, c.p2_cycles - 1))
    return out
