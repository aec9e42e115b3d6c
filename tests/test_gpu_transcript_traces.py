"""The precompile prover's ChunkNode and TranscriptEval traces built on the device (run with -m gpu): mh_chunk_node_trace_build and
mh_transcript_eval_trace_build (csrc/transcript_traces.hip) against the in-tree generators testing/precompile_trace.chunk_node_trace /
transcript_eval_trace cell for cell -- the session, the edge ledger, the small cases, padding -- with the Poseidon2 trace they read
built on the device from the ledger with digest REFERENCES (no permutation on the host); every refusal by kind, index and operand; the
public root; and a whole session whose twelve traces all come from device builders, through to a byte-equal proof.  Every build is made
twice and must leave the same bytes.  The ledgers and defects are tests/transcript_traces_cases.py's, shared with the host-side run of
the same row bodies (tests/test_transcript_traces_cpu.py)."""
import ctypes as C
import numpy as np
import pytest
import transcript_traces_cases as TC

pkg = TC.pkg
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu
UNTOUCHED = 0x1234


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def _vp(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


class DeviceBackend:
    """the two builds on the ABI's own arguments, each TWICE.  The out pointer of a refused call keeps the value it had; an accepted
    call's second run leaves the same bytes.  p2(case): the Poseidon2 trace built on the device from the ledger with references."""

    def __init__(self, ctx):
        self.ctx, lib = ctx, ctx.lib
        lib.mh_chunk_node_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                  C.POINTER(C.c_void_p), C.POINTER(pkg.ChunkNodeInfo)]
        lib.mh_transcript_eval_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                       C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(pkg.TranscriptEvalInfo)]
        self._p2 = {}

    def p2(self, case):
        if case.name not in self._p2:
            absorptions, blocks, refs = TC.p2_lists(case)
            if absorptions.size:
                self._p2[case.name] = pkg.poseidon2_chiplet_trace(self.ctx, absorptions, blocks, refs)[0]
            else:                                                        # no absorption (a ZERO root): one padding cycle
                pad = np.zeros((16, 32), dtype=np.uint64)
                self._p2[case.name] = self.ctx.upload_trace(pad)
        return self._p2[case.name]

    def _twice(self, call, width, felts=None):
        runs = []
        for _ in range(2):
            h = C.c_void_p(UNTOUCHED)
            if felts is not None:
                felts[:] = UNTOUCHED
            rc, info = call(h)
            if rc != 0:
                assert h.value == UNTOUCHED, "a refusal leaves the out pointer alone"
                assert felts is None or (felts == UNTOUCHED).all(), "a refusal leaves the root alone"
                msg = self.ctx.lib.mh_last_error(self.ctx.h).decode()
                assert f"defect {info.defect_kind}, index {info.defect_index}, operand {info.defect_operand}" in msg, msg
                return rc, info, None
            t = pkg.Trace.from_handle(self.ctx, h, int(info.rows).bit_length() - 1, width)
            runs.append((t.download(), None if felts is None else [int(x) for x in felts]))
            t.free()
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1] == runs[1][1], "a second call leaves the same bytes"
        return 0, info, runs[0]

    def cn(self, p2, lists, log_n=-1):
        data, digests, rec = lists

        def call(h):
            info = pkg.ChunkNodeInfo()
            return self.ctx.lib.mh_chunk_node_trace_build(self.ctx.h, p2.h, _vp(data), data.size, _vp(digests), _vp(rec), rec.size, log_n, C.byref(h),
                                                          C.byref(info)), info
        rc, info, run = self._twice(call, 42)
        return rc, info, None if run is None else run[0]

    def te(self, p2, lists, log_n=-1):
        nodes, terms, limbs, root = lists
        felts = np.zeros(4, dtype=np.uint64)

        def call(h):
            info = pkg.TranscriptEvalInfo()
            return self.ctx.lib.mh_transcript_eval_trace_build(self.ctx.h, p2.h, _vp(nodes), nodes.size, _vp(terms), terms.size, _vp(limbs), limbs.shape[0],
                                                               root, log_n, C.byref(h), _vp(felts), C.byref(info)), info
        rc, info, run = self._twice(call, 39, felts)
        return (rc, info, None, None) if run is None else (0, info, run[0], run[1])


@pytest.fixture(scope="module")
def dev(ctx):
    return DeviceBackend(ctx)


def test_session_ledgers_give_the_sessions_traces_and_the_public_root(dev):
    """precompile_session([b"", b"abc", b"abc", bytes(range(200))]): 42 nodes of every kind but PAI, a record read twice, one of 7 chunks;
    the digests of the node rows and every hash of the eval rows read from the device-built Poseidon2 trace"""
    c = TC.session_case()
    TC.same(dev.p2(c).download(), c.traces[1], "the Poseidon2 trace from references")
    info = TC.check(dev, c)
    assert (info.n_nodes, info.n_terms, info.rows, info.n_zero) == (42, 2, 64, 1)


def test_edge_ledger_wave_and_block_edges(dev):
    """300 Keccak claims of lengths 0..299, a repeated input, a 130-step uint_add chain, 70 points, P + pai is P, a 70-term MSM in reversed
    order, a pin: 658 nodes on 727 active rows, 300 records on 2048 rows, 2877 Poseidon2 cycles, none a multiple of 64"""
    c = TC.edge_case()
    info = TC.check(dev, c)
    assert info.n_nodes % 64 and info.active_rows % 64 and info.rows == 1024 and info.p2_cycles == 4096 and c.s.p2.next_seq % 64


@pytest.mark.parametrize("which", range(4), ids=["pinned_root", "zero_root", "zeros_merged", "ec_sub"])
def test_small_cases(dev, which):
    """a lone pinned root, a ZERO root, four ZERO leaves merged under three ANDs (all three with an empty record list: height 2), ec_sub"""
    TC.check(dev, TC.small_cases()[which])


def test_padding(dev):
    TC.check(dev, TC.session_case(), log_cn=6, log_te=8)
    TC.check(dev, TC.small_cases()[0], log_cn=3, log_te=3)
    c = TC.session_case()
    p2 = dev.p2(c)
    TC.refused(dev.cn(p2, c.cn_lists, 3), 7, 16, 0)
    TC.refused(dev.te(p2, c.te_lists, 5), 7, 64, 0)


def test_every_refusal_names_kind_index_and_operand(dev, ctx):
    c = TC.session_case()
    p2 = dev.p2(c)
    te = TC.te_device_defects(c)
    assert {d[2] for d in te} == set(range(8, 16))
    for what, lists, kind, index, operand in te:
        TC.refused(dev.te(p2, lists), kind, index, operand)
    cn = TC.cn_device_defects(c)
    assert {d[2] for d in cn} == {8, 9}
    for what, lists, kind, index, operand in cn:
        TC.refused(dev.cn(p2, lists), kind, index, operand)
    # the planner's, through the build entries: a record past the bytes, a root that is a value node, a p2 of the wrong width
    rec = c.cn_lists[2].copy()
    rec["len"][2] = 201
    TC.refused(dev.cn(p2, (c.cn_lists[0], c.cn_lists[1], rec)), 2, 2, 0)
    TC.refused(dev.te(p2, c.te_lists[:3] + (0,)), 4, 0, 0)
    narrow = ctx.upload_trace(np.zeros((16, 16), dtype=np.uint64))
    TC.refused(dev.cn(narrow, c.cn_lists), 1, 0, 3)
    TC.refused(dev.te(narrow, c.te_lists), 1, 0, 3)
    narrow.free()
    TC.check(dev, c)                                                    # the context goes on


def test_whole_session_from_device_builders_proves_the_same_bytes(dev, ctx):
    """All twelve traces from device builders -- keccak_traces, poseidon2_trace with references, the two new ones, uint_traces, ec_traces,
    the byte-pair table a zero matrix filled by fill_multiplicities -- no generator matrix is uploaded.  check and the exact balance are
    clean, the proof is the bytes of the proof from the uploaded generator matrices, and verify_precompile accepts."""
    c = TC.session_case()
    traces, led, s = c.traces, c.out["ledgers"], c.s
    root = c.public_root
    pc = pkg.Precompile(ctx)
    absorptions, blocks, refs = TC.p2_lists(c)
    p2, _ = pc.poseidon2_trace(absorptions, blocks, refs)
    inv = s.sponge.invocations
    rt, st, _, dig = pc.keccak_traces([r["input"] for r in inv], [r["chunk_head"] for r in inv], want_digests=True)
    data, _digests, rec = c.cn_lists
    cn, _ = pc.chunk_node_trace(p2, data, dig, rec)                    # the digests the device's Keccak returned
    te, _, got_root = pc.transcript_eval_trace(p2, *c.te_lists, log_n=traces[5].shape[0].bit_length() - 1)
    assert got_root == root
    log = lambda i: traces[i].shape[0].bit_length() - 1                # noqa: E731
    tu, ta, _ = pc.uint_traces(*PT.uint_lists(led["store"], led["adds"], led["muls"], own_reads_recorded=True), log(6), log(7))
    ec, _ = pc.ec_traces(*PT.ec_lists(led["ec"], led["ec_add"], led["msm"], own_reads_recorded=True), log(8), log(9), log(10), log(11))
    trs = [cn, p2, rt, ctx.upload_trace(np.zeros_like(traces[3])), st, te, tu, ta] + list(ec)
    w, rep = pc.fill_multiplicities(trs, root, [(3,) + slot for slot in PA.BYTE_PAIR_LUT_MULT_SLOTS])
    assert rep == [] and w == 3 * PA.BPL_TRACE_HEIGHT
    for i, (t, e) in enumerate(zip(trs, traces)):
        TC.same(t.download(), e, PT.SessionTraces.NAMES[i])
    assert pc.check(trs, root) == [] and pc.check_balance(trs, root, exact=True) == []
    proof = pc.prove(trs, root)
    uploaded = pc.prove([ctx.upload_trace(t) for t in traces], root)
    assert bytes(proof.bytes) == bytes(uploaded.bytes)
    ok, digest = pkg.verify_precompile(pc.preprocessed_root(), root, proof.bytes)
    assert ok and (digest == proof.digest).all()
