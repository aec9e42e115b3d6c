"""The precompile prover's Poseidon2 chiplet trace built on the device (run with -m gpu): mh_poseidon2_chiplet_trace_build
(csrc/poseidon2_chiplet.hip) against the in-tree generator testing/precompile_trace.poseidon2_chiplet_trace cell for cell, the digests
against Poseidon2Requires.digest, the permutation outputs against the generator's, the reference form (digest references, poisoned
literals) against the literal form, every refusal, and a whole session whose trace 1 comes from the device through to a byte-equal
proof."""
import ctypes as C
import numpy as np
import pytest
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu
P = pkg.P


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def records(absorptions):
    return np.array([(tuple(int(x) for x in cap), n, im, om) for cap, n, im, om in absorptions], dtype=pkg.P2C_ABSORPTION_DTYPE)


def same(got, exp):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]


def felts(rng, n):
    return [int(x) for x in rng.integers(0, P, n, dtype=np.uint64)]


def literal_ledger(shape, seed):
    """absorptions of shape[i] random blocks each"""
    rng, req = np.random.default_rng(seed), PT.Poseidon2Requires()
    for n in shape:
        req.require_absorption(felts(rng, 4), [(felts(rng, 4), felts(rng, 4)) for _ in range(n)])
    return req


def expected(req, check_digests=True):
    main, outs = PT.poseidon2_chiplet_trace(req)
    tails = [start + len(blocks) - 1 for _, blocks, start, _, _ in req.absorptions]
    dig = outs[tails, 0:4] if tails else np.zeros((0, 4), dtype=np.uint64)
    if check_digests:
        assert [[int(x) for x in d] for d in dig] == [[int(x) for x in req.digest(i)] for i in range(len(req.absorptions))]
    return main, outs, dig


def build(ctx, req, refs=False, unreduced=False, lists=None, **kw):
    absorptions, blocks, r = lists or req.lists(refs=refs)
    rec = records(absorptions)
    if unreduced:  # the same felts as representatives >= p where 64 bits have room
        room = np.uint64((1 << 64) - P)
        blocks = np.where((blocks < room) & (np.repeat(r, 4, axis=1) < 0), blocks + np.uint64(P), blocks)
        rec["cap"] = np.where(rec["cap"] < room, rec["cap"] + np.uint64(P), rec["cap"])
    return pkg.poseidon2_chiplet_trace(ctx, rec, blocks, r if refs else None, want_digests=True, want_outputs=True, **kw)


def check(ctx, req, rows, refs=False, check_digests=True, **kw):
    main, outs, dig = expected(req, check_digests)
    t, info, got_dig, got_outs = build(ctx, req, refs=refs, **kw)
    assert (1 << t.log_n, t.width) == main.shape == (rows, 32) and (info.rows_needed, info.defect_kind) == (rows, 0)
    assert (info.n_absorptions, info.n_cycles) == (len(req.absorptions), req.next_seq)
    got = t.download()
    same(got, main)
    same(got_outs, outs)
    same(got_dig, dig)
    return got, info


# ---- the literal form ----
@pytest.mark.parametrize("shape,rows", [((), 16), ((1,), 16), ((1,) * 70, 2048), ((2, 1, 40, 3, 1, 2), 1024)],
                         ids=["none", "one-block", "70-one-shots", "a-long-chain-among-short"])
def test_literal_ledgers_equal_the_generator(ctx, shape, rows):
    req = literal_ledger(shape, seed=len(shape))
    got, info = check(ctx, req, rows)
    assert info.n_levels == (1 if shape else 0)
    again = build(ctx, req)[0].download()                                  # a second call leaves the same bytes
    assert got.tobytes() == again.tobytes()
    t = pkg.poseidon2_chiplet_trace(ctx, records(req.lists()[0]), req.lists()[1])[0]   # nothing asked back: the same trace
    assert t.download().tobytes() == got.tobytes()


def test_multiplicities_and_felts_are_reduced_mod_p(ctx):
    req = literal_ledger((1, 3, 2), seed=7)
    for a, (im, om) in zip(req.absorptions, [(3, 0), (1, 2), (P + 5, (1 << 64) - 1)]):
        a[3], a[4] = im, om
    got, _ = check(ctx, req, 128, unreduced=True)
    assert (got[5 * 16, PA.P2C_IN_MULT], got[5 * 16, PA.P2C_OUT_MULT]) == (5, ((1 << 64) - 1) % P)
    assert got[:, PA.P2C_IS_ABSORB].reshape(-1, 16)[:, 0].tolist() == [0, 0, 1, 1, 0, 1, 0, 0]


def test_a_level_wider_than_the_group_form_takes(ctx):
    """8200 one-shots: the level leaves the 16-lanes-a-chain kernel for the lane-a-chain one; the absorption behind reads a digest it wrote"""
    req = literal_ledger((1,) * 8200, seed=12)
    req.require_absorption([1, 2, 3, 4], [(req.digest(8199), [5, 6, 7, 8]), ([9, 9, 9, 9], req.digest(0))])
    absorptions, blocks, refs = req.lists()                            # the two references by hand: lists(refs=True) hashes every absorption
    refs[8200, 0], refs[8201, 1] = 8199, 0
    blocks[8200, 0:4] = blocks[8201, 4:8] = PT.Poseidon2Requires.POISON
    _, info = check(ctx, req, 1 << 18, refs=True, check_digests=False, lists=(absorptions, blocks, refs))
    assert info.n_levels == 2


# ---- the reference form: digests as rate words, the literals behind them poisoned ----
def node_triple():
    rng, req = np.random.default_rng(21), PT.Poseidon2Requires()
    chain = req.require_absorption(PT.TAG_CHUNKS_WORD, [(felts(rng, 4), felts(rng, 4)) for _ in range(3)])
    shot = req.require_absorption(felts(rng, 4), [(felts(rng, 4), felts(rng, 4))])
    req.require_absorption(felts(rng, 4), [(req.digest(chain), req.digest(shot))])
    return req, 2, 2


def fold_chain(depth=70):
    rng, req = np.random.default_rng(22), PT.Poseidon2Requires()
    prev = req.require_absorption(felts(rng, 4), [(felts(rng, 4), felts(rng, 4))])
    for k in range(1, depth):
        halves = (req.digest(prev), felts(rng, 4))
        prev = req.require_absorption(felts(rng, 4), [halves if k % 2 else halves[::-1]])
    return req, depth, depth - 1


def wide_level(n=300):
    rng, req = np.random.default_rng(23), PT.Poseidon2Requires()
    leaves = [req.require_absorption(felts(rng, 4), [(felts(rng, 4), felts(rng, 4))]) for _ in range(n)]
    for i in rng.permutation(n):
        req.require_absorption(felts(rng, 4), [(felts(rng, 4), req.digest(leaves[i]))])
    return req, 2, n


@pytest.mark.parametrize("make", [node_triple, fold_chain, wide_level])
def test_reference_form_equals_the_literal_form(ctx, make):
    req, levels, n_refs = make()
    _, blocks, refs = req.lists(refs=True)
    assert int((refs >= 0).sum()) == n_refs and int((blocks == PT.Poseidon2Requires.POISON).sum()) == 4 * n_refs
    rows = max(16, 1 << (16 * req.next_seq - 1).bit_length())
    got, info = check(ctx, req, rows, refs=True)
    assert info.n_levels == levels
    lit, lit_info = check(ctx, req, rows, refs=False)
    assert lit_info.n_levels == 1 and got.tobytes() == lit.tobytes()


# ---- a session's ledger ----
@pytest.fixture(scope="module")
def session():
    rng = np.random.default_rng(9)
    pairs, traces, info = PT.precompile_session([b"", b"abc", bytes(rng.integers(0, 256, 300, dtype=np.uint8))])
    return traces, info


def test_session_ledger_in_both_forms_equals_trace_1(ctx, session):
    traces, info = session
    p2 = info["ledgers"]["p2"]
    assert int((p2.lists(refs=True)[2] >= 0).sum()) == 55
    for refs in (False, True):
        got, pinfo = check(ctx, p2, 1024, refs=refs)
        same(got, traces[1])
        assert (pinfo.n_absorptions, pinfo.n_cycles, pinfo.n_levels) == (49, 59, 10 if refs else 1)


def test_larger_height_pads_and_smaller_is_refused(ctx, session):
    p2 = session[1]["ledgers"]["p2"]
    absorptions, blocks, refs = p2.lists(refs=True)
    t, info = pkg.poseidon2_chiplet_trace(ctx, records(absorptions), blocks, refs, log_n=12)
    assert (t.log_n, info.log_n, info.rows_needed) == (12, 12, 1024)
    same(t.download(), PT.poseidon2_chiplet_trace(p2, min_height=4096)[0])
    with pytest.raises(pkg.MidenHipError, match="defect 6, index 1024") as e:
        pkg.poseidon2_chiplet_trace(ctx, records(absorptions), blocks, refs, log_n=9)
    assert (e.value.info.defect_kind, e.value.info.defect_index, e.value.info.rows_needed) == (6, 1024, 1024)
    t, info = pkg.poseidon2_chiplet_trace(ctx, [], np.zeros((0, 8), dtype=np.uint64), log_n=6)        # no absorption, padded
    same(t.download(), PT.poseidon2_chiplet_trace(PT.Poseidon2Requires(), min_height=64)[0])


# ---- refusals ----
def raw_call(ctx, rec, blocks, refs, n_cycles, log_n=-1, null=()):
    """the ABI itself with a sentinel out-pointer -> (rc, info, out)"""
    lib = ctx.lib
    lib.mh_poseidon2_chiplet_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                                     C.c_void_p, C.c_void_p, C.POINTER(pkg.Poseidon2ChipletInfo)]
    h, info = C.c_void_p(0x1234), pkg.Poseidon2ChipletInfo()
    rc = lib.mh_poseidon2_chiplet_trace_build(ctx.h, None if "abs" in null else rec.ctypes.data_as(C.c_void_p), rec.size,
                                              None if "blocks" in null else blocks.ctypes.data_as(C.c_void_p),
                                              None if refs is None else refs.ctypes.data_as(C.c_void_p), n_cycles, log_n,
                                              None if "out" in null else C.byref(h), None, None, C.byref(info))
    return rc, info, h.value


def test_every_refusal_names_kind_and_index_and_leaves_the_out_pointer(ctx):
    good = [([1, 2, 3, 4], 1, 1, 0), ([0] * 4, 3, 1, 1), ([0] * 4, 2, 1, 1)]           # cycles 0 | 1 2 3 | 4 5
    blocks = np.arange(64, dtype=np.uint64).reshape(8, 8)
    lit = np.full((8, 2), -1, dtype=np.int64)
    bad_ref = lit.copy()
    bad_ref[4, 1], bad_ref[5, 0] = 2, 9
    cases = [
        (good, 6, lit, dict(null=("abs",)), 1, 0),
        (good, 6, lit, dict(null=("blocks",)), 1, 0),
        (good, 6, lit, dict(null=("out",)), 1, 0),
        (good + [([0] * 4, 0, 1, 1)], 6, lit, {}, 2, 3),
        (good, 5, lit, {}, 3, 2),
        (good, 8, lit, {}, 3, 3),
        (good, 6, bad_ref, {}, 4, 9),
        (good, 6, lit, dict(log_n=6), 6, 128),
        (good, 6, None, dict(log_n=0), 6, 128),
    ]
    for absorptions, n_cycles, refs, kw, kind, index in cases:
        rc, info, h = raw_call(ctx, records(absorptions), blocks, refs, n_cycles, **kw)
        assert rc == 1 and (info.defect_kind, info.defect_index) == (kind, index), (kind, index, rc, info)
        assert h == 0x1234 and (info.n_absorptions, info.n_cycles) == (len(absorptions), n_cycles)
        assert f"defect {kind}, index {index}" in ctx.lib.mh_last_error(ctx.h).decode()
        if kind == 6:
            assert (info.rows_needed, info.n_levels) == (128, 1)
    big = records([([0] * 4, (1 << 20) + 1, 1, 1)])
    rc, info, h = raw_call(ctx, big, blocks, None, (1 << 20) + 1)                 # refused before a block is read
    assert rc == 1 and (info.defect_kind, info.defect_index, h) == (5, (1 << 20) + 1, 0x1234)
    # the context goes on
    req = literal_ledger((2, 1), seed=3)
    check(ctx, req, 64)


# ---- a whole session ----
def test_session_with_device_built_poseidon2_trace_proves_the_same_bytes(ctx, session):
    traces, info = session
    root, inv, p2 = info["public_root"], info["session"].sponge.invocations, info["ledgers"]["p2"]
    pc = pkg.Precompile(ctx)
    absorptions, blocks, refs = p2.lists(refs=True)
    pt, pinfo, dig = pc.poseidon2_trace(records(absorptions), blocks, refs, want_digests=True)
    assert pinfo.n_levels == 10 and [[int(x) for x in d] for d in dig] == [[int(x) for x in p2.digest(i)] for i in range(len(absorptions))]
    same(pt.download(), traces[1])
    rt, st, _ = pc.keccak_traces([r["input"] for r in inv], [r["chunk_head"] for r in inv])
    trs = [ctx.upload_trace(t) for t in traces]
    trs[1], trs[2], trs[4] = pt, rt, st
    trs[3] = ctx.upload_trace(np.zeros_like(traces[3]))
    w, rep = pc.fill_multiplicities(trs, root, [(3,) + s for s in PA.BYTE_PAIR_LUT_MULT_SLOTS])
    assert rep == [] and w == 3 * PA.BPL_TRACE_HEIGHT
    same(trs[3].download(), traces[3])
    assert pc.check(trs, root) == [] and pc.check_balance(trs, root, exact=True) == []
    proof = pc.prove(trs, root)
    uploaded = pc.prove([ctx.upload_trace(t) for t in traces], root)
    assert bytes(proof.bytes) == bytes(uploaded.bytes)
    ok, digest = pkg.verify_precompile(pc.preprocessed_root(), root, proof.bytes)
    assert ok and (digest == proof.digest).all()
