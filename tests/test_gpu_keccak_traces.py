"""The precompile prover's Keccak round and sponge traces built on the device (run with -m gpu): mh_keccak_round_trace_build and
mh_keccak_traces_build (csrc/keccak_traces.hip) against the in-tree generators testing/precompile_trace.keccak_round_trace,
SpongeRequires and keccak_sponge_trace cell for cell, the digests against the generator's and two known answers, every refusal, and a
whole session whose traces 2 and 4 come from the device through to a byte-equal proof."""
import ctypes as C
import numpy as np
import pytest
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 7, 8, 31, 32, 33, 129, 130, 135, 136, 137, 271, 272, 300]
KNOWN = {b"": "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
         b"abc": "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"}


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def states():
    rng = np.random.default_rng(11)
    return np.array([[0] * 25] + [[int(x) for x in rng.integers(0, 1 << 63, 25)] for _ in range(6)], dtype=np.uint64)


def sponge_of(messages):
    sp = PT.SpongeRequires()
    outs = [sp.require(m) for m in messages]
    return sp, [o["chunk_head"] for o in outs], [o["keccak_digest"] for o in outs]


def messages_of(lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lengths]


@pytest.fixture(scope="module")
def hashed():
    """the messages of every boundary length once: (messages, SpongeRequires, chunk heads, digests, sponge trace, round trace)"""
    msgs = messages_of(LENGTHS) + [b"abc"]
    sp, heads, digests = sponge_of(msgs)
    return msgs, sp, heads, digests, PT.keccak_sponge_trace(sp), PT.keccak_round_trace(sp.perm_inputs)[0]


def same(got, exp):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]


# ---- the round builder on its own ----
@pytest.mark.parametrize("n", [7, 1, 2, 0])
def test_round_trace_equals_the_generator(ctx, states, n):
    exp = PT.keccak_round_trace(states[:n])[0]
    t, outs = pkg.keccak_round_trace(ctx, states[:n], want_outputs=True)
    assert (1 << t.log_n, t.width) == exp.shape and (n != 7 or t.log_n == 14)
    same(t.download(), exp)
    assert outs.shape == (n, 25)
    for k in range(n):
        assert [int(x) for x in outs[k]] == PT.keccak_f_reference([int(x) for x in states[k]])
    same(pkg.keccak_round_trace(ctx, states[:n]).download(), exp)     # without outputs, and a second call: the same bytes


def test_round_trace_pads_above_the_least_height_and_refuses_below(ctx, states):
    exp = PT.keccak_round_trace(states)[0]
    padded = np.zeros((1 << 15, PA.KR_MAIN_COLS), dtype=np.uint64)      # the generator's rule: zero rows, ip running on in both lanes
    padded[:1 << 14] = exp
    for lane in range(PA.KR_NUM_LANES):
        cb = lane * PA.KR_LANE_WIDTH
        padded[:, cb + PA.KR_COL_IP] = np.arange(1 << 15, dtype=np.uint64) + exp[0, cb + PA.KR_COL_IP]
    t = pkg.keccak_round_trace(ctx, states, log_n=15)
    assert t.log_n == 15
    same(t.download(), padded)
    with pytest.raises(pkg.MidenHipError, match="16384 rows needed"):
        pkg.keccak_round_trace(ctx, states, log_n=13)
    with pytest.raises(pkg.MidenHipError, match="more than 2\\^24 rows"):
        pkg.keccak_round_trace(ctx, np.zeros((10485, 25), dtype=np.uint64))


# ---- both builders from messages ----
def test_both_traces_and_digests_equal_the_generators(ctx, hashed):
    msgs, sp, heads, digests, exp_sponge, exp_round = hashed
    rt, st, info, dig = pkg.keccak_traces(ctx, msgs, heads, want_digests=True)
    assert info.n_perms == len(sp.perm_inputs) == 23 and info.sponge_rows == sp.next_sponge_seq and info.defect_kind == 0
    assert (info.round_rows_needed, info.sponge_rows_needed) == (exp_round.shape[0], exp_sponge.shape[0])
    same(st.download(), exp_sponge)
    same(rt.download(), exp_round)
    assert [bytes(d) for d in dig] == digests
    for m, d in zip(msgs, dig):
        if m in KNOWN:
            assert bytes(d).hex() == KNOWN[m]
    rt2, st2, _ = pkg.keccak_traces(ctx, msgs, heads)                  # no digests asked; a second call leaves the same bytes
    same(rt2.download(), exp_round)
    same(st2.download(), exp_sponge)


def test_subset_sizes_empty_message_alone_and_no_message(ctx):
    msgs = messages_of([0, 1, 135, 136, 137, 271, 272, 300], seed=4)
    sp, heads, digests = sponge_of(msgs)
    rt, st, info, dig = pkg.keccak_traces(ctx, msgs, heads, want_digests=True)
    assert (info.n_perms, info.sponge_rows_needed, info.round_rows_needed) == (15, 512, 1 << 15)
    same(st.download(), PT.keccak_sponge_trace(sp))
    same(rt.download(), PT.keccak_round_trace(sp.perm_inputs)[0])
    assert [bytes(d) for d in dig] == digests and bytes(dig[0]).hex() == KNOWN[b""]
    # no message: one inactive round cycle, 32 sponge padding rows
    sp0 = PT.SpongeRequires()
    rt, st, info, dig = pkg.keccak_traces(ctx, [], [], want_digests=True)
    assert (info.n_perms, info.sponge_rows, info.sponge_rows_needed, info.round_rows_needed) == (0, 0, 32, 4096) and dig.shape == (0, 32)
    same(st.download(), PT.keccak_sponge_trace(sp0))
    same(rt.download(), PT.keccak_round_trace([])[0])


def test_larger_heights_pad_by_the_generators_rule(ctx):
    msgs = [b"abc", bytes(range(137))]
    sp, heads, _ = sponge_of(msgs)
    exp_round = PT.keccak_round_trace(sp.perm_inputs)[0]
    rt, st, info = pkg.keccak_traces(ctx, msgs, heads, log_round=14, log_sponge=8)
    assert (rt.log_n, st.log_n, info.round_rows_needed, info.sponge_rows_needed) == (14, 8, 1 << 13, 128)
    same(st.download(), PT.keccak_sponge_trace(sp, min_height=256))
    got = rt.download()
    same(got[:1 << 13], exp_round)
    rest = got[1 << 13:].copy()
    for lane in range(PA.KR_NUM_LANES):
        cb = lane * PA.KR_LANE_WIDTH
        assert (rest[:, cb + PA.KR_COL_IP] == np.arange(1 << 13, 1 << 14, dtype=np.uint64) + exp_round[0, cb + PA.KR_COL_IP]).all()
        rest[:, cb + PA.KR_COL_IP] = 0
    assert not rest.any()


# ---- refusals ----
def raw_call(ctx, data, rec, log_round=-1, log_sponge=-1, null=()):
    """the ABI itself with sentinel out-pointers -> (rc, info, round_out, sponge_out)"""
    lib = ctx.lib
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rec = np.ascontiguousarray(rec, dtype=pkg.KECCAK_MSG_DTYPE)
    lib.mh_keccak_traces_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(pkg.KeccakTracesInfo)]
    hr, hs, info = C.c_void_p(0x1234), C.c_void_p(0x5678), pkg.KeccakTracesInfo()
    rc = lib.mh_keccak_traces_build(ctx.h, None if "bytes" in null else data.ctypes.data_as(C.c_void_p), data.size,
                                    None if "msgs" in null else rec.ctypes.data_as(C.c_void_p), rec.size, log_round, log_sponge,
                                    None if "round_out" in null else C.byref(hr), None if "sponge_out" in null else C.byref(hs), None, C.byref(info))
    return rc, info, hr.value, hs.value


def test_every_refusal_names_kind_and_index_and_leaves_the_out_pointers(ctx):
    data = np.arange(300, dtype=np.uint8)
    good = [(0, 3, 0), (3, 137, 1), (140, 100, 6)]                                  # 1 + 2 + 1 blocks
    cases = [
        (good[:2] + [(140, 161, 6)], {}, 1, 2),                                    # offset + len past n_bytes
        ([(301, 0, 0)] + good, {}, 1, 0),                                          # ... by the offset alone, the lowest message
        (good[:1] + [(3, 137, (1 << 30) - 2)], {}, 2, 1),                          # 4 chunk_head + 20 lanes reaches 2^32
        (good[:2] + [(0, 0, 1 << 62)], {}, 2, 2),                                  # ... and a head whose quadruple wraps
        ([(0, 0, 0)] * 10485, {}, 3, 10484),                                       # 10485 permutations: the round trace leaves 2^24 rows
        (good, dict(null=("msgs",)), 4, 0),
        (good, dict(null=("bytes",)), 4, 0),
        (good, dict(null=("round_out",)), 4, 0),
        (good, dict(null=("sponge_out",)), 4, 0),
        (good, dict(log_round=12), 5, 1 << 13),                                    # 4 permutations: 2 a lane, 6400 rows
        (good, dict(log_sponge=6), 6, 128),
    ]
    for rec, kw, kind, index in cases:
        rc, info, hr, hs = raw_call(ctx, data, rec, **kw)
        assert rc == 1 and (info.defect_kind, info.defect_index) == (kind, index), (kind, index, rc, info)
        assert hr == 0x1234 and hs == 0x5678
        assert f"defect {kind}" in ctx.lib.mh_last_error(ctx.h).decode()
        if kind >= 5:
            assert (info.n_perms, info.round_rows_needed, info.sponge_rows_needed) == (4, 1 << 13, 128)
    with pytest.raises(pkg.MidenHipError) as e:
        pkg.keccak_traces(ctx, [b"abc"], [1 << 30])
    assert (e.value.info.defect_kind, e.value.info.defect_index) == (2, 0)
    # the largest head that fits is taken, and the context goes on
    sp, heads, _ = sponge_of([b"abc"])
    rt, st, info = pkg.keccak_traces(ctx, [b"abc"], [(1 << 30) - 1 - 1])
    exp = PT.keccak_sponge_trace(sp)
    exp[:, PA.SPC_CHUNK_PTR] += np.uint64(4 * ((1 << 30) - 2 - heads[0]))
    same(st.download(), exp)


# ---- a whole session ----
def test_session_with_device_built_keccak_traces_proves_the_same_bytes(ctx):
    rng = np.random.default_rng(9)
    pairs, traces, info = PT.precompile_session([b"", b"abc", bytes(rng.integers(0, 256, 300, dtype=np.uint8))])
    root, inv = info["public_root"], info["session"].sponge.invocations
    pc = pkg.Precompile(ctx)
    rt, st, kinfo, dig = pc.keccak_traces([r["input"] for r in inv], [r["chunk_head"] for r in inv], want_digests=True)
    assert [bytes(d) for d in dig] == list(info["keccak_digests"]) and kinfo.n_perms == 5
    same(rt.download(), traces[2])
    same(st.download(), traces[4])
    trs = [ctx.upload_trace(t) for t in traces]
    trs[2], trs[4] = rt, st
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
