"""GPU: the hasher controller's trace section built on the device from an op list (mh_hasher_section_build, mh_miden_hasher_section,
csrc/hasher_section.hip), run with -m gpu.

Every built section is held bit for bit -- all 20 cells, `info` and `results` -- to tests/hasher_section_ref.py (which
tests/test_hasher_section_cpu.py holds to the generator's Hasher.section() and to the reference processor's snapshots), at the sizes
where a kernel can go wrong: around the wave of the chains kernel, around one and two tiles of the scans, and once with more tile
aggregates than the one wave that scans them takes at a time."""
import ctypes as C
import numpy as np
import pytest
import corner_felts as CF
import hasher_section_ref as HR
import range_airs as RA
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import chiplets_trace as CT, core_trace as CV  # noqa: E402

pytestmark = pytest.mark.gpu
P = HR.P
DT = HR.DT
T = pkg.hasher_section_tile()


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def build_and_compare(ctx, ops, felts, log_n=None):
    """mh_hasher_section_build against the rule: every cell of the trace (zeros below the section), the results, the info."""
    ops = np.asarray(ops, dtype=DT)
    rows, results, ref = HR.section(ops, felts)
    n = rows.shape[0]
    want_log = HR.min_log_n(n) if log_n is None else log_n
    t, info, got_res = pkg.hasher_section(ctx, ops, felts, log_n, want_results=True)
    got = t.download()
    assert got.shape == (1 << want_log, 20) and t.log_n == want_log
    assert (got[:n] == rows).all(), (np.argwhere(got[:n] != rows)[:8], n)
    assert not got[n:].any()
    for f in ("addr", "state", "old_root"):
        assert (got_res[f] == results[f]).all(), (f, np.argwhere(got_res[f] != results[f])[:8])
    assert (info.n_rows, info.n_permutations, info.n_requests, info.mrupdate_id, info.log_n, info.defect, info.defect_index) == \
        (n, ref["n_permutations"], ref["n_requests"], ref["mrupdate_id"], want_log, 0, 0)
    t.free()
    return got[:n], ref


def permutes(n, seed, pool=None):
    """n permute ops; pool: the states are drawn from that many distinct ones (None: all distinct)"""
    rng = np.random.default_rng(seed)
    k = n if pool is None else pool
    felts = rng.integers(0, 1 << 64, 12 * k, dtype=np.uint64)
    ops = np.zeros(n, dtype=DT)
    ops["payload"] = 12 * (np.arange(n) if pool is None else rng.integers(0, k, n))
    return ops, felts


def one_kind(kind, n, seed, count=1):
    rng = np.random.default_rng(seed)
    per = {0: 12, 1: 8, 2: 8 * count, 3: 4 + 4 * count, 4: 8 + 4 * count}[kind]
    ops = np.zeros(n, dtype=DT)
    ops["kind"], ops["count"], ops["payload"] = kind, count if kind >= 2 else 0, per * np.arange(n)
    if kind >= 3:
        ops["index"] = rng.integers(0, 1 << min(count, 63), n, dtype=np.uint64)
    if kind == 1:
        ops["index"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return ops, rng.integers(0, 1 << 64, per * n, dtype=np.uint64)


# ---- sizes ----
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 127, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_permute_lists_of_every_size_equal_the_rule(ctx, n):
    """Op count = chain count = permutation count n: rows = 2n padded, so n = 1..4 gives every residue mod 8; 63..65 the wave of the
    chains kernel; 127, 255..257 the block of the rows kernel (256 rows, 2 rows a permutation); T the tile of the plan and id scans."""
    rows, ref = build_and_compare(ctx, *permutes(n, seed=n))
    assert rows.shape[0] % 8 == 0 and rows.shape[0] - 2 * n == (-2 * n) % 8


@pytest.mark.parametrize("n", [63, 64, 65])
def test_chain_counts_around_a_wave_with_updates(ctx, n):
    """n // 3 updates and the rest verifies: n chains from fewer ops, the two legs of an update in different waves at 65."""
    ups = n // 3
    ops_u, felts_u = one_kind(4, ups, seed=n, count=3)
    ops_v, felts_v = one_kind(3, n - 2 * ups, seed=n + 1, count=2)
    ops_v["payload"] += len(felts_u)
    ops = np.concatenate([ops_v[:1], ops_u, ops_v[1:]])
    build_and_compare(ctx, ops, np.concatenate([felts_u, felts_v]))


def test_more_tile_aggregates_than_one_wave_scans_at_a_time(ctx):
    """65 T + 1 permutes from a pool of 1000 states: 66 tiles in the plan scan and in the id scan, first appearances far from repeats."""
    n = 65 * T + 1
    rows, ref = build_and_compare(ctx, *permutes(n, seed=5, pool=1000))
    assert ref["n_requests"] == 1000


def test_empty_list_and_taller_traces(ctx):
    t, info, res = pkg.hasher_section(ctx, np.zeros(0, dtype=DT), np.zeros(0, dtype=np.uint64), want_results=True)
    assert t.log_n == 6 and not t.download().any() and res.size == 0
    assert (info.n_rows, info.n_permutations, info.n_requests, info.mrupdate_id, info.log_n, info.defect) == (0, 0, 0, 0, 6, 0)
    t.free()
    build_and_compare(ctx, *permutes(33, seed=3), log_n=9)
    build_and_compare(ctx, *permutes(32, seed=4), log_n=6)           # the section fills the trace
    build_and_compare(ctx, *permutes(33, seed=4))                    # log_n = -1 goes to 7


# ---- kinds ----
@pytest.mark.parametrize("kind,count", [(0, 1), (1, 1), (2, 1), (2, 2), (2, 3), (2, 9), (3, 1), (3, 2), (3, 64), (4, 1), (4, 2), (4, 64)])
def test_each_kind_alone(ctx, kind, count):
    n = 70 if count < 64 else 9
    ops, felts = one_kind(kind, n, seed=10 * kind + count, count=count)
    if kind >= 3:                                                    # index 0, all ones (the largest there is at depth 64: p - 1)
        ops["index"][0] = 0
        ops["index"][1] = (1 << count) - 1 if count < 64 else P - 1
        if count == 64:
            ops["index"][2:] = np.random.default_rng(count).integers(1 << 63, P, n - 2, dtype=np.uint64)
    rows, ref = build_and_compare(ctx, ops, felts)
    assert ref["mrupdate_id"] == (n if kind == 4 else 0)


@pytest.mark.parametrize("seed", range(6))
def test_all_kinds_mixed(ctx, seed):
    """Seeded mixed lists of 100..700 ops with ops listed again; depths to 12, blocks to 9 batches: an update directly after a verify
    is in every one of them, so mrupdate_id steps in the middle of the list."""
    ops, felts = HR.random_list(100 + seed, n_ops=100 + 120 * seed, max_depth=12, max_batches=9)
    k = [int(x) for x in ops["kind"]]
    assert any(a == 3 and b == 4 for a, b in zip(k, k[1:]))
    rows, ref = build_and_compare(ctx, ops, felts)
    assert ref["n_requests"] < ref["n_permutations"] <= 4500


# ---- perm_id ----
def test_perm_ids_of_repeated_states(ctx):
    w = lambda a: [a, a + 1, a + 2, a + 3]  # noqa: E731
    small = [5, 2 ** 32 - 2, 0, 1] * 3
    # the same state twice; once canonical and once as x + p
    rows, ref = build_and_compare(ctx, np.array([(0, 0, 0, 0), (0, 0, 0, 12), (0, 0, 0, 0)], dtype=DT), small + [x + P for x in small])
    assert [int(x) for x in rows[:6, 19]] == [0] * 6 and ref["n_requests"] == 1 and ref["multiplicities"] == [3]
    # an update with old == new: every state of the new leg repeats the old leg's; a verify of the same path before it
    felts = w(1) + w(1) + w(20) + w(30) + w(40)
    rows, ref = build_and_compare(ctx, np.array([(3, 3, 5, 4), (4, 3, 5, 0)], dtype=DT), felts)
    assert [int(x) for x in rows[0:18:2, 19]] == [0, 1, 2] * 3 and ref["multiplicities"] == [3, 3, 3]
    # two verifies that share the upper half of a path: leaves 4 and 5 of one tree are siblings, so the levels above agree
    leaf4, leaf5, up = w(100), w(200), w(300) + w(400) + w(500)
    felts = leaf4 + leaf5 + up + leaf5 + leaf4 + up
    rows, ref = build_and_compare(ctx, np.array([(3, 4, 4, 0), (3, 4, 5, 20)], dtype=DT), felts)
    assert [int(x) for x in rows[0:16:2, 19]] == [0, 1, 2, 3, 0, 1, 2, 3] and ref["n_requests"] == 4
    assert (rows[0, 3:15] == rows[8, 3:15]).all() and int(rows[0, 18]) == 0 and int(rows[8, 18]) == 1


@pytest.mark.parametrize("pool", [1, 2, None])
def test_perm_ids_all_equal_few_and_all_distinct(ctx, pool):
    """3 T + 7 permutes: all states equal (one slot of the table takes every permutation), two states, all distinct; the ids, n_requests
    and the multiplicities (counts per id) against the generator's ledger."""
    n = 3 * T + 7
    ops, felts = permutes(n, seed=9, pool=pool)
    rows, ref = build_and_compare(ctx, ops, felts)
    ids = rows[0:2 * n:2, 19].astype(np.int64)
    assert ref["n_requests"] == (pool or n) == ids.max() + 1
    assert (np.bincount(ids) == np.array(ref["multiplicities"])).all()
    h, _ = HR.replay(ops[:300], felts)                               # the generator's own ledger on a prefix: ids are first appearances
    assert [m for _, m in h.perm_requests] == np.bincount(ids[:300]).tolist()


def test_a_repeat_whose_first_appearance_lies_in_another_tile(ctx):
    n = 2 * T + 50
    ops, felts = permutes(n, seed=21)
    for late, early in ((T + 3, 5), (2 * T + 9, T - 1), (2 * T + 49, 0), (300, 299)):
        ops["payload"][late] = ops["payload"][early]
    rows, ref = build_and_compare(ctx, ops, felts)
    ids = rows[0:2 * n:2, 19]
    assert ref["n_requests"] == n - 4 and ids[T + 3] == ids[5] == 5 and ids[2 * T + 49] == 0 and ids[2 * T + 9] == ids[T - 1]


# ---- field corners ----
def test_field_corners(ctx):
    """States, values and siblings from corner_felts: 0, 1, p - 1, p - 2, 2^32 - 1, 2^32, ... and 2^64 - 1 as a non-canonical input."""
    corners = [int(c) for c in CF.CORNERS] + [(1 << 64) - 1, P]
    ops, felts = [], []
    for v in CF.corner_vectors(12, 24, seed=1) + [np.array([c] * 12, dtype=np.uint64) for c in corners[-2:]]:
        ops.append((0, 0, 0, len(felts)))
        felts += [int(x) for x in v]
    for j, c in enumerate(corners):
        nxt = corners[(j + 1) % len(corners)]
        ops.append((1, 0, c, len(felts)))                            # the domain is a corner too
        felts += [c] * 4 + [nxt] * 4
        ops.append((2, 3, 0, len(felts)))
        felts += [c, nxt] * 12
        ops.append((3, 3, 5, len(felts)))
        felts += [c] * 4 + [nxt] * 4 + [c] * 4 + [nxt, c, nxt, c]
        ops.append((4, 2, 2, len(felts)))
        felts += [nxt] * 4 + [c] * 4 + [c] * 8
    rows, ref = build_and_compare(ctx, np.array(ops, dtype=DT), np.array(felts, dtype=np.uint64))
    assert (rows < np.uint64(P)).all() and ref["n_requests"] < ref["n_permutations"]     # p and 0, 2^64 - 1 and 2^32 - 2 are one state


# ---- defects ----
def refused(call):
    with pytest.raises(pkg.MidenHipError) as e:
        call()
    return e.value


def mixed(n, seed):
    return HR.random_list(seed, n_ops=n, max_depth=3, max_batches=2, repeat=0.0)


DEFECTS = {
    1: lambda o, nf: dict(kind=5 + int(o["payload"]) % 3),
    2: lambda o, nf: dict(kind=2 + int(o["payload"]) % 3, count=0 if int(o["payload"]) % 3 == 0 or int(o["payload"]) % 2 else 65),
    3: lambda o, nf: dict(kind=3, count=2, index=4),
    4: lambda o, nf: dict(kind=0, payload=nf - 11),
}


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_defects_are_refused_with_the_rules_index(ctx, kind):
    """Offending ops in three different tiles, given in descending order of index: the lowest index comes back, from both entries;
    nothing is written, the context goes on, and a second call names the same defect."""
    n = 2 * T + 11
    at = [2 * T + 7, T + 5, 300 + kind]
    ops, felts = mixed(n, seed=40 + kind)
    for i in at:
        for f, v in DEFECTS[kind](ops[i], len(felts)).items():
            ops[f][i] = v
    with pytest.raises(HR.Defect) as ref:
        HR.section(ops, felts)
    assert (ref.value.kind, ref.value.index) == (kind, min(at))
    for _ in range(2):
        e = refused(lambda: pkg.hasher_section(ctx, ops, felts))
        assert (e.info.defect, e.info.defect_index, e.info.n_rows) == (kind, min(at), 0) and f"defect {kind}" in str(e) and f"op {min(at)}" in str(e)
    m = pkg.Miden(ctx)
    before = np.random.default_rng(kind).integers(0, P, (1 << 14, 22), dtype=np.uint64)
    chip = pkg.Trace(ctx, before)
    e = refused(lambda: m.hasher_section(chip, ops, felts))
    assert (e.info.defect, e.info.defect_index, e.info.log_n) == (kind, min(at), 14)
    assert (chip.download() == before).all()
    good, gfelts = mixed(n, seed=40 + kind)
    info, _ = m.hasher_section(chip, good, gfelts)
    rows = HR.section(good, gfelts)[0]
    got = chip.download()
    assert info.defect == 0 and (got[:len(rows), 1:21] == rows).all() and not got[:len(rows), 0].any()
    build_and_compare(ctx, good, gfelts)
    m.free()


def test_the_lowest_defective_op_whatever_its_kind(ctx):
    ops, felts = mixed(T + 40, seed=50)
    ops["kind"][T + 20] = 9                                          # defect 1 late, defect 4 early: the earlier op is named
    ops["payload"][17] = len(felts)
    e = refused(lambda: pkg.hasher_section(ctx, ops, felts))
    with pytest.raises(HR.Defect) as ref:
        HR.section(ops, felts)
    assert (e.info.defect, e.info.defect_index) == (ref.value.kind, ref.value.index) == (4, 17)


def test_a_section_that_does_not_fit(ctx):
    ops, felts = mixed(40, seed=60)
    rows, _, ref = HR.section(ops, felts)
    n = rows.shape[0]
    assert 64 < n <= 256
    with pytest.raises(HR.Defect) as want:
        HR.section(ops, felts, cap_rows=64)
    e = refused(lambda: pkg.hasher_section(ctx, ops, felts, 6))
    assert (e.info.defect, e.info.defect_index, e.info.log_n, e.info.n_rows) == (5, want.value.index, 6, 0) and "defect 5" in str(e)
    assert 0 < want.value.index < 40
    m = pkg.Miden(ctx)
    before = np.random.default_rng(0).integers(0, P, (64, 22), dtype=np.uint64)
    chip = pkg.Trace(ctx, before)
    e = refused(lambda: m.hasher_section(chip, ops, felts))
    assert (e.info.defect, e.info.defect_index) == (5, want.value.index)
    assert (chip.download() == before).all()
    exact, efelts = permutes(32, seed=61)                           # 64 rows: the last row of the trace is the last row of the section
    info, res = m.hasher_section(chip, exact, efelts, want_results=True)
    erows, eres, _ = HR.section(exact, efelts)
    got = chip.download()
    assert info.n_rows == 64 and (got[:, 1:21] == erows).all() and not got[:, 0].any() and (got[:, 21] == before[:, 21]).all()
    assert (res["state"] == eres["state"]).all() and (res["addr"] == eres["addr"]).all()
    info, _ = m.hasher_section(chip, exact[:0], efelts)             # nothing
    assert info.n_rows == 0 and (chip.download() == got).all()
    m.free()


def test_refused_before_anything_is_written(ctx):
    ops, felts = permutes(10, seed=2)
    m = pkg.Miden(ctx)
    before = np.random.default_rng(1).integers(0, P, (64, 22), dtype=np.uint64)
    chip = pkg.Trace(ctx, before)
    m.hasher_section(chip, ops, felts)                               # sets the argument types
    pkg.hasher_section(ctx, ops, felts)[0].free()
    after = chip.download()
    lib, info, h = ctx.lib, pkg.HasherSectionInfo(), C.c_void_p()
    op, fp = ops.ctypes.data_as(C.c_void_p), felts.ctypes.data_as(C.c_void_p)
    assert lib.mh_miden_hasher_section(ctx.h, None, op, 10, fp, 120, None, C.byref(info)) == 1 and "null" in lib.mh_last_error(ctx.h).decode()
    assert lib.mh_miden_hasher_section(ctx.h, chip.h, None, 10, fp, 120, None, None) == 1
    assert lib.mh_miden_hasher_section(ctx.h, chip.h, op, 10, None, 120, None, None) == 1
    assert lib.mh_miden_hasher_section(None, chip.h, op, 10, fp, 120, None, None) == 1
    assert lib.mh_hasher_section_build(ctx.h, op, 10, fp, 120, -1, None, None, None) == 1
    assert lib.mh_hasher_section_build(ctx.h, None, 10, fp, 120, -1, C.byref(h), None, None) == 1 and not h.value
    assert lib.mh_hasher_section_build(ctx.h, op, (1 << 24) + 1, fp, 120, -1, C.byref(h), None, C.byref(info)) == 1
    assert "2^24" in lib.mh_last_error(ctx.h).decode() and not h.value
    assert lib.mh_miden_hasher_section(ctx.h, chip.h, op, (1 << 24) + 1, fp, 120, None, None) == 1
    assert lib.mh_hasher_section_build(ctx.h, op, 10, fp, 120, -1, C.byref(h), None, None) == 0 and h.value    # results and info may be null
    lib.mh_trace_free(h)
    # more than 2^24 permutations in few ops: a block of 2^24 batches after one permute, a block of 2^32 - 1
    for count in (1 << 24, (1 << 32) - 1):
        big = np.array([(0, 0, 0, 0), (2, count, 0, 0)], dtype=DT)
        e = refused(lambda: pkg.hasher_section(ctx, big, felts))
        assert "2^24" in str(e) and (e.info.defect, e.info.n_rows) == (0, 0)
        with pytest.raises(HR.TooMany):
            HR.section(big, felts)
        assert "2^24" in str(refused(lambda: m.hasher_section(chip, big, felts)))
    assert "log_n" in str(refused(lambda: pkg.hasher_section(ctx, ops, felts, 5))) and "log_n" in str(refused(lambda: pkg.hasher_section(ctx, ops, felts, 33)))
    assert "22" in str(refused(lambda: m.hasher_section(pkg.Trace(ctx, np.zeros((64, 21), dtype=np.uint64)), ops, felts)))
    other = pkg.Ctx(0)
    try:
        assert "another context" in str(refused(lambda: m.hasher_section(pkg.Trace(other, np.zeros((64, 22), dtype=np.uint64)), ops, felts)))
    finally:
        other.close()
    assert (chip.download() == after).all()
    build_and_compare(ctx, ops, felts)                               # the context goes on
    m.free()


def test_two_calls_leave_the_same_bytes(ctx):
    ops, felts = HR.random_list(70, n_ops=2 * T + 300, max_depth=6, max_batches=3, repeat=0.4)
    a, ia, ra = pkg.hasher_section(ctx, ops, felts, want_results=True)
    b, ib, rb = pkg.hasher_section(ctx, ops, felts, want_results=True)
    assert a.download().tobytes() == b.download().tobytes() and ra.tobytes() == rb.tobytes() and bytes(ia) == bytes(ib)


# ---- the Miden entry ----
def junk_controller_rows(t):
    """columns 1..20 of the hasher's rows (column 0 = 0) overwritten, a different word in every cell"""
    rows = np.nonzero(t[:, 0] == 0)[0]
    assert rows.size and rows[0] == 0 and (np.diff(rows) == 1).all()
    j = t.copy()
    j[rows, 1:21] = (np.arange(1, rows.size * 20 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(rows.size, 20)
    return j, rows.size


@pytest.mark.parametrize("seed", range(4))
def test_miden_entry_restores_sampled_chiplets(ctx, seed):
    c = CT.sample_chiplets(seed=seed, n_hperm=3 + seed % 3, n_bitwise=5 + seed, n_mem=12 + 40 * seed, merkle_depth=3 + seed % 2)
    t, p2 = c.into_traces()
    junk, n = junk_controller_rows(t)
    ops, felts = c.hasher.op_list()
    m = pkg.Miden(ctx)
    chip = pkg.Trace(ctx, junk)
    info, res = m.hasher_section(chip, ops, felts, want_results=True)
    got = chip.download()
    assert (got == t).all(), np.argwhere(got != t)[:8]
    assert (info.n_rows, info.n_permutations, info.n_requests, info.mrupdate_id, info.log_n, info.defect) == \
        (n, len(c.hasher.rows) // 2, len(c.hasher.perm_requests), c.hasher.mrupdate_id, t.shape[0].bit_length() - 1, 0)
    assert (res["addr"] == HR.section(ops, felts)[1]["addr"]).all()
    third, p2info = m.poseidon2_trace(chip)
    assert p2info.n_requests == info.n_requests and (third.download() == p2).all()
    m.free()


@pytest.fixture(scope="module")
def program():
    """A testing/core_trace.py program at the smallest height: its three traces, never modified, and the hasher's op list"""
    vm = CV.CoreVM(stack_inputs=tuple(range(16)))
    r = CV.prove_inputs(vm, RA.u32_memory_program(1))
    assert r["core"].shape[0] == 64
    r["hash_ops"] = vm.chiplets.hasher.op_list()
    return r


def test_miden_entry_in_the_statement(ctx, program):
    """The controller rows rebuilt on the device, then the third trace from them: the original traces come back, the statement's
    constraints and buses hold, and the proof is the proof over the generator's traces byte for byte."""
    r = program
    pv, aux_in = r["public_values"], r["aux_inputs"]
    junk, n = junk_controller_rows(r["chiplets"])
    m = pkg.Miden(ctx)
    chip = pkg.Trace(ctx, junk)
    info, _ = m.hasher_section(chip, *r["hash_ops"])
    assert info.n_rows == n
    got = chip.download()
    assert (got == r["chiplets"]).all(), np.argwhere(got != r["chiplets"])[:8]
    third, p2info = m.poseidon2_trace(chip, log_n=r["poseidon2"].shape[0].bit_length() - 1)
    assert p2info.n_requests == info.n_requests and (third.download() == r["poseidon2"]).all()
    trs = [pkg.Trace(ctx, r["core"]), chip, third]
    assert m.check(*trs, pv, aux_in) == [] and m.check_balance(*trs, pv, aux_in) == []
    got = m.prove(*trs, pv, aux_in)
    exp = m.prove(*[pkg.Trace(ctx, r[k]) for k in ("core", "chiplets", "poseidon2")], pv, aux_in)
    assert got.bytes == exp.bytes
    ok, dig = pkg.verify_miden(pv, aux_in, got.bytes)
    assert ok and (dig == got.digest).all()
    m.free()


def test_miden_entry_after_an_upload_in_flight(ctx, program):
    junk, n = junk_controller_rows(program["chiplets"])
    host, owner = pkg.pinned_array(ctx.lib, junk.shape)
    host[:] = junk
    m = pkg.Miden(ctx)
    chip = pkg.Trace.upload_async(ctx, host)                         # no Trace.wait: the library orders itself after the copy
    m.hasher_section(chip, *program["hash_ops"])
    assert (chip.download() == program["chiplets"]).all()
    m.free()
    del owner
