"""GPU: the memory chiplet's trace section built on the device from an access list (mh_memory_section_build, mh_miden_memory_section,
csrc/memory_section.hip), run with -m gpu.

Every built section is held bit for bit to tests/memory_section_ref.py (which tests/test_memory_section_cpu.py holds to the generator's
Memory.section()), at the sizes where a kernel can go wrong: around a wave, a block, a sort chunk, a carry tile, and once with more
aggregates than the one wave that scans them takes at a time."""
import ctypes as C
import numpy as np
import pytest
import memory_section_ref as MR
import range_airs as RA
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import chiplets_trace as CT, core_trace as CV  # noqa: E402

pytestmark = pytest.mark.gpu
P = MR.P
DT = pkg.MEM_ACCESS_DTYPE
T = pkg.memory_section_tile()
M32 = (1 << 32) - 1
Z = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def arr(records):
    return np.array([(c, a, k, kd, tuple(v)) for c, a, k, kd, v in records], dtype=DT)


def traffic(n, seed, n_words=None, ctxs=(0, 3, 7)):
    """n accesses a processor could emit, vectorised: one access per cycle (clk = arrival index), every kind, a few words so that most
    words are touched many times and their carries cross wave, block and tile boundaries; 64-bit values, also in the slots reads ignore."""
    rng = np.random.default_rng(seed)
    n_words = n_words or max(1, n // 40)
    a = np.zeros(n, dtype=DT)
    a["ctx"] = np.array(ctxs, dtype=np.uint32)[rng.integers(0, len(ctxs), n)]
    kind = rng.integers(0, 4, n).astype(np.uint32)
    word = (rng.integers(0, n_words, n) * 5 % (1 << 30)).astype(np.uint32) * np.uint32(4)
    a["addr"] = np.where(kind & 2, word, word + rng.integers(0, 4, n).astype(np.uint32))
    a["clk"] = np.arange(n, dtype=np.uint32)
    a["kind"] = kind
    a["value"] = rng.integers(0, 1 << 64, (n, 4), dtype=np.uint64)
    return a


def build_and_compare(ctx, acc, log_n=None):
    """mh_memory_section_build against the oracle: every cell of the trace (zeros below the section), row_of, the info."""
    acc = acc if isinstance(acc, np.ndarray) else arr(acc)
    rows, row_of, n_words, n_contexts = MR.section(acc)
    n = len(acc)
    want_log = MR.min_log_n(n) if log_n is None else log_n
    t, info, got_rows = pkg.memory_section(ctx, acc, log_n, want_rows=True)
    got = t.download()
    assert got.shape == (1 << want_log, 17) and t.log_n == want_log
    assert (got[:n] == rows).all(), (np.argwhere(got[:n] != rows)[:8], n)
    assert not got[n:].any()
    assert (got_rows == row_of).all(), np.argwhere(got_rows != row_of)[:8]
    assert (info.n_rows, info.n_words, info.n_contexts, info.log_n, info.defect, info.defect_index) == (n, n_words, n_contexts, want_log, 0, 0)
    t.free()
    return got[:n], got_rows


# ---- sizes ----
AGG = 65 * T + 1   # 66 tiles: the wave that scans the aggregates goes round twice
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, AGG]
assert AGG <= 1 << 17


@pytest.mark.parametrize("n", SIZES)
def test_sizes_equal_the_rule(ctx, n):
    build_and_compare(ctx, traffic(n, seed=n))


def test_empty_list_and_taller_traces(ctx):
    t, info, rows = pkg.memory_section(ctx, np.zeros(0, dtype=DT), want_rows=True)
    assert t.log_n == 6 and not t.download().any() and rows.size == 0
    assert (info.n_rows, info.n_words, info.n_contexts, info.log_n, info.defect) == (0, 0, 0, 6, 0)
    build_and_compare(ctx, traffic(65, seed=3), log_n=9)
    build_and_compare(ctx, traffic(64, seed=4), log_n=6)


# ---- stability and the digit plan ----
def reads_of_one_word(n, vary=None):
    """n reads of word 8 of context 5 in cycle 9; vary = (field, bit): that one bit alternates in a seeded pattern"""
    a = np.zeros(n, dtype=DT)
    a["ctx"], a["addr"], a["clk"], a["kind"] = 5, 8, 9, 1
    a["addr"] += np.arange(n, dtype=np.uint32) % 4            # element reads of all four elements: one word, one key
    if vary:
        flips = np.random.default_rng(n).integers(0, 2, n).astype(np.uint32)
        a[vary[0]] ^= flips << np.uint32(vary[1])
    return a


@pytest.mark.parametrize("n", [300, 2 * T + 5])
def test_equal_keys_keep_arrival_order(ctx, n):
    """No digit varies, no pass runs: the rows are the list."""
    _, row_of = build_and_compare(ctx, reads_of_one_word(n))
    assert (row_of == np.arange(n)).all()


@pytest.mark.parametrize("field,bit", [("ctx", 31), ("clk", 0), ("addr", 31)])
def test_keys_that_differ_in_one_bit(ctx, field, bit):
    """One pass runs (the top digit, the lowest digit, the digit of word bit 29): within either half the rows keep arrival order."""
    n = 2 * T + 5
    acc = reads_of_one_word(n, (field, bit))
    _, row_of = build_and_compare(ctx, acc)
    hi = ((acc[field] >> np.uint32(bit)) & 1).astype(bool)
    assert 0 < hi.sum() < n
    assert (row_of[~hi] == np.arange((~hi).sum())).all() and (row_of[hi] == (~hi).sum() + np.arange(hi.sum())).all()


def test_all_twelve_digits_vary(ctx):
    """Contexts, words and clocks over their whole 32 (30) bits; a fifth of the list on a pool of sixteen (ctx, word) pairs so that
    words still carry.  Clocks run against arrival order here: the order rule alone decides, as the header says."""
    n = 3 * T + 17
    rng = np.random.default_rng(12)
    a = traffic(n, seed=12)
    a["ctx"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    word = rng.integers(0, 1 << 30, n, dtype=np.uint64).astype(np.uint32) * np.uint32(4)
    pool = rng.integers(0, n, 16)
    pick = rng.integers(0, 5, n) == 0
    src = pool[rng.integers(0, 16, n)]
    a["ctx"] = np.where(pick, a["ctx"][src], a["ctx"])
    word = np.where(pick, word[src], word)
    a["addr"] = np.where(a["kind"] & 2, word, word + (a["addr"] & 3))
    a["clk"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys_hi = (a["ctx"].astype(np.uint64) << np.uint64(30)) | (a["addr"] >> np.uint32(2)).astype(np.uint64)
    vary_hi = np.bitwise_or.reduce(keys_hi) ^ np.bitwise_and.reduce(keys_hi)
    vary_lo = int(np.bitwise_or.reduce(a["clk"]) ^ np.bitwise_and.reduce(a["clk"]))
    assert all((int(vary_hi) >> (8 * d)) & 255 for d in range(8)) and all((vary_lo >> (8 * d)) & 255 for d in range(4))
    build_and_compare(ctx, a)


# ---- carries ----
@pytest.mark.parametrize("word_write", [False, True])
def test_one_word_carried_across_three_tiles(ctx, word_write):
    """3T element writes of one word, the index rotating: every tile aggregate has a full mask only by combining, and the word of a row
    holds values written in up to three other rows.  Then the same with a word write in the middle tile."""
    n = 3 * T
    a = np.zeros(n, dtype=DT)
    a["ctx"], a["clk"] = 2, np.arange(n, dtype=np.uint32)
    a["addr"] = 1024 + np.arange(n, dtype=np.uint32) % 4
    a["value"] = np.random.default_rng(5).integers(0, 1 << 64, (n, 4), dtype=np.uint64)
    if word_write:
        a["addr"][T + T // 2] = 1024
        a["kind"][T + T // 2] = 2
    rows, _ = build_and_compare(ctx, a)
    assert (rows[:3, 7:11] == 0).sum() == 3 + 2 + 1 and rows[3:, 7:11].all()


def test_short_masks_across_tiles(ctx):
    """Words written once at their start and read for more than a tile; words never written (zeros carried); one element written in
    tile 0 and the next one two tiles later."""
    n = 3 * T + 9
    a = np.zeros(n, dtype=DT)
    a["clk"] = np.arange(n, dtype=np.uint32)
    a["kind"] = 1
    a["addr"] = 64 + np.arange(n, dtype=np.uint32) % 3          # one word, element reads
    a["value"] = 77
    a["kind"][1], a["addr"][1], a["value"][1] = 0, 66, (P - 1, 5, 5, 5)
    a["kind"][2 * T + 40], a["addr"][2 * T + 40], a["value"][2 * T + 40] = 0, 67, (1 << 63, 0, 0, 0)
    a["ctx"][T + 3:T + 3 + T // 2] = 9                            # another context: the same word there was never written
    rows, _ = build_and_compare(ctx, a)
    assert (rows[rows[:, 2] == 9][:, 7:11] == 0).all()


# ---- field corners ----
def test_field_corners(ctx):
    vals = [0, 1, P - 1, P, (1 << 64) - 1]
    acc = [(0, 0, 0, 1, Z)]                                                   # a first clock of 0, untouched memory
    clk = 1
    for c in (0, M32):
        for addr in (M32 - 3, 0):
            for v in vals:
                acc.append((c, addr, clk, 2, (v, vals[(clk + 1) % 5], vals[(clk + 2) % 5], vals[(clk + 3) % 5])))
                acc.append((c, addr + 3, clk + 1, 0, (vals[(clk + 4) % 5], 1, 1, 1)))     # addr 2^32 - 1 among them
                acc.append((c, addr + 3, clk + 2, 1, (v, v, v, v)))
                clk += 3
    acc.append((0, M32 - 3, M32, 3, Z))                                        # the last clock there is
    acc.append((7, 12, 0, 0, (P + 2, 0, 0, 0)))
    acc.append((7, 12, M32, 1, Z))                                             # a clock delta of exactly 2^32 - 1
    rows, _ = build_and_compare(ctx, acc)
    delta = rows[:, 11].astype(object) + rows[:, 12].astype(object) * 65536
    assert (delta == M32).sum() >= 1 and int(rows[0, 6]) == 0 and int(delta[0]) == 1
    assert M32 - 3 in [int(d) for d in delta]                                   # the word step 0 -> 2^32 - 4
    assert {int(x) for x in rows[:, 2]} == {0, 7, M32} and (rows[:, 7:11] < np.uint64(P)).all()
    # a context step of exactly 2^32 - 1
    rows, _ = build_and_compare(ctx, [(M32, 4, 3, 0, (P - 1, 0, 0, 0)), (0, 4, 3, 2, (1, 2, 3, 4))])
    assert int(rows[1, 11]) + (int(rows[1, 12]) << 16) == M32 and int(rows[1, 13]) == pow(M32, P - 2, P)


# ---- defects ----
def refused(call):
    with pytest.raises(pkg.MidenHipError) as e:
        call()
    return e.value


def with_defects(n, at, record):
    a = traffic(n, seed=n + 1)
    for i in at:
        for f, v in record(a, i).items():
            a[f][i] = v
    return a


DEFECTS = {
    1: lambda a, i: dict(kind=4 + i % 3),
    2: lambda a, i: dict(kind=2 + i % 2, addr=(int(a["addr"][i]) & ~3) + 1 + i % 3),
    # the access takes ctx, word and cycle of the access three places before it, and writes
    3: lambda a, i: dict(ctx=a["ctx"][i - 3], addr=a["addr"][i - 3], clk=a["clk"][i - 3], kind=int(a["kind"][i - 3]) & 2),
}


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_defects_are_refused_with_the_rules_index(ctx, kind):
    """Offending accesses in three different tiles, given in descending order of index: the lowest index comes back, from both entries;
    nothing is written, the context goes on, and a second call names the same defect."""
    n = 3 * T + 11
    at = [2 * T + 77, T + 5, 300 + kind]
    acc = with_defects(n, at, DEFECTS[kind])
    with pytest.raises(MR.Defect) as ref:
        MR.section(acc)
    assert (ref.value.kind, ref.value.index) == (kind, min(at))
    for _ in range(2):
        e = refused(lambda: pkg.memory_section(ctx, acc))
        assert (e.info.defect, e.info.defect_index, e.info.n_rows) == (kind, min(at), 0) and f"defect {kind}" in str(e) and f"access {min(at)} " in str(e)
    m = pkg.Miden(ctx)
    before = np.random.default_rng(kind).integers(0, P, (1 << 12, 22), dtype=np.uint64)
    chip = pkg.Trace(ctx, before)
    e = refused(lambda: m.memory_section(chip, 100, acc))
    assert (e.info.defect, e.info.defect_index, e.info.log_n) == (kind, min(at), 12)
    assert (chip.download() == before).all()
    good = traffic(n, seed=n + 1)
    info, _ = m.memory_section(chip, 100, good)
    assert info.defect == 0 and (chip.download()[100:100 + n, 3:20] == MR.section(good)[0]).all()
    build_and_compare(ctx, good)
    m.free()


def test_earlier_write_then_read_in_one_cycle_and_reads_that_may_share_one(ctx):
    ok = [(1, 4, 7, 2, (1, 2, 3, 4)), (1, 5, 8, 1, Z), (1, 4, 8, 3, Z), (1, 7, 8, 1, Z)]
    build_and_compare(ctx, ok)
    for bad, index in ((ok + [(1, 6, 8, 0, (9, 0, 0, 0))], 4), ([ok[0], (1, 6, 7, 1, Z)] + ok[1:], 1), ([ok[0], (1, 4, 7, 2, Z)], 1)):
        with pytest.raises(MR.Defect) as ref:
            MR.section(bad)
        assert (ref.value.kind, ref.value.index) == (3, index)
        e = refused(lambda: pkg.memory_section(ctx, arr(bad)))
        assert (e.info.defect, e.info.defect_index) == (3, index)


def test_a_section_that_does_not_fit(ctx):
    acc = traffic(65, seed=1)
    e = refused(lambda: pkg.memory_section(ctx, acc, 6))
    assert (e.info.defect, e.info.defect_index, e.info.log_n) == (4, 64, 6) and "defect 4" in str(e)
    m = pkg.Miden(ctx)
    before = np.random.default_rng(0).integers(0, P, (128, 22), dtype=np.uint64)
    chip = pkg.Trace(ctx, before)
    e = refused(lambda: m.memory_section(chip, 64, acc))
    assert (e.info.defect, e.info.defect_index) == (4, 64)
    e = refused(lambda: m.memory_section(chip, 200, acc))
    assert (e.info.defect, e.info.defect_index) == (4, 0)
    assert (chip.download() == before).all()
    info, rows = m.memory_section(chip, 63, acc, want_rows=True)             # the last row of the trace is the last row of the section
    exp, row_of, _, _ = MR.section(acc)
    got = chip.download()
    assert (got[63:, 3:20] == exp).all() and (rows == row_of).all() and (got[:63] == before[:63]).all()
    assert (got[63:, 0:3] == [1, 1, 0]).all() and (got[63:, 20:22] == before[63:, 20:22]).all()
    info, rows = m.memory_section(chip, 128, acc[:0], want_rows=True)        # nothing, at the very end
    assert info.n_rows == 0 and rows.size == 0 and (chip.download() == got).all()
    m.free()


def test_refused_before_any_launch(ctx):
    acc = traffic(10, seed=2)
    m = pkg.Miden(ctx)
    chip = pkg.Trace(ctx, np.zeros((64, 22), dtype=np.uint64))
    m.memory_section(chip, 0, acc)                                            # sets the argument types
    pkg.memory_section(ctx, acc)[0].free()
    lib, info, h = ctx.lib, pkg.MemSectionInfo(), C.c_void_p()
    ap = acc.ctypes.data_as(C.c_void_p)
    assert lib.mh_miden_memory_section(ctx.h, None, 0, ap, 10, None, C.byref(info)) == 1 and "null" in lib.mh_last_error(ctx.h).decode()
    assert lib.mh_miden_memory_section(ctx.h, chip.h, 0, None, 10, None, None) == 1
    assert lib.mh_miden_memory_section(None, chip.h, 0, ap, 10, None, None) == 1
    assert lib.mh_memory_section_build(ctx.h, ap, 10, -1, None, None, None) == 1
    assert lib.mh_memory_section_build(ctx.h, None, 10, -1, C.byref(h), None, None) == 1 and not h.value
    assert lib.mh_memory_section_build(ctx.h, ap, (1 << 24) + 1, -1, C.byref(h), None, C.byref(info)) == 1 and "2^24" in lib.mh_last_error(ctx.h).decode()
    assert lib.mh_miden_memory_section(ctx.h, chip.h, 0, ap, (1 << 24) + 1, None, None) == 1
    assert lib.mh_memory_section_build(ctx.h, ap, 10, -1, C.byref(h), None, None) == 0 and h.value    # row_of and info may be null
    lib.mh_trace_free(h)
    assert "log_n" in str(refused(lambda: pkg.memory_section(ctx, acc, 5))) and "log_n" in str(refused(lambda: pkg.memory_section(ctx, acc, 33)))
    assert "22" in str(refused(lambda: m.memory_section(pkg.Trace(ctx, np.zeros((64, 21), dtype=np.uint64)), 0, acc)))
    other = pkg.Ctx(0)
    try:
        assert "another context" in str(refused(lambda: m.memory_section(pkg.Trace(other, np.zeros((64, 22), dtype=np.uint64)), 0, acc)))
    finally:
        other.close()
    m.free()


def test_two_calls_leave_the_same_bytes(ctx):
    acc = traffic(2 * T + 300, seed=8, n_words=7)
    a, _, ra = pkg.memory_section(ctx, acc, want_rows=True)
    b, _, rb = pkg.memory_section(ctx, acc, want_rows=True)
    assert a.download().tobytes() == b.download().tobytes() and ra.tobytes() == rb.tobytes()


# ---- the Miden entry ----
def memory_rows(t):
    return np.nonzero((t[:, 0] == 1) & (t[:, 1] == 1) & (t[:, 2] == 0))[0]


def junk_memory_rows(t):
    """columns 0..19 of the memory rows overwritten, a different word in every cell"""
    rows = memory_rows(t)
    assert rows.size and (np.diff(rows) == 1).all()
    j = t.copy()
    j[rows, 0:20] = (np.arange(1, rows.size * 20 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(rows.size, 20)
    return j, int(rows[0]), rows.size


@pytest.mark.parametrize("seed", range(4))
def test_miden_entry_restores_sampled_chiplets(ctx, seed):
    c = CT.sample_chiplets(seed=seed, n_hperm=3 + seed % 3, n_bitwise=5 + seed, n_mem=12 + 40 * seed, merkle_depth=3 + seed % 2)
    t, _ = c.into_traces()
    junk, start, n = junk_memory_rows(t)
    acc = c.memory.access_array()
    assert len(acc) == n == c.memory.num_rows
    m = pkg.Miden(ctx)
    chip = pkg.Trace(ctx, junk)
    info, row_of = m.memory_section(chip, start, acc, want_rows=True)
    got = chip.download()
    assert (got == t).all(), np.argwhere(got != t)[:8]
    assert (info.n_rows, info.n_contexts, info.log_n, info.defect) == (n, len(c.memory.trace), t.shape[0].bit_length() - 1, 0)
    assert (row_of == MR.section(acc)[1]).all()
    m.free()


@pytest.fixture(scope="module")
def program():
    """A testing/core_trace.py program with memory operations at the smallest height: its three traces, never modified"""
    vm = CV.CoreVM(stack_inputs=tuple(range(16)))
    r = CV.prove_inputs(vm, RA.u32_memory_program(1))
    assert r["core"].shape[0] == 64
    r["accesses"] = vm.chiplets.memory.access_array()
    return r


def test_miden_entry_in_the_statement(ctx, program):
    """The memory rows rebuilt, then the range table they look up (the chain): the original traces come back, the statement's
    constraints and buses hold, and the proof is the proof over the generator's traces byte for byte."""
    r = program
    pv, aux_in = r["public_values"], r["aux_inputs"]
    junk, start, n = junk_memory_rows(r["chiplets"])
    assert n == len(r["accesses"])
    m = pkg.Miden(ctx)
    trs = [pkg.Trace(ctx, t) for t in (RA.junked(r["core"]), junk, r["poseidon2"])]
    info, _ = m.memory_section(trs[1], start, r["accesses"])
    assert info.n_rows == n
    got = trs[1].download()
    assert (got == r["chiplets"]).all(), np.argwhere(got != r["chiplets"])[:8]
    rep, _ = m.fill_range_table(trs, pv, aux_in)
    core = trs[0].download()
    assert rep == [] and (core == r["core"]).all(), np.argwhere(core != r["core"])[:8]
    assert m.check(*trs, pv, aux_in) == [] and m.check_balance(*trs, pv, aux_in) == []
    got = m.prove(*trs, pv, aux_in)
    exp = m.prove(*[pkg.Trace(ctx, r[k]) for k in ("core", "chiplets", "poseidon2")], pv, aux_in)
    assert got.bytes == exp.bytes
    ok, dig = pkg.verify_miden(pv, aux_in, got.bytes)
    assert ok and (dig == got.digest).all()
    m.free()


def test_miden_entry_after_an_upload_in_flight(ctx, program):
    junk, start, n = junk_memory_rows(program["chiplets"])
    host, owner = pkg.pinned_array(ctx.lib, junk.shape)
    host[:] = junk
    m = pkg.Miden(ctx)
    chip = pkg.Trace.upload_async(ctx, host)                                 # no Trace.wait: the library orders itself after the copy
    m.memory_section(chip, start, program["accesses"])
    assert (chip.download() == program["chiplets"]).all()
    m.free()
    del owner
