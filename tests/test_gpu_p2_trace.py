"""GPU: the Poseidon2 permutation trace built on the device (mh_poseidon2_trace_build, mh_miden_poseidon2_trace, csrc/p2_trace.hip),
run with -m gpu.

Every built trace is held cell for cell to miden_air.poseidon2_permutation_trace (the in-tree restatement of
fill_poseidon2_permutation_trace), the request lists read from chiplets traces to the generators' own ledgers, and the arithmetic a
second time to the fast device permutation and to the constraints of the stand-alone Poseidon2PermutationAir."""
import ctypes as C
import numpy as np
import pytest
import corner_felts as CF
import p2_trace_ref as PR
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import miden_air as MA  # noqa: E402
from miden_vm_amd.testing import chiplets_trace as CT, core_trace as CV  # noqa: E402

pytestmark = pytest.mark.gpu
P = MA.P
MULTS = [0, 1, 1 << 32, P - 1, P + 5]
CORNERS = [int(c) for c in CF.CORNERS] + [(1 << 32) + 1]
SHAPES = [(6, 0), (6, 1), (6, 3), (10, 62), (10, 63), (11, 64), (11, 65), (11, 127), (13, 255), (13, 256), (13, 257), (13, 511)]


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def state_pool(n):
    """[n, 12]: the all-zero state, every corner in all lanes, every corner in every lane position (the other lanes a seeded mixture of
    corners), non-canonical words, then uniform words of 64 bits (a 2^-32 share of them non-canonical)."""
    rng = np.random.default_rng(20)
    rows = [np.zeros(12, dtype=np.uint64)] + [np.full(12, c, dtype=np.uint64) for c in CORNERS]
    for c in CORNERS:
        for lane in range(12):
            s = CF.mixture((12,), 100 + lane).copy()
            s[lane] = c
            rows.append(s)
    rows += [np.full(12, (1 << 64) - 1, dtype=np.uint64), np.full(12, P, dtype=np.uint64),
             np.array([P + i for i in range(12)], dtype=np.uint64), np.array([(1 << 64) - 1 - i for i in range(12)], dtype=np.uint64)]
    fixed = np.stack(rows)
    rnd = rng.integers(0, 1 << 64, (max(0, n - fixed.shape[0]), 12), dtype=np.uint64)
    return np.concatenate([fixed, rnd])[:n]


POOL = state_pool(511)
assert POOL.shape == (511, 12) and (POOL >= np.uint64(P)).any()


def requests(k, shift=0):
    st = np.roll(POOL, -shift, axis=0)[:k]
    mu = np.array([MULTS[(i + shift) % len(MULTS)] for i in range(k)], dtype=np.uint64)
    return st, mu


# ---- 1, 2: a host list ----
@pytest.mark.parametrize("log_n,k", SHAPES)
def test_host_list_equals_the_restatement(ctx, log_n, k):
    # small k would only ever see the head of the pool: start it somewhere else per shape
    st, mu = requests(k, shift=0 if k >= 127 else 7 * log_n + k)
    t = pkg.poseidon2_trace(ctx, st, mu, log_n)
    got = t.download()
    exp = MA.poseidon2_permutation_trace(log_n, st, mu)
    assert got.shape == exp.shape == (1 << log_n, 16)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    assert (got < np.uint64(P)).all()
    info = t.p2_info
    assert (info.n_requests, info.n_input_rows, info.log_n, info.defect) == (k, 0, log_n, 0)


@pytest.mark.parametrize("k", [0, 3, 4, 63, 64])
def test_host_list_minimal_height(ctx, k):
    st, mu = requests(k, shift=k)
    t = pkg.poseidon2_trace(ctx, st, mu)
    log_n = PR.min_log_n(k)
    assert t.log_n == log_n == max(6, int(np.ceil(np.log2((k + 1) * 16))))
    assert (t.download() == MA.poseidon2_permutation_trace(log_n, st, mu)).all()


def test_arithmetic_against_the_fast_permutation_and_the_air(ctx):
    k, log_n = 257, 13
    st, mu = requests(k)
    t = pkg.poseidon2_trace(ctx, st, mu, log_n)
    got = t.download()
    out = ctx.poseidon2_permute(st % np.uint64(P))       # poseidon2_fast.cuh: another code path
    assert (got[15::16][:k, MA.COL_STATE:MA.COL_STATE + 12] == out).all()
    assert (got[0::16][:k, MA.COL_STATE:MA.COL_STATE + 12] == st % np.uint64(P)).all()
    air, lookup = MA.poseidon2_permutation_air()
    dev_air, dev_lk = pkg.DeviceAir(ctx, air), pkg.DeviceLookup(ctx, lookup)
    rnd = [(3, 5), (7, 11)]
    aux, fin = dev_lk.build_aux(t, rnd)
    for exact in (False, True):
        assert pkg.check_constraints(ctx, dev_air, t, aux=aux, randomness=rnd, aux_values=[fin], exact=exact) == ([], [])


# ---- 3: from a chiplets trace ----
def sample(seed):
    return CT.sample_chiplets(seed=seed, n_hperm=3 + seed % 3, n_bitwise=5 + seed, n_mem=12 + 4 * seed, merkle_depth=3 + seed % 2)


@pytest.fixture(scope="module")
def chiplets_cases():
    """name -> (chiplets matrix, expected Poseidon2 trace at the minimal height, k, input rows): computed once, never modified"""
    out = {}
    for seed in range(8):
        c = sample(seed)
        t, p2 = c.into_traces()
        out[f"sample{seed}"] = (t, p2, len(c.hasher.perm_requests), len(c.hasher.rows) // 2)
    for log_n in (8, 11, 13):
        t, p2 = CT.bulk_chiplets(log_n)
        k = (1 << log_n) // 16 - 1
        out[f"bulk{log_n}"] = (np.ascontiguousarray(t), p2, k, k)
    return out


CASE_NAMES = [f"sample{s}" for s in range(8)] + ["bulk8", "bulk11", "bulk13"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_from_chiplets_equals_the_generator(ctx, chiplets_cases, name):
    t, p2, k, n_in = chiplets_cases[name]
    m = pkg.Miden(ctx)
    log_n_p2 = p2.shape[0].bit_length() - 1
    for ask in (None, log_n_p2):
        tr, info = m.poseidon2_trace(pkg.Trace(ctx, t), ask)
        assert (info.n_requests, info.n_input_rows, info.log_n, info.defect, info.defect_row) == (k, n_in, log_n_p2, 0, 0)
        got = tr.download()
        assert (got == p2).all(), np.argwhere(got != p2)[:8]
    m.free()


def test_from_an_upload_in_flight_and_a_taller_trace(ctx, chiplets_cases):
    t, p2, k, n_in = chiplets_cases["bulk11"]
    host, owner = pkg.pinned_array(ctx.lib, t.shape)
    host[:] = t
    m = pkg.Miden(ctx)
    tr, info = m.poseidon2_trace(pkg.Trace.upload_async(ctx, host))     # no Trace.wait: the library orders itself after the copy
    assert (tr.download() == p2).all() and info.n_requests == k
    # many padding cycles
    t, p2, k, n_in = chiplets_cases["sample3"]
    tall = 12
    tr, info = m.poseidon2_trace(pkg.Trace(ctx, t), tall)
    st, mu, _ = PR.scan(t)
    assert info.log_n == tall and (tr.download() == MA.poseidon2_permutation_trace(tall, st, mu)).all()
    m.free()
    del owner


# ---- 4: the statement ----
def test_statement_proves_the_same_bytes(ctx):
    r = CV.prove_inputs(CV.CoreVM(stack_inputs=tuple(range(16))), CV.bench_program(4))
    assert r["core"].shape[0] <= 1 << 10
    pv, aux_in = r["public_values"], r["aux_inputs"]
    m = pkg.Miden(ctx)
    core, chiplets = pkg.Trace(ctx, r["core"]), pkg.Trace(ctx, r["chiplets"])
    derived, info = m.poseidon2_trace(chiplets)
    assert (derived.download() == r["poseidon2"]).all()
    assert m.check(core, chiplets, derived, pv, aux_in) == [] and m.check_balance(core, chiplets, derived, pv, aux_in) == []
    for hash_fn in ("poseidon2", "blake3"):
        got = m.prove(core, chiplets, derived, pv, aux_in, hash_fn=hash_fn)
        exp = m.prove(core, chiplets, pkg.Trace(ctx, r["poseidon2"]), pv, aux_in, hash_fn=hash_fn)
        assert got.bytes == exp.bytes
        ok, dig = pkg.verify_miden(pv, aux_in, got.bytes, hash_fn=hash_fn)
        assert ok and [int(x) for x in dig] == [int(x) for x in got.digest]
    m.free()


# ---- 5: defects and refusals ----
def refused(m, trace, log_n=None):
    with pytest.raises(pkg.MidenHipError) as e:
        m.poseidon2_trace(trace, log_n)
    return e.value


def good_call(ctx, m, case):
    t, p2, k, n_in = case
    tr, info = m.poseidon2_trace(pkg.Trace(ctx, t))
    assert (tr.download() == p2).all() and (info.n_requests, info.n_input_rows, info.defect) == (k, n_in, 0)


def test_defects_name_the_lowest_row_and_leave_the_context_usable(ctx, chiplets_cases):
    case = chiplets_cases["sample1"]
    t = case[0]
    m = pkg.Miden(ctx)
    rows = PR.input_rows(t)
    ids = t[rows, PR.COL_PERM_ID]
    # 2: the controller pair of the largest id moves one id up
    bad = t.copy()
    last = int(rows[ids == ids.max()][0])
    bad[last:last + 2, PR.COL_PERM_ID] += np.uint64(1)
    e = refused(m, pkg.Trace(ctx, bad))
    assert (e.info.defect, e.info.defect_row) == (2, int(ids.max())) and "defect 2" in str(e) and f"perm_id {int(ids.max())} " in str(e)
    good_call(ctx, m, case)
    # 3: a state cell of a repeated request's later input row
    rep = [int(r) for r in rows if (ids == t[r, PR.COL_PERM_ID]).sum() > 1]
    assert len(rep) >= 2
    bad = t.copy()
    bad[rep[-1], PR.COL_STATE + 11] = (int(bad[rep[-1], PR.COL_STATE + 11]) + 1) % P
    e = refused(m, pkg.Trace(ctx, bad))
    assert (e.info.defect, e.info.defect_row) == (3, rep[-1]) and "defect 3" in str(e) and f"row {rep[-1]} " in str(e)
    with pytest.raises(PR.Defect) as ref:
        PR.scan(bad)
    assert (ref.value.kind, ref.value.row) == (3, rep[-1])
    good_call(ctx, m, case)
    # 1: an id far beyond the table, reported before the conflict still in `bad` and before the gap its own id leaves
    assert int(rows[2]) not in rep
    bad[rows[2], PR.COL_PERM_ID] = 1 << 40
    e = refused(m, pkg.Trace(ctx, bad))
    assert (e.info.defect, e.info.defect_row) == (1, int(rows[2])) and "defect 1" in str(e)
    good_call(ctx, m, case)
    # ... and the smallest id that is out of range: N/2 + 1 entries
    bad = t.copy()
    bad[rows[0], PR.COL_PERM_ID] = t.shape[0] // 2 + 1
    e = refused(m, pkg.Trace(ctx, bad))
    assert (e.info.defect, e.info.defect_row) == (1, int(rows[0]))
    good_call(ctx, m, case)
    # 4: one row-doubling too few
    k = case[2]
    small = PR.min_log_n(k) - 1
    assert small >= 6
    e = refused(m, pkg.Trace(ctx, t), small)
    assert (e.info.defect, e.info.defect_row, e.info.n_requests, e.info.log_n) == (4, (1 << small) // 16 - 1, k, small) and "defect 4" in str(e)
    good_call(ctx, m, case)
    with pytest.raises(pkg.MidenHipError) as e4:
        pkg.poseidon2_trace(ctx, *requests(4), 6)
    assert "defect 4" in str(e4.value)
    good_call(ctx, m, case)
    m.free()


def test_refused_before_any_launch(ctx, chiplets_cases):
    case = chiplets_cases["sample0"]
    t = case[0]
    m = pkg.Miden(ctx)
    lib = ctx.lib
    good = pkg.Trace(ctx, t)
    m.poseidon2_trace(good)                                   # sets the argument types
    h, info = C.c_void_p(), pkg.P2TraceInfo()
    assert lib.mh_miden_poseidon2_trace(ctx.h, None, -1, C.byref(h), C.byref(info)) == 1 and "null" in lib.mh_last_error(ctx.h).decode()
    assert lib.mh_miden_poseidon2_trace(ctx.h, good.h, -1, None, C.byref(info)) == 1
    assert lib.mh_miden_poseidon2_trace(None, good.h, -1, C.byref(h), C.byref(info)) == 1
    pkg.poseidon2_trace(ctx, *requests(1))
    assert lib.mh_poseidon2_trace_build(ctx.h, None, None, 2, -1, C.byref(h), None) == 1
    assert lib.mh_poseidon2_trace_build(ctx.h, None, None, 0, -1, None, None) == 1
    assert "22" in str(refused(m, pkg.Trace(ctx, np.ascontiguousarray(t[:, :21]))))
    assert "log_n" in str(refused(m, good, 5)) and "log_n" in str(refused(m, good, 33))
    with pytest.raises(pkg.MidenHipError, match="log_n"):
        pkg.poseidon2_trace(ctx, *requests(1), 5)
    other = pkg.Ctx(0)
    try:
        assert "another context" in str(refused(m, pkg.Trace(other, t)))
    finally:
        other.close()
    good_call(ctx, m, case)
    m.free()


# ---- 6: memory ----
MB = 1 << 20


def test_three_rounds_leave_memory_where_the_first_left_it(ctx, chiplets_cases):
    """Ctx.mem_stats after rounds 2 and 3 of build + free equals the value after round 1: the pooled bytes and the table bytes exactly,
    the device memory in use (total - free, the pool included) within the 8 MB tests/test_gpu_soak.py allows a shared device.  A pool
    figure alone cannot see a buffer that never comes back, so the shapes are chosen to make any such buffer show in the device figure:
    2^20 chiplets rows give id tables of 8.4 MB, 60 000 listed requests an upload of 6.2 MB, and both traces are 2^20 x 16 = 128 MB --
    one buffer of either kind lost per round is more than 12 MB by round 3.  (The 40-byte word block of the scan is below anything a
    device figure resolves.)"""
    small = chiplets_cases["bulk11"][0]
    tall = np.zeros((1 << 20, 22), dtype=np.uint64)
    tall[:small.shape[0]] = small
    tall[small.shape[0]:, 0:5] = 1                               # fill_padding_rows: no chiplet's rows
    m = pkg.Miden(ctx)
    chip = pkg.Trace(ctx, tall)
    st, mu = np.random.default_rng(6).integers(0, P, (60000, 12), dtype=np.uint64), np.ones(60000, dtype=np.uint64)
    stats = []
    for _ in range(3):
        tr, info = m.poseidon2_trace(chip, 20)
        assert info.n_requests == chiplets_cases["bulk11"][2]
        lst = pkg.poseidon2_trace(ctx, st, mu, 20)
        tr.free()
        lst.free()
        stats.append(ctx.mem_stats())
    first = stats[0]
    for later in stats[1:]:
        assert (later["pool"], later["tables"], later["total"]) == (first["pool"], first["tables"], first["total"]), stats
        assert abs((later["total"] - later["free"]) - (first["total"] - first["free"])) <= 8 * MB, stats
    m.free()
    chip.free()
    ctx.trim()
