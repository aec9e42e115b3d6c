"""CPU-only parts of the device-built Poseidon2 chiplet trace (include/midenhip.h mh_poseidon2_chiplet_plan,
mh_poseidon2_chiplet_trace_build): the planner's starts and levels against a restatement written here, every planner refusal by kind and
index, the reference form of the generator's ledger (`Poseidon2Requires.lists(refs=True)`) resolved back to its literal blocks, the
counts of a session's ledger, and the ABI across header, Rust declarations, Python layer and the built library."""
import ctypes as C
import os, re
import numpy as np
import pytest
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

FUNCS = ["mh_poseidon2_chiplet_plan", "mh_poseidon2_chiplet_trace_build"]


def library():
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return pkg.load_library()


def records(absorptions):
    return np.array([(tuple(int(x) for x in cap), n, im, om) for cap, n, im, om in absorptions], dtype=pkg.P2C_ABSORPTION_DTYPE)


def restated_plan(n_blocks, refs):
    """start = the blocks before; level = 0 without a reference, else one above the highest level referenced"""
    start, level, at = [], [], 0
    for n in n_blocks:
        used = [int(r) for r in refs[at:at + n].reshape(-1) if r >= 0]
        level.append(1 + max(level[r] for r in used) if used else 0)
        start.append(at)
        at += n
    return start, level


@pytest.fixture(scope="module")
def session_ledger():
    rng = np.random.default_rng(9)
    _, traces, info = PT.precompile_session([b"", b"abc", bytes(rng.integers(0, 256, 300, dtype=np.uint8))])
    return info["ledgers"]["p2"], traces[1]


def test_planner_gives_the_restated_starts_and_levels():
    lib = library()
    rng = np.random.default_rng(5)
    for trial in range(20):
        n_abs = int(rng.integers(1, 40))
        n_blocks = [int(x) for x in rng.integers(1, 5, n_abs)]
        total = sum(n_blocks)
        refs = np.full((total, 2), -1, dtype=np.int64)
        at = 0
        for i, n in enumerate(n_blocks):
            for c in range(at, at + n):
                for h in range(2):
                    if i and rng.integers(0, 3) == 0:
                        refs[c, h] = rng.integers(0, i)
            at += n
        rec = records([([1, 2, 3, 4], n, 1, 0) for n in n_blocks])
        start, level, info = pkg.poseidon2_chiplet_plan(rec, total, refs, lib=lib)
        exp_start, exp_level = restated_plan(n_blocks, refs)
        assert [int(x) for x in start] == exp_start and [int(x) for x in level] == exp_level
        rows = max(16, 1 << (16 * total - 1).bit_length())
        assert (info.n_absorptions, info.n_cycles, info.n_levels, info.rows_needed, 1 << info.log_n, info.defect_kind) == \
            (n_abs, total, max(exp_level) + 1, rows, rows, 0)
        _, lit_level, lit_info = pkg.poseidon2_chiplet_plan(rec, total, None, lib=lib)
        assert not lit_level.any() and lit_info.n_levels == 1
    start, level, info = pkg.poseidon2_chiplet_plan([], 0, None, lib=lib)
    assert (start.size, level.size, info.n_levels, info.rows_needed, info.log_n, info.defect_kind) == (0, 0, 0, 16, 4, 0)
    # starts and levels may be left out
    info = pkg.Poseidon2ChipletInfo()
    rec = records([([0] * 4, 2, 1, 1), ([0] * 4, 1, 1, 0)])
    refs = np.array([[-1, -1], [-1, -1], [0, 0]], dtype=np.int64)
    lib.mh_poseidon2_chiplet_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(pkg.Poseidon2ChipletInfo)]
    assert lib.mh_poseidon2_chiplet_plan(rec.ctypes.data_as(C.c_void_p), 2, refs.ctypes.data_as(C.c_void_p), 3, None, None, C.byref(info)) == 0
    assert (info.n_levels, info.rows_needed) == (2, 64)


def test_every_planner_refusal_names_kind_and_index():
    lib = library()
    good = [([1, 2, 3, 4], 1, 1, 0), ([0] * 4, 3, 1, 1), ([0] * 4, 2, 1, 1)]           # cycles 0 | 1 2 3 | 4 5
    lit = np.full((6, 2), -1, dtype=np.int64)

    def with_ref(c, h, v):
        r = lit.copy()
        r[c, h] = v
        return r
    cases = [
        (good[:1] + [([0] * 4, 0, 1, 1)] + good[1:] + [([0] * 4, 0, 0, 0)], 6, lit, 2, 1),      # the lowest empty absorption
        (good, 5, lit[:5], 3, 2),                                                              # the third runs past n_cycles
        (good, 0, lit[:0], 3, 0),
        (good, 7, np.full((7, 2), -1, dtype=np.int64), 3, 3),                                  # the list ends short: n_abs
        (good[:2] + [([0] * 4, 1 << 63, 1, 1), ([0] * 4, 1 << 63, 1, 1)], 6, lit, 3, 2),        # counts whose sum would wrap
        (good, 6, with_ref(0, 0, 0), 4, 0),                                                    # absorption 0 has nothing earlier
        (good, 6, with_ref(2, 1, 1), 4, 5),                                                    # itself
        (good, 6, with_ref(4, 0, 2), 4, 8),
        (good, 6, with_ref(5, 1, -2), 4, 11),                                                  # neither -1 nor an index
        (good, 6, with_ref(3, 0, 1 << 40), 4, 6),
        ([([0] * 4, (1 << 20) + 1, 1, 1)], (1 << 20) + 1, None, 5, (1 << 20) + 1),
    ]
    for absorptions, n_cycles, refs, kind, index in cases:
        with pytest.raises(pkg.MidenHipError) as e:
            pkg.poseidon2_chiplet_plan(records(absorptions), n_cycles, refs, lib=lib)
        info = e.value.info
        assert (info.defect_kind, info.defect_index) == (kind, index), (kind, index, info)
        assert (info.n_absorptions, info.n_cycles) == (len(absorptions), n_cycles)
    # the lowest kind first: an empty absorption (2) before the sum (3) before a reference (4)
    with pytest.raises(pkg.MidenHipError) as e:
        pkg.poseidon2_chiplet_plan(records(good + [([0] * 4, 0, 0, 0)]), 9, np.full((9, 2), 7, dtype=np.int64), lib=lib)
    assert (e.value.info.defect_kind, e.value.info.defect_index) == (2, 3)
    with pytest.raises(pkg.MidenHipError) as e:
        pkg.poseidon2_chiplet_plan(records(good), 9, np.full((9, 2), 7, dtype=np.int64), lib=lib)
    assert (e.value.info.defect_kind, e.value.info.defect_index) == (3, 3)
    # a needed pointer that is NULL
    info = pkg.Poseidon2ChipletInfo()
    lib.mh_poseidon2_chiplet_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(pkg.Poseidon2ChipletInfo)]
    assert lib.mh_poseidon2_chiplet_plan(None, 3, None, 6, None, None, C.byref(info)) == 1
    assert (info.defect_kind, info.defect_index, info.n_absorptions, info.n_cycles) == (1, 0, 3, 6)
    assert lib.mh_poseidon2_chiplet_plan(None, 0, None, 0, None, None, None) == 1
    # the largest ledger is taken
    _, _, info = pkg.poseidon2_chiplet_plan(records([([0] * 4, 1 << 20, 1, 1)]), 1 << 20, None, lib=lib)
    assert (info.rows_needed, info.log_n) == (1 << 24, 24)


def test_reference_form_resolves_to_the_literal_blocks(session_ledger):
    p2, _ = session_ledger
    absorptions, lit, none = p2.lists()
    absorptions_r, poisoned, refs = p2.lists(refs=True)
    assert absorptions == absorptions_r and (none == -1).all() and lit.shape == poisoned.shape == (p2.next_seq, 8)
    assert [a[1] for a in absorptions] == [len(a[1]) for a in p2.absorptions]
    resolved = poisoned.copy()
    owner = np.repeat(np.arange(len(absorptions)), [a[1] for a in absorptions])
    for c, h in np.argwhere(refs >= 0):
        assert refs[c, h] < owner[c]
        assert (poisoned[c, 4 * h:4 * h + 4] == PT.Poseidon2Requires.POISON).all()
        resolved[c, 4 * h:4 * h + 4] = p2.digest(int(refs[c, h]))
    assert (resolved == lit).all()
    assert (poisoned[np.repeat(refs, 4, axis=1) < 0] == lit[np.repeat(refs, 4, axis=1) < 0]).all()


def test_session_ledger_counts(session_ledger):
    """The session of tests/test_gpu_poseidon2_chiplet.py: the reference form must not degrade to literals."""
    p2, main = session_ledger
    absorptions, blocks, refs = p2.lists(refs=True)
    assert (len(absorptions), blocks.shape[0], int((refs >= 0).sum())) == (49, 59, 55)
    _, level, info = pkg.poseidon2_chiplet_plan(records(absorptions), blocks.shape[0], refs, lib=library())
    assert [int(x) for x in np.bincount(level)] == [22, 10, 5, 5, 2, 1, 1, 1, 1, 1] and info.n_levels == 10
    assert info.rows_needed == main.shape[0] == 1024


def test_abi_agrees_across_header_rust_python_and_library():
    doc = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    lib = library()
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
        assert hasattr(lib, f), f
    for name in ("mh_p2c_absorption", "mh_p2c_info"):
        assert re.search(r"typedef struct " + name + r" \{", h) and re.search(r"pub struct " + name + r" \{", rs), name
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    assert rust("mh_p2c_absorption") == [("cap", "[u64; 4]"), ("n_blocks", "u64"), ("in_mult", "u64"), ("out_mult", "u64")]
    assert rust("mh_p2c_info") == [("n_absorptions", "u64"), ("n_cycles", "u64"), ("n_levels", "u64"), ("rows_needed", "u64"), ("log_n", "i32"),
                                   ("defect_kind", "i32"), ("defect_index", "u64")]
    body = re.search(r"typedef struct mh_p2c_info \{(.*?)\} mh_p2c_info", h, flags=re.S).group(1)
    fields = [(d.split()[0], n.strip()) for d in body.split(";") if d.strip() for n in d.split(None, 1)[1].split(",")]
    assert fields == [("uint64_t", "n_absorptions"), ("uint64_t", "n_cycles"), ("uint64_t", "n_levels"), ("uint64_t", "rows_needed"), ("int32_t", "log_n"),
                      ("int32_t", "defect_kind"), ("uint64_t", "defect_index")]
    dt = pkg.P2C_ABSORPTION_DTYPE
    assert dt.itemsize == 56 and list(dt.names) == ["cap", "n_blocks", "in_mult", "out_mult"] and [dt.fields[n][1] for n in dt.names] == [0, 32, 40, 48]
    assert pkg.Poseidon2ChipletInfo._fields_ == [("n_absorptions", C.c_uint64), ("n_cycles", C.c_uint64), ("n_levels", C.c_uint64), ("rows_needed", C.c_uint64),
                                                 ("log_n", C.c_int32), ("defect_kind", C.c_int32), ("defect_index", C.c_uint64)]
    assert C.sizeof(pkg.Poseidon2ChipletInfo) == 48 and pkg.Poseidon2ChipletInfo.defect_index.offset == 40
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    assert args("mh_poseidon2_chiplet_plan") == rargs("mh_poseidon2_chiplet_plan") == ["abs", "n_abs", "refs", "n_cycles", "start", "level", "info"]
    assert args("mh_poseidon2_chiplet_trace_build") == rargs("mh_poseidon2_chiplet_trace_build") == [
        "ctx", "abs", "n_abs", "blocks", "refs", "n_cycles", "log_n", "out", "digests", "outputs", "info"]
    assert callable(pkg.poseidon2_chiplet_plan) and callable(pkg.poseidon2_chiplet_trace) and callable(pkg.Precompile.poseidon2_trace)
    sec = doc[doc.index("the precompile prover's Poseidon2 chiplet trace, built on the device"):]
    assert "Not in scope" in sec
    for word in ("Interning".lower(), "chunk / node", "transcript", "uint", "EC", "sharded"):
        assert word in sec[sec.index("Not in scope"):], word
