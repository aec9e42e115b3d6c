"""CPU-only parts of the device-built Keccak round and sponge traces (include/midenhip.h mh_keccak_round_program ..
mh_keccak_traces_build): the library's round programme against precompile_airs.keccak_round_slots(), the level schedule the
permutation kernel runs against a level computation restated here, and the ABI across header, Rust declarations, Python layer and the
built library."""
import ctypes as C
import os, re
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402

FUNCS = ["mh_keccak_round_program", "mh_keccak_round_levels", "mh_keccak_round_trace_build", "mh_keccak_traces_build"]
WIDTHS = [5, 5, 5, 5, 5, 5, 25, 25, 25, 1]


def library():
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return pkg.load_library()


def sources(slot, entry):
    """the slots of the SAME round that slot `slot` reads: a back-offset that stays inside the round"""
    op, _, back_a, back_b, _ = entry
    backs = [] if op == PA.OP_NOP else [back_a] + ([back_b] if op in (PA.OP_KXOR, PA.OP_KANDNOT, PA.OP_XORROL) else [])
    assert all(b > 0 for b in backs)
    return [slot - b for b in backs if b <= slot]


def restated_levels(program):
    level = [-1] * PA.ROUND_PERIOD
    for slot, entry in enumerate(program):
        if entry[0] == PA.OP_NOP:
            continue
        # a NOP slot that is read holds a constant of the round (RC): nothing to wait for
        level[slot] = max([0] + [level[s] + 1 for s in sources(slot, entry) if program[s][0] != PA.OP_NOP])
    return level


def test_round_program_is_the_generators():
    got = pkg.keccak_round_program(library())
    assert got == [tuple(int(x) for x in s) for s in PA.keccak_round_slots()]
    assert sum(1 for s in got if s[0] != PA.OP_NOP) == 106


def test_levels_are_the_restated_ones_and_only_read_below():
    lib = library()
    program, level = pkg.keccak_round_program(lib), pkg.keccak_round_levels(lib)
    assert level == restated_levels(PA.keccak_round_slots())
    assert [sum(1 for l in level if l == k) for k in range(10)] == WIDTHS and max(level) == 9
    assert all((l == -1) == (s[0] == PA.OP_NOP) for l, s in zip(level, program))
    for slot, entry in enumerate(program):
        for s in sources(slot, entry):
            assert level[s] < level[slot], (slot, s)       # same round: a lower level (or a constant, level -1)
    # a back-offset that leaves the round lands on the previous round's outputs, which no slot of this round writes
    outputs = {PA.SLOT_IOTA} | {PA.SLOT_CHI_XOR_BEGIN + i for i in range(24)}
    for slot, (op, _, back_a, back_b, _) in enumerate(program):
        for b in (back_a, back_b):
            if b > slot:
                assert slot - b + PA.ROUND_PERIOD in outputs, (slot, b)


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
    for name in ("mh_keccak_msg", "mh_keccak_traces_info"):
        assert re.search(r"typedef struct " + name + r" \{", h) and re.search(r"pub struct " + name + r" \{", rs), name
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    assert rust("mh_keccak_msg") == [("offset", "u64"), ("len", "u64"), ("chunk_head", "u64")]
    assert rust("mh_keccak_traces_info") == [("n_perms", "u64"), ("sponge_rows", "u64"), ("round_rows_needed", "u64"), ("sponge_rows_needed", "u64"),
                                             ("defect_kind", "i32"), ("defect_index", "u64")]
    dt = pkg.KECCAK_MSG_DTYPE
    assert dt.itemsize == 24 and list(dt.names) == ["offset", "len", "chunk_head"] and [dt.fields[n][1] for n in dt.names] == [0, 8, 16]
    assert pkg.KeccakTracesInfo._fields_ == [("n_perms", C.c_uint64), ("sponge_rows", C.c_uint64), ("round_rows_needed", C.c_uint64),
                                             ("sponge_rows_needed", C.c_uint64), ("defect_kind", C.c_int32), ("defect_index", C.c_uint64)]
    assert C.sizeof(pkg.KeccakTracesInfo) == 48 and pkg.KeccakTracesInfo.defect_index.offset == 40
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    assert args("mh_keccak_round_program") == rargs("mh_keccak_round_program") == ["out"]
    assert args("mh_keccak_round_levels") == rargs("mh_keccak_round_levels") == ["out"]
    assert args("mh_keccak_round_trace_build") == rargs("mh_keccak_round_trace_build") == ["ctx", "states", "n_perms", "log_n", "out", "outputs"]
    assert args("mh_keccak_traces_build") == rargs("mh_keccak_traces_build") == ["ctx", "bytes", "n_bytes", "msgs", "n_msgs", "log_round", "log_sponge",
                                                                                "round_out", "sponge_out", "digests", "info"]
    assert callable(pkg.keccak_round_trace) and callable(pkg.keccak_traces) and callable(pkg.Precompile.keccak_traces)
    sec = doc[doc.index("the precompile prover's Keccak round and sponge traces, built on the device"):]
    assert "Not in scope" in sec
    for word in ("chunk / node", "Poseidon2", "transcript", "uint", "EC"):
        assert word in sec[sec.index("Not in scope"):], word
