"""The verifier derives its own setup commitment (host only, no GPU): mh_commit_host, mh_precompile_setup_root and the root pinned by
mh_verify_precompile.

  * mh_commit_host == the CPU checker's commit_traces root under each of the five hashers, at the smallest shapes at which a distinct
    path can go wrong: a tree of two leaves (log_blowup 0), a single absorb block, a width above the sponge's rate (a second absorb
    block; the row crosses a 64-byte Blake3 block), mixed heights (lifting, two height groups, state carried between them) at
    log_blowup 1, 2 and 3, and cells >= p;
  * every argument refusal of the header;
  * mh_precompile_setup_root == the checker's commitment of the 2^16 x 4 byte-pair table at log_blowup 3, stable, thread-safe;
  * mh_verify_precompile compares a given root with the derived one BEFORE the proof is read, and derives it when given none;
  * the CPU checker's session proof at the production parameters verifies with the derived root as with the explicit one;
  * mh_precompile_pre_observe refuses parameters it cannot frame."""
import ctypes as C
import threading
import numpy as np
import pytest
import oracle_binding as ob
import proof_parser
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA, protocol  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

HASHERS = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
P = pkg.P
MH_ERR_INVALID = 1
u64p, u8p, szp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)


def matrix(seed, log_h, w):
    return np.random.default_rng(seed).integers(0, P, (1 << log_h, w), dtype=np.uint64)


def mixed():
    """proof order (ascending height): lifting, two height groups, the state carried from the first to the second"""
    return [matrix(10, 3, 3), matrix(11, 5, 10), matrix(12, 5, 1)]


CASES = {
    "two_leaves": (lambda: [matrix(1, 1, 1)], 0),       # mh_commit_traces accepts log_blowup 0
    "8x5": (lambda: [matrix(2, 3, 5)], 1),
    "64x9": (lambda: [matrix(3, 6, 9)], 2),             # width above the rate of 8; 72-byte rows cross a Blake3 block
    "mixed_lb1": (mixed, 1),
    "mixed_lb2": (mixed, 2),
    "mixed_lb3": (mixed, 3),
}


def oracle_root(hasher, mats, log_blowup):
    ob.set_lmcs(hasher)
    try:
        return ob.commit_traces(mats, log_blowup)["root"]
    finally:
        ob.set_lmcs("poseidon2")


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("hasher", HASHERS)
def test_root_equals_the_checkers(hasher, case):
    make, lb = CASES[case]
    mats = make()
    assert list(pkg.commit_host(mats, lb, lmcs=hasher)) == list(oracle_root(hasher, mats, lb))


@pytest.mark.parametrize("hasher", HASHERS)
def test_cells_are_reduced_mod_p(hasher):
    """cells >= p and 2^64 - 1 commit like their canonical values (every upload path canonicalises)"""
    m = matrix(4, 3, 5)
    raw = m.copy()
    raw[0, 0], raw[1, 2], raw[7, 4], raw[3, 3] = np.uint64(P), np.uint64(2**64 - 1), np.uint64(P + 5), np.uint64(int(m[3, 3]) % (2**32 - 1) + P)
    canon = (raw.astype(object) % P).astype(np.uint64)
    assert (raw != canon).sum() == 4
    got = pkg.commit_host([raw], 1, lmcs=hasher)
    assert list(got) == list(pkg.commit_host([canon], 1, lmcs=hasher)) == list(oracle_root(hasher, [canon], 1))


def call_commit_host(lmcs, n_mats, mats, log_heights, widths, log_blowup, null=()):
    """the raw entry: `null` names the pointer arguments passed as NULL"""
    lib = pkg.load_library()
    lib.mh_commit_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    keep = [np.ascontiguousarray(m, dtype=np.uint64) for m in mats]
    ptrs = (C.c_void_p * max(1, len(keep)))(*[None if i in null else m.ctypes.data for i, m in enumerate(keep)])
    lhs = (C.c_uint8 * max(1, len(keep)))(*log_heights)
    ws = (C.c_size_t * max(1, len(keep)))(*widths)
    root, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(256)
    rc = lib.mh_commit_host(lmcs, n_mats, None if "rowmajor" in null else ptrs, None if "log_heights" in null else lhs,
                            None if "widths" in null else ws, log_blowup, None if "root" in null else root.ctypes.data, err, 256)
    return rc, err.value.decode()


def test_argument_refusals():
    m = matrix(5, 3, 2)
    ok = dict(lmcs=0, n_mats=1, mats=[m], log_heights=[3], widths=[2], log_blowup=1)
    rc, msg = call_commit_host(**ok)
    assert rc == 0 and msg == ""
    bad = [dict(null=("rowmajor",)), dict(null=("log_heights",)), dict(null=("widths",)), dict(null=("root",)), dict(null=(0,)),
           dict(n_mats=0), dict(n_mats=-1), dict(widths=[0]), dict(log_blowup=-1), dict(log_blowup=9),
           dict(log_heights=[32]), dict(log_heights=[25], log_blowup=8), dict(lmcs=-1), dict(lmcs=5)]
    for change in bad:
        rc, msg = call_commit_host(**dict(ok, **change))
        assert rc == MH_ERR_INVALID and msg, (change, rc, msg)
    # heights must ascend, as for mh_commit_traces
    rc, msg = call_commit_host(0, 2, [matrix(6, 4, 1), m], [4, 3], [1, 2], 1)
    assert rc == MH_ERR_INVALID and "ascending" in msg
    with pytest.raises(pkg.MidenHipError):
        pkg.commit_host([m], 9)


def byte_pair_table():
    i = np.arange(1 << 16, dtype=np.uint64)
    a, b = i >> np.uint64(8), i & np.uint64(0xff)
    return np.stack([a, b, (~a & np.uint64(0xff)) & b, a ^ b], axis=1)


def raw_setup_root(lmcs_id):
    lib = pkg.load_library()
    lib.mh_precompile_setup_root.argtypes = [C.c_int, C.c_void_p]
    root = np.zeros(4, dtype=np.uint64)
    return lib.mh_precompile_setup_root(lmcs_id, root.ctypes.data), root


def test_setup_root_first_called_from_four_threads():
    """Runs before any other test of this file derives a root (pytest runs a file's tests in order; the parity tests above do not):
    the four first calls per hasher race for the derivation and must all return the one root."""
    for hasher in HASHERS:
        got = [None] * 4

        def work(k):
            got[k] = pkg.precompile_setup_root(hasher)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert all(g is not None and list(g) == list(got[0]) for g in got), (hasher, got)
    assert len({tuple(int(x) for x in pkg.precompile_setup_root(h)) for h in HASHERS}) == 5


@pytest.mark.parametrize("hasher", HASHERS)
def test_setup_root_equals_the_checkers_table_commitment(hasher):
    assert np.asarray(PA.byte_pair_preprocessed(), dtype=np.uint64).tolist() == byte_pair_table().tolist()
    first = pkg.precompile_setup_root(hasher)
    assert list(first) == list(oracle_root(hasher, [byte_pair_table()], protocol.PROD_PARAMS["log_blowup"]))
    assert list(pkg.precompile_setup_root(hasher)) == list(first)
    assert raw_setup_root(5)[0] == MH_ERR_INVALID and raw_setup_root(-1)[0] == MH_ERR_INVALID
    lib = pkg.load_library()
    lib.mh_precompile_setup_root.argtypes = [C.c_int, C.c_void_p]
    assert lib.mh_precompile_setup_root(0, None) == MH_ERR_INVALID


@pytest.mark.parametrize("hasher", HASHERS)
def test_root_is_pinned_before_the_proof_is_read(hasher):
    """No proof needed: a root one bit off is refused for being the wrong setup commitment even with no proof bytes at all; with no
    root given the same call gets as far as the proof bytes."""
    setup = [int(x) for x in pkg.precompile_setup_root(hasher)]
    public_root = [1, 2, 3, 4]
    for word in range(4):
        flipped = list(setup)
        flipped[word] ^= 1
        ok, msg = pkg.verify_precompile(flipped, public_root, b"", hash_fn=hasher)
        assert not ok and "setup commitment" in msg and "preprocessed_root" in msg, msg
    ok, msg = pkg.verify_precompile(None, public_root, b"", hash_fn=hasher)
    assert not ok and "proof bytes" in msg and "setup" not in msg, msg
    ok, msg = pkg.verify_precompile(setup, public_root, b"", hash_fn=hasher)
    assert not ok and "proof bytes" in msg and "setup" not in msg, msg
    # the raw entry: MH_ERR_INVALID both times
    lib = pkg.load_library()
    lib.mh_verify_precompile.argtypes = [C.c_int, u64p, u64p, C.c_void_p, C.c_size_t, u64p, C.c_char_p, C.c_size_t]
    pub, dig, err, buf = np.array(public_root, dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.create_string_buffer(256), (C.c_uint8 * 1)()
    bad = np.array(setup, dtype=np.uint64)
    bad[3] ^= np.uint64(1 << 40)
    lmcs = pkg.Ctx.LMCS[hasher]
    assert lib.mh_verify_precompile(lmcs, bad.ctypes.data_as(u64p), pub.ctypes.data_as(u64p), buf, 0, dig.ctypes.data_as(u64p), err, 256) == MH_ERR_INVALID
    assert b"setup commitment" in err.value
    assert lib.mh_verify_precompile(lmcs, None, pub.ctypes.data_as(u64p), buf, 0, dig.ctypes.data_as(u64p), err, 256) == MH_ERR_INVALID
    assert b"proof bytes" in err.value


def test_derived_root_equals_explicit_root_on_the_checkers_session_proof(fast_oracle_build):
    """The CPU checker's proof of the session tests/test_gpu_precompile_c_abi.py builds, at the production parameters: accepted with the
    root derived (None) and with the explicit root, same digest; the checker's own setup commitment is the derived one."""
    pairs, traces, info = PT.precompile_session([b"", b"abc", b"abc", bytes(range(200))], lambda *a: ob.lookup_build_aux(*a))
    airs, root = [p[0] for p in pairs], info["public_root"]
    exp = ob.prove(airs, traces, root, dict(protocol.PROD_PARAMS), init_state=protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST))
    data = proof_parser.serialize([int(h) for h in exp["log_heights"]], exp["fields"], exp["commitments"])
    setup = pkg.precompile_setup_root("poseidon2")
    assert [int(x) for x in exp["preprocessed_root"]] == [int(x) for x in setup]
    ok_derived, dig_derived = pkg.verify_precompile(None, root, data)
    ok_explicit, dig_explicit = pkg.verify_precompile(setup, root, data)
    assert ok_derived and ok_explicit, (dig_derived, dig_explicit)
    assert list(dig_derived) == list(dig_explicit) == [int(x) for x in exp["digest"]]
    ok, msg = pkg.verify_precompile(None, [(int(root[0]) + 1) % P] + [int(x) for x in root[1:]], data)
    assert not ok and "setup" not in msg
    wrong = [int(x) for x in setup]
    wrong[0] = (wrong[0] + 1) % P
    ok, msg = pkg.verify_precompile(wrong, root, data)
    assert not ok and "setup commitment" in msg


def test_pre_observe_refuses_parameters_it_cannot_frame():
    lib = pkg.load_library()
    good = pkg.PcsParams.from_dict(protocol.PROD_PARAMS)
    root, out = np.zeros(4, dtype=np.uint64), np.zeros(19, dtype=np.uint64)
    call = lambda p: lib.mh_precompile_pre_observe(C.byref(p), root.ctypes.data_as(u64p), root.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
    assert call(good) == 0
    for arity in (-1, 0, 4, 64):
        p = pkg.PcsParams.from_dict(dict(protocol.PROD_PARAMS, log_folding_arity=arity))
        assert call(p) == MH_ERR_INVALID, arity
    for field in ("log_blowup", "log_final_degree", "num_queries", "query_pow_bits", "deep_pow_bits", "folding_pow_bits"):
        p = pkg.PcsParams.from_dict(dict(protocol.PROD_PARAMS, **{field: -1}))
        assert call(p) == MH_ERR_INVALID, field
