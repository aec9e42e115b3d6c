"""CPU: mh_lmcs_verify (csrc/lmcs_verify.cpp, csrc/lmcs_plan.hpp) -- the counterpart of mh_tree_open -- against openings made by the
CPU checker (oracle_binding.commit_traces, the reference's prove_batch restated): accepted under all five configurations, every
damage class rejected with a reason, the plan's sibling count equal to the length of the checker's stream.  The call-level refusals
of the batch entries that need no device are here too."""
import ctypes as C
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
from __graft_entry__ import load_package

pkg = load_package()

CONFIGS = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
ALIGN = {"poseidon2": 8, "blake3": 1, "keccak": 17, "rpo": 8, "rpx": 8}
LOG_BLOWUP = 1
DEPTH = 4  # the taller matrix has 8 rows
INDEX_SETS = {
    "single": [5],
    "two_siblings": [6, 7],
    "two_apart": [1, 12],
    "all_leaves": list(range(16)),
    "duplicated_unsorted": [9, 2, 9, 15, 2, 3],
}
_cache = {}


def traces():
    rng = np.random.default_rng(11)
    return [rng.integers(0, A.P, (4, 3), dtype=np.uint64), rng.integers(0, A.P, (8, 9), dtype=np.uint64)]


def opening(cfg, name):
    """(root, widths, indices as the caller gives them, fields, commitments[k][4]) from the checker; made once, never changed."""
    if (cfg, name) not in _cache:
        ob.set_lmcs(cfg)
        try:
            idx = INDEX_SETS[name]
            r = ob.commit_traces(traces(), LOG_BLOWUP, sorted(set(idx)), ALIGN[cfg])
        finally:
            ob.set_lmcs("poseidon2")
        for a in (r["root"], r["fields"], r["commitments"]):
            a.setflags(write=False)
        _cache[(cfg, name)] = (r["root"], [3, 9], idx, r["fields"], r["commitments"])
    return _cache[(cfg, name)]


def check(cfg, root, widths, idx, fields, commits, log_height=DEPTH, salt=0, alignment=None):
    return pkg.lmcs_verify(dict(root=root, log_height=log_height, widths=widths, alignment=alignment or ALIGN[cfg], indices=idx,
                                fields=fields, commitments=commits), cfg, salt)


def expected_siblings(idx, depth):
    """digests an opening streams: per level, the opened nodes whose sibling is not opened"""
    level, n = sorted(set(idx)), 0
    for _ in range(depth):
        s = set(level)
        n += sum(1 for x in level if (x ^ 1) not in s)
        level = sorted({x >> 1 for x in level})
    return n


@pytest.mark.parametrize("name", list(INDEX_SETS))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_accepts_the_checkers_openings(cfg, name):
    root, widths, idx, f, c = opening(cfg, name)
    # the plan's counts are exact: the checker's streams pass the length checks only if both agree with the plan
    assert c.shape[0] == expected_siblings(idx, DEPTH)
    if name == "all_leaves":
        assert c.shape[0] == 0
    ok, why = check(cfg, root, widths, idx, f, c)
    assert ok, why
    assert why == ""


@pytest.mark.parametrize("name", list(INDEX_SETS))
def test_sibling_count_is_exact(name):
    """one digest more or fewer than the checker streamed is a length error, not a root mismatch: the plan knows the count"""
    root, widths, idx, f, c = opening("poseidon2", name)
    ok, why = check("poseidon2", root, widths, idx, f, np.concatenate([c, np.ones((1, 4), dtype=np.uint64)]))
    assert not ok and "trailing data in the commitment stream" in why
    if c.shape[0]:
        ok, why = check("poseidon2", root, widths, idx, f, c[:-1])
        assert not ok and "commitment stream too short" in why


def damages(root, widths, idx, f, c):
    """name -> (arguments of check(), a word the reason must contain)"""
    bad_f = f.copy(); bad_f[7] = (int(bad_f[7]) + 1) % A.P
    bad_c = c.copy(); bad_c[1, 2] = (int(bad_c[1, 2]) + 1) % A.P
    bad_root = root.copy(); bad_root[0] = (int(bad_root[0]) + 1) % A.P
    noncanon = f.copy(); noncanon[3] = A.P
    one = np.ones((1, 4), dtype=np.uint64)
    return {
        "flipped_felt": ((root, widths, idx, bad_f, c), "Merkle root mismatch"),
        "flipped_sibling_word": ((root, widths, idx, f, bad_c), "Merkle root mismatch"),
        "wrong_root": ((bad_root, widths, idx, f, c), "Merkle root mismatch"),
        "one_felt_too_few": ((root, widths, idx, f[:-1], c), "field stream too short"),
        "one_felt_too_many": ((root, widths, idx, np.append(f, np.uint64(0)), c), "trailing data in the field stream"),
        "one_digest_too_few": ((root, widths, idx, f, c[:-1]), "commitment stream too short"),
        "one_digest_too_many": ((root, widths, idx, f, np.concatenate([c, one])), "trailing data in the commitment stream"),
        "non_canonical_felt": ((root, widths, idx, noncanon, c), "non-canonical field element"),
        "index_outside_the_tree": ((root, widths, idx + [1 << DEPTH], f, c), "outside the tree"),
    }


DAMAGES = ["flipped_felt", "flipped_sibling_word", "wrong_root", "one_felt_too_few", "one_felt_too_many", "one_digest_too_few",
           "one_digest_too_many", "non_canonical_felt", "index_outside_the_tree"]


@pytest.mark.parametrize("damage", DAMAGES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_rejects_damage_with_a_reason(cfg, damage):
    args, word = damages(*opening(cfg, "duplicated_unsorted"))[damage]
    ok, why = check(cfg, *args)
    assert not ok
    assert why.startswith("opening rejected: ") and word in why, why


def test_refuses_bad_configuration_and_shape():
    root, widths, idx, f, c = opening("poseidon2", "single")
    lib = pkg.load_library()
    o = pkg.LmcsOpening.make(root, DEPTH, widths, 8, idx, f, c)
    err = C.create_string_buffer(256)
    lib.mh_lmcs_verify.argtypes = [C.c_int, C.c_int, C.POINTER(pkg.LmcsOpening), C.c_char_p, C.c_size_t]
    for lmcs, salt, word in [(5, 0, "unknown LMCS"), (-1, 0, "unknown LMCS"), (0, -1, "salt_elems"), (0, pkg.MH_MAX_SALT_ELEMS + 1, "salt_elems")]:
        assert lib.mh_lmcs_verify(lmcs, salt, C.byref(o), err, 256) == 1 and word in err.value.decode()
    assert lib.mh_lmcs_verify(0, 0, None, err, 256) == 1 and "null" in err.value.decode()
    assert lib.mh_lmcs_verify(0, 0, C.byref(o), None, 0) == 0  # no room for a reason is fine
    assert not check("poseidon2", root, widths, [], f, c)[0]                   # no index
    assert not check("poseidon2", root, widths, idx, f, c, log_height=33)[0]   # taller than any domain
    assert not check("poseidon2", root, widths, idx, f, c, log_height=-1)[0]
    assert not check("poseidon2", root, widths, idx, f, c, alignment=1)[0]     # another alignment: other lengths
    ok, why = check("poseidon2", root, widths, idx, f, c, salt=1)              # an unsalted opening read as salted: too short
    assert not ok and "field stream too short" in why
    bad_c = c.copy(); bad_c[0, 0] = A.P
    ok, why = check("poseidon2", root, widths, idx, f, bad_c)
    assert not ok and "non-canonical digest element" in why
    root_b, _, idx_b, f_b, c_b = opening("blake3", "single")
    bad_c = c_b.copy(); bad_c[0, 0] = np.uint64(2**64 - 1)                     # a byte digest's words are not felts: hashed, not refused
    ok, why = check("blake3", root_b, widths, idx_b, f_b, bad_c)
    assert not ok and "Merkle root mismatch" in why


@pytest.mark.parametrize("salt", [1, 8])
def test_accepts_a_salted_opening(salt):
    """The checker has no hiding LMCS; its Poseidon2 sponge and compression build one here: 8 leaves, one matrix of width 3, the salt
    absorbed after the aligned row as one more (short) matrix (lmcs/proof.rs:108-137)."""
    rng = np.random.default_rng(5)
    rows = np.zeros((8, 8), dtype=np.uint64)
    rows[:, :3] = rng.integers(0, A.P, (8, 3), dtype=np.uint64)
    salts = rng.integers(0, A.P, (8, salt), dtype=np.uint64)
    layer = [ob.sponge_absorb(ob.sponge_absorb(np.zeros(12, dtype=np.uint64), rows[i]), salts[i])[:4] for i in range(8)]
    layers = [layer]
    while len(layer) > 1:
        layer = [ob.compress(layer[2 * i], layer[2 * i + 1]) for i in range(len(layer) // 2)]
        layers.append(layer)
    idx = [1, 6]
    fields = np.concatenate([np.concatenate([rows[i], salts[i]]) for i in idx])
    commits = np.array([layers[0][0], layers[0][7], layers[1][1], layers[1][2]], dtype=np.uint64)  # bottom-up, left to right
    ok, why = check("poseidon2", layers[-1][0], [3], idx, fields, commits, log_height=3, salt=salt)
    assert ok, why
    bad = fields.copy(); bad[8] = (int(bad[8]) + 1) % A.P  # the first salt felt
    assert not check("poseidon2", layers[-1][0], [3], idx, bad, commits, log_height=3, salt=salt)[0]
    assert not check("poseidon2", layers[-1][0], [3], idx, fields, commits, log_height=3, salt=0)[0]


def test_batch_entries_refuse_a_null_context():
    """the call-level refusals that need no device; with a context they are in tests/test_gpu_verify_batch.py"""
    lib = pkg.load_library()
    root, widths, idx, f, c = opening("poseidon2", "single")
    o = pkg.LmcsOpening.make(root, DEPTH, widths, 8, idx, f, c)
    ok = (C.c_int * 1)(7)
    lib.mh_lmcs_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(pkg.LmcsOpening), C.POINTER(C.c_int)]
    assert lib.mh_lmcs_verify_batch(None, 0, 0, 1, C.byref(o), ok) == 1
    assert lib.mh_lmcs_verify_batch(None, 0, 0, 0, None, None) == 1
    assert ok[0] == 7
    lib.mh_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p]
    assert lib.mh_verify_batch(None, 0, 0, None, 1, None, None, None, None, 0, None, None) == 1
    lib.mh_verify_miden_batch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    assert lib.mh_verify_miden_batch(None, 0, 0, None, None) == 1
