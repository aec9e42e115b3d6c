"""CPU: mh_lmcs_witness_size / mh_lmcs_witness (csrc/lmcs_verify.cpp, lmcs_plan::PathTable) -- an opening read back as a Merkle
witness -- against the CPU checker.  The independent yardstick for a path is the checker's own SINGLE-index opening of the same
leaf: for one leaf the commitment stream is its authentication path, bottom up.  Nodes and leaf digests are held to the checker's
full layers.  Shapes, configurations and index sets are those of tests/test_lmcs_verify.py."""
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
DEPTH = 4
WIDTHS = [3, 9]
INDEX_SETS = {
    "single": [5],
    "two_siblings": [6, 7],
    "two_apart": [1, 12],
    "all_leaves": list(range(16)),
    "duplicated_unsorted": [9, 2, 9, 15, 2, 3],
}
SENTINEL = 0xA5A5A5A5A5A5A5A5
_cache = {}


def traces():
    rng = np.random.default_rng(11)
    return [rng.integers(0, A.P, (4, 3), dtype=np.uint64), rng.integers(0, A.P, (8, 9), dtype=np.uint64)]


def checker(cfg, idx, want_lde=False):
    """the checker's opening of the sorted unique indices; made once per (cfg, indices), never changed"""
    key = (cfg, tuple(idx), want_lde)
    if key not in _cache:
        ob.set_lmcs(cfg)
        try:
            r = ob.commit_traces(traces(), LOG_BLOWUP, sorted(set(idx)), ALIGN[cfg], want_lde=want_lde)
            if want_lde:
                r["layers"] = ob.lmcs_build(r["ldes"], want_layers=True)[1]
        finally:
            ob.set_lmcs("poseidon2")
        _cache[key] = r
    return _cache[key]


def opening(cfg, idx, **change):
    r = checker(cfg, idx)
    return dict(dict(root=r["root"], log_height=DEPTH, widths=WIDTHS, alignment=ALIGN[cfg], indices=list(idx), fields=r["fields"],
                     commitments=r["commitments"]), **change)


def distinct_ancestors(idx, depth):
    level, n = set(idx), 0
    for _ in range(depth):
        level = {x >> 1 for x in level}
        n += len(level)
    return n


def layer(layers, l, height=1 << DEPTH):
    """level l of the checker's layers (leaves first)"""
    off = 2 * height - ((2 * height) >> l)
    return layers[off:off + (height >> l)]


@pytest.mark.parametrize("name", list(INDEX_SETS))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_paths_equal_the_checkers_single_openings(cfg, name):
    idx = INDEX_SETS[name]
    o = opening(cfg, idx)
    w = pkg.lmcs_witness(o, cfg)
    uniq = sorted(set(idx))
    assert list(w.indices) == uniq
    assert w.leaf_digests.shape == (len(uniq), 4) and w.paths.shape == (len(uniq), DEPTH, 4)
    row_len = o["fields"].size // len(uniq)
    for q, i in enumerate(uniq):
        single = checker(cfg, [i])
        assert single["commitments"].shape == (DEPTH, 4)
        assert (w.path(i) == single["commitments"]).all(), (i, w.path(i), single["commitments"])
        # ... and (rows of leaf q, path(q)) is an opening of its own
        ok, why = pkg.lmcs_verify(dict(o, indices=[i], fields=o["fields"][q * row_len:(q + 1) * row_len], commitments=w.path(i)), cfg)
        assert ok, why
    with pytest.raises(KeyError):
        w.path(4 if 4 not in uniq else 16)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_a_path_element_may_be_the_neighbours_leaf_hash(cfg):
    """in [6, 7] nothing is streamed for level 0: path(6)[0] is the leaf digest of 7, which the checker streams when 6 is opened alone"""
    w = pkg.lmcs_witness(opening(cfg, [6, 7]), cfg)
    from_checker = checker(cfg, [6])["commitments"][0]
    assert (w.leaf_digests[1] == from_checker).all()
    assert (w.path(6)[0] == w.leaf_digests[1]).all() and (w.path(7)[0] == w.leaf_digests[0]).all()


@pytest.mark.parametrize("name", list(INDEX_SETS))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_sizes_and_nodes_against_the_full_layers(cfg, name):
    idx = INDEX_SETS[name]
    uniq = sorted(set(idx))
    o = opening(cfg, idx)
    k, m = pkg.lmcs_witness_size(o)
    assert (k, m) == (len(uniq), distinct_ancestors(uniq, DEPTH))
    if name == "all_leaves":
        assert m == 15 and o["commitments"].shape[0] == 0
    w = pkg.lmcs_witness(o, cfg)
    assert w.nodes.shape == (m, 4)
    assert (w.nodes[-1] == o["root"]).all() and (w.root() == o["root"]).all()
    layers = checker(cfg, idx, want_lde=True)["layers"]
    assert (layers[-1] == o["root"]).all()
    for q, i in enumerate(uniq):
        assert (w.leaf_digests[q] == layer(layers, 0)[i]).all()
        for l in range(DEPTH):
            assert (w.path(i)[l] == layer(layers, l)[(i >> l) ^ 1]).all()
    at, level = 0, uniq
    for l in range(1, DEPTH + 1):  # plan order: level by level, ascending position
        level = sorted({x >> 1 for x in level})
        for pos in level:
            assert (w.nodes[at] == layer(layers, l)[pos]).all(), (l, pos)
            at += 1
    assert at == m
    assert pkg.lmcs_witness(o, cfg, nodes=False).nodes is None  # nodes = NULL


@pytest.mark.parametrize("cfg", CONFIGS)
def test_depth_zero_and_depth_one(cfg):
    rng = np.random.default_rng(3)
    align = ALIGN[cfg]
    one = rng.integers(0, A.P, (1, 5), dtype=np.uint64)
    root = pkg.commit_host([one], 0, lmcs=cfg)
    row = np.zeros((5 + align - 1) // align * align, dtype=np.uint64)
    row[:5] = one[0]
    o = dict(root=root, log_height=0, widths=[5], alignment=align, indices=[0], fields=row, commitments=np.zeros((0, 4), dtype=np.uint64))
    assert pkg.lmcs_verify(o, cfg) == (True, "")
    assert pkg.lmcs_witness_size(o) == (1, 0)
    w = pkg.lmcs_witness(o, cfg)
    assert w.paths.shape == (1, 0, 4) and w.nodes.shape == (0, 4)
    assert (w.leaf_digests[0] == root).all() and (w.root() == root).all()
    two = rng.integers(0, A.P, (2, 5), dtype=np.uint64)
    ob.set_lmcs(cfg)
    try:
        both = ob.commit_traces([two], 0, [0, 1], align)
        single = [ob.commit_traces([two], 0, [i], align) for i in (0, 1)]
    finally:
        ob.set_lmcs("poseidon2")
    for idx, r in (([0], single[0]), ([1], single[1]), ([0, 1], both)):
        o = dict(root=r["root"], log_height=1, widths=[5], alignment=align, indices=idx, fields=r["fields"], commitments=r["commitments"])
        assert pkg.lmcs_witness_size(o) == (len(idx), 1)
        w = pkg.lmcs_witness(o, cfg)
        assert (w.nodes[0] == r["root"]).all()
        for i in idx:
            assert (w.path(i) == single[i]["commitments"]).all()
    w = pkg.lmcs_witness(dict(o), cfg)
    assert (w.path(0)[0] == w.leaf_digests[1]).all() and (w.path(1)[0] == w.leaf_digests[0]).all()


# ---- refusals: mh_lmcs_verify's code and reason, and nothing written ------------------------------------------------------------------
def damages(o):
    """the damage classes of tests/test_lmcs_verify.py: name -> (opening, a word of the reason)"""
    f, c, root = o["fields"], o["commitments"], o["root"]
    bad_f = f.copy(); bad_f[7] = (int(bad_f[7]) + 1) % A.P
    bad_c = c.copy(); bad_c[1, 2] = (int(bad_c[1, 2]) + 1) % A.P
    bad_root = root.copy(); bad_root[0] = (int(bad_root[0]) + 1) % A.P
    noncanon = f.copy(); noncanon[3] = A.P
    one = np.ones((1, 4), dtype=np.uint64)
    return {
        "flipped_felt": (dict(o, fields=bad_f), "Merkle root mismatch"),
        "flipped_sibling_word": (dict(o, commitments=bad_c), "Merkle root mismatch"),
        "wrong_root": (dict(o, root=bad_root), "Merkle root mismatch"),
        "one_felt_too_few": (dict(o, fields=f[:-1]), "field stream too short"),
        "one_felt_too_many": (dict(o, fields=np.append(f, np.uint64(0))), "trailing data in the field stream"),
        "one_digest_too_few": (dict(o, commitments=c[:-1]), "commitment stream too short"),
        "one_digest_too_many": (dict(o, commitments=np.concatenate([c, one])), "trailing data in the commitment stream"),
        "non_canonical_felt": (dict(o, fields=noncanon), "non-canonical field element"),
        "index_outside_the_tree": (dict(o, indices=o["indices"] + [1 << DEPTH]), "outside the tree"),
    }


DAMAGES = ["flipped_felt", "flipped_sibling_word", "wrong_root", "one_felt_too_few", "one_felt_too_many", "one_digest_too_few",
           "one_digest_too_many", "non_canonical_felt", "index_outside_the_tree"]


def raw_witness(o, cfg, salt=0, lmcs_id=None):
    """mh_lmcs_witness on sentinel-filled buffers sized for the undamaged opening -> (code, reason, the three buffers)"""
    lib = pkg.load_library()
    item = pkg.LmcsOpening.make(**o)
    bufs = [np.full(n, SENTINEL, dtype=np.uint64) for n in (4 * 16, 4 * 16 * DEPTH, 4 * 31)]
    err = C.create_string_buffer(512)
    lib.mh_lmcs_witness.argtypes = [C.c_int, C.c_int, C.POINTER(pkg.LmcsOpening), C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    rc = lib.mh_lmcs_witness(pkg.Ctx.LMCS[cfg] if lmcs_id is None else lmcs_id, salt, C.byref(item), *[b.ctypes.data for b in bufs], err, 512)
    return rc, err.value.decode(), bufs


@pytest.mark.parametrize("damage", DAMAGES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_damage_gives_the_verifiers_reason_and_writes_nothing(cfg, damage):
    o, word = damages(opening(cfg, INDEX_SETS["duplicated_unsorted"]))[damage]
    ok, why = pkg.lmcs_verify(o, cfg)
    assert not ok and word in why
    rc, reason, bufs = raw_witness(o, cfg)
    assert rc == 1 and reason == why
    assert all((b == SENTINEL).all() for b in bufs)
    with pytest.raises(pkg.MidenHipError, match=word):
        pkg.lmcs_witness(o, cfg)


def test_accepted_opening_fills_exactly_its_arrays():
    o = opening("poseidon2", INDEX_SETS["duplicated_unsorted"])
    rc, reason, bufs = raw_witness(o, "poseidon2")
    assert rc == 0 and reason == ""
    k, m = pkg.lmcs_witness_size(o)
    w = pkg.lmcs_witness(o, "poseidon2")
    for b, a, n in zip(bufs, (w.leaf_digests, w.paths, w.nodes), (4 * k, 4 * k * DEPTH, 4 * m)):
        assert (b[:n] == a.reshape(-1)).all() and (b[n:] == SENTINEL).all()


def test_refuses_bad_configuration_like_the_verifier():
    o = opening("poseidon2", [5])
    lib = pkg.load_library()
    lib.mh_lmcs_verify.argtypes = [C.c_int, C.c_int, C.POINTER(pkg.LmcsOpening), C.c_char_p, C.c_size_t]
    item, err = pkg.LmcsOpening.make(**o), C.create_string_buffer(512)
    for lmcs_id, salt in [(5, 0), (-1, 0), (0, -1), (0, pkg.MH_MAX_SALT_ELEMS + 1), (0, 1)]:
        assert lib.mh_lmcs_verify(lmcs_id, salt, C.byref(item), err, 512) == 1
        rc, reason, bufs = raw_witness(o, "poseidon2", salt, lmcs_id)
        assert rc == 1 and reason == err.value.decode() and all((b == SENTINEL).all() for b in bufs)
    lib.mh_lmcs_witness.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    assert lib.mh_lmcs_witness(0, 0, None, None, None, None, err, 512) == 1 and "null" in err.value.decode()
    buf = np.zeros(4 * DEPTH, dtype=np.uint64)
    assert lib.mh_lmcs_witness(0, 0, C.byref(item), None, buf.ctypes.data, None, err, 512) == 1 and "null output" in err.value.decode()
    assert lib.mh_lmcs_witness(0, 0, C.byref(item), buf.ctypes.data, buf.ctypes.data, None, None, 0) == 0  # no room for a reason is fine


def test_witness_size_refuses_what_the_index_checks_refuse():
    o = opening("poseidon2", [5])
    for change, word in [(dict(indices=[]), "at least one index"), (dict(indices=[5, 16]), "index 1 outside the tree"),
                         (dict(log_height=33), "tree height out of range"), (dict(log_height=-1), "tree height out of range")]:
        bad = dict(o, **change)
        ok, why = pkg.lmcs_verify(bad)
        assert not ok and word in why
        with pytest.raises(pkg.MidenHipError) as e:
            pkg.lmcs_witness_size(bad)
        assert str(e.value) == why
    # shape only: the streams are not read
    assert pkg.lmcs_witness_size(dict(o, indices=[9, 2, 9, 15, 2, 3], fields=o["fields"][:1])) == (4, distinct_ancestors([2, 3, 9, 15], DEPTH))
    lib = pkg.load_library()
    lib.mh_lmcs_witness_size.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    err = C.create_string_buffer(64)
    assert lib.mh_lmcs_witness_size(None, None, None, err, 64) == 1 and "null" in err.value.decode()
