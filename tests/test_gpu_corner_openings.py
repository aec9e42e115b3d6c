"""GPU (run with -m gpu): the verifier's leaf and node hashers (csrc/verify_batch.hip k_vfy_leaves<H>, k_vfy_paths<H>, k_vfy_witness<H>)
on hand-made openings over corner rows.  So far they were compared with the library's own host code only, and only on openings of random
trees.  An opening is caller data: the trees here are built by the CPU oracle (ob.lmcs_build, no LDE in between) over matrices whose
rows are the patterns of tests/corner_felts.py, and the openings are put together by hand from those matrices and the oracle's layers
(corner_felts.hand_opening, held to the oracle's own openings in tests/test_corner_felts.py).
  * lmcs_verify_batch accepts every opening;
  * lmcs_witness_batch returns leaf digests, paths and nodes equal to the oracle's layers at those positions;
  * the host calls lmcs_verify / lmcs_witness say the same (an additional assertion, not the yardstick);
  * a field raised by 1 is rejected by both, a felt >= p refused by both (the host names the reason).
Index sets: all leaves (no sibling streamed; 1024 leaves go through the strided loops), one leaf, and 65 seeded distinct leaves -- or
all but three where the tree has fewer than 68."""
import numpy as np
import pytest
import oracle_binding as ob
import corner_felts as cf
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
P = ob.P
HASHERS = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
ALIGN = {"poseidon2": 8, "blake3": 1, "keccak": 17, "rpo": 8, "rpx": 8}
SHAPES = {"one": [(8, 9)], "lifted": [(16, 9), (32, 17)], "strided": [(1024, 17)]}
ROW_PATTERNS = [1, 2, 5]      # of corner_felts.digest_patterns: the heaviest corner everywhere, a mixture, a quarter of the rows random
_TREES = {}


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    try:
        yield c
    finally:
        c.set_lmcs("poseidon2")
        c.set_salt(0)
        ob.set_lmcs("poseidon2")
        c.close()


def oracle_tree(hasher, shape, k):
    """(pattern name, matrices, root, layers) -- built once, never changed"""
    key = (hasher, shape, k)
    if key not in _TREES:
        pats = [cf.digest_patterns(rows, width, seed=7 * i + rows)[k] for i, (rows, width) in enumerate(SHAPES[shape])]
        mats = [m for _, m in pats]
        ob.set_lmcs(hasher)
        try:
            root, layers = ob.lmcs_build(mats, want_layers=True)
        finally:
            ob.set_lmcs("poseidon2")
        for a in mats + [root, layers]:
            a.setflags(write=False)
        _TREES[key] = (pats[0][0], mats, root, layers)
    return _TREES[key]


def index_sets(height, seed):
    rng = np.random.default_rng(seed)
    some = [int(i) for i in rng.permutation(height)[:min(65, height - 3)]]
    return {"all": list(range(height)), "one": [int(rng.integers(0, height))], "some": some}


def openings_of(hasher, shape):
    out = []
    for k in ROW_PATTERNS:
        name, mats, root, layers = oracle_tree(hasher, shape, k)
        for which, idx in index_sets(mats[-1].shape[0], 100 + k).items():
            out.append(((hasher, shape, name, which), layers, cf.hand_opening(mats, root, layers, idx, ALIGN[hasher])))
    return out


def check_witness(what, w, o, layers):
    uniq = sorted(set(o["indices"]))
    depth = o["log_height"]
    assert list(w.indices) == uniq, what
    assert w.leaf_digests.shape == (len(uniq), 4) and w.paths.shape == (len(uniq), depth, 4), what
    lv = [cf.layer(layers, l) for l in range(depth + 1)]
    assert (w.leaf_digests == lv[0][uniq]).all(), ("leaf digests",) + what
    for l in range(depth):
        sib = [(i >> l) ^ 1 for i in uniq]
        assert (w.paths[:, l] == lv[l][sib]).all(), ("paths", l) + what
    exp, level = [], uniq
    for l in range(1, depth + 1):          # every derived parent, level by level, ascending position
        level = sorted({x >> 1 for x in level})
        exp.append(lv[l][level])
    exp = np.concatenate(exp)
    assert w.nodes.shape == exp.shape and (w.nodes == exp).all(), ("nodes",) + what
    assert (w.root() == o["root"]).all(), what


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hasher", HASHERS)
def test_corner_openings(ctx, hasher, shape):
    pkg = load_package()
    items = openings_of(hasher, shape)
    ops = [o for _, _, o in items]
    assert pkg.lmcs_verify_batch(ctx, ops, hasher) == [1] * len(ops), [w for w, _, _ in items]
    ws = pkg.lmcs_witness_batch(ctx, ops, hasher)
    for (what, layers, o), w in zip(items, ws):
        assert w is not None, what
        check_witness(("device",) + what, w, o, layers)
        ok, why = pkg.lmcs_verify(o, hasher)
        assert ok and why == "", what + (why,)
        hw = pkg.lmcs_witness(o, hasher)
        check_witness(("host",) + what, hw, o, layers)


@pytest.mark.parametrize("hasher", HASHERS)
def test_damaged_corner_openings(ctx, hasher):
    """next to the intact opening in one batch: one field raised by 1 (still canonical) -> root mismatch; one felt >= p -> refused before
    anything is hashed"""
    pkg = load_package()
    what, layers, good = [x for x in openings_of(hasher, "lifted") if x[0][3] == "some"][1]
    raised = dict(good, fields=good["fields"].copy())
    at = next(i for i, v in enumerate(raised["fields"]) if int(v) < P - 1)
    raised["fields"][at] += np.uint64(1)
    assert int(raised["fields"][at]) < P
    noncanon = dict(good, fields=good["fields"].copy())
    noncanon["fields"][3] = np.uint64(P)
    batch = [good, raised, noncanon, good]
    assert pkg.lmcs_verify_batch(ctx, batch, hasher) == [1, 0, 0, 1], what
    ws = pkg.lmcs_witness_batch(ctx, batch, hasher)
    assert ws[0] is not None and ws[1] is None and ws[2] is None and ws[3] is not None, what
    check_witness(("device",) + what, ws[3], good, layers)
    for bad, word in ((raised, "Merkle root mismatch"), (noncanon, "non-canonical field element")):
        ok, why = pkg.lmcs_verify(bad, hasher)
        assert not ok and why.startswith("opening rejected: ") and word in why, what + (why,)
        with pytest.raises(pkg.MidenHipError, match=word):
            pkg.lmcs_witness(bad, hasher)
