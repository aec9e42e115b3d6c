"""GPU (run with -m gpu): the leaf sponges of the commit path on corner operands.  test_gpu_p2_tails.py puts corner rows into the TRACE,
but the leaf kernels (csrc/lmcs.hip k_leaf_absorb*: the P2F_CAPACITY / P2F_ALL / P2F_DIGEST tails, the state carried between height
groups, and the rpo / rpx / keccak / blake3 forms) read the LDE on the shifted coset, where those rows no longer exist.  A constant column
has a constant LDE: a trace whose columns are constants from tests/corner_felts.py puts those constants into every lane of the sponge.
  1. tree.download_lde(i) is that constant everywhere -- an NTT case of its own, a coefficient vector of one felt and zeros;
  2. tree.download_layers() and the root equal ob.lmcs_build over LDE matrices written directly in numpy (the oracle's LDE is not
     involved): the oracle's sponge and compression are the only reference.
A tree of constant columns has ONE distinct leaf state, so many tiny trees are the point: every vector at log_n = 1 under both blowups,
four of them at log_n = 3 as well."""
import numpy as np
import pytest
import oracle_binding as ob
import corner_felts as cf
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
SEED = [0x0123456789ABCDEF, 0xFFFFFFFF00000005, 7, 0xFEDCBA9876543210]
SPONGE_WIDTHS = [1, 7, 8, 9, 16, 17, 25]           # around the rate of 8: one DIGEST step .. three CAPACITY steps and a padded chunk
WIDTHS = {"poseidon2": SPONGE_WIDTHS, "rpo": SPONGE_WIDTHS, "rpx": SPONGE_WIDTHS,
          "blake3": [1, 4, 5, 12, 13],             # 32 + 8 w bytes: the 64-byte block boundaries
          "keccak": [16, 17, 18, 34, 35]}          # rate 17
N_VECTORS = {"poseidon2": 16, "rpo": 4, "rpx": 4, "blake3": 4, "keccak": 4}
THREE_GROUPS = [(2, 5), (4, 11), (4, 8)]           # (rows, width): the carried state is written, re-read, and read lifted by the short group


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    ob.set_lmcs("poseidon2")
    c.close()


def vectors(hasher, width):
    """poseidon2: each corner in every position, then mixtures (16; the 8 of the table at width 1).  The others: the two heaviest
    corners everywhere and two mixtures."""
    vs = cf.corner_vectors(width, 16)
    if hasher == "poseidon2":
        return vs
    return [vs[k] for k in ((2, 3, 8, 9) if len(vs) > 9 else (2, 3, 4, 6))]


def check_constant_tree(ctx, hasher, shapes, vecs, lb, salt=0):
    """shapes: [(rows, width)] ascending, vecs: one constant vector per matrix.  Caller has set the hasher on ctx and on the oracle."""
    pkg = load_package()
    what = (hasher, shapes, f"lb={lb}", f"salt={salt}", [[hex(int(x)) for x in v] for v in vecs])
    traces = [cf.constant_rows(rows, v) for (rows, _), v in zip(shapes, vecs)]
    tree = pkg.commit_traces(ctx, [ctx.upload_trace(t) for t in traces], lb).tree()
    try:
        direct = [cf.constant_rows(rows << lb, v) for (rows, _), v in zip(shapes, vecs)]
        for i, d in enumerate(direct):
            got = tree.download_lde(i)
            assert got.shape == d.shape and (got == d).all(), ("LDE", i) + what
        mats = direct + ([tree.salt()] if salt else [])
        root, layers = ob.lmcs_build(mats, want_layers=True)
        got = tree.download_layers()
        assert got.shape == layers.shape and (got == layers).all(), ("layers", int(np.nonzero((got != layers).any(axis=1))[0][0])) + what
        assert (tree.root() == root).all(), ("root",) + what
    finally:
        tree.free()


@pytest.mark.parametrize("hasher,width", [(h, w) for h in WIDTHS for w in WIDTHS[h]])
def test_constant_corner_columns(ctx, hasher, width):
    vs = vectors(hasher, width)
    assert len(vs) >= min(N_VECTORS[hasher], len(cf.CORNERS))
    ctx.set_salt(0)
    ctx.set_lmcs(hasher)
    ob.set_lmcs(hasher)
    try:
        for lb in (1, 3):
            for v in vs:
                check_constant_tree(ctx, hasher, [(2, width)], [v], lb)
            for v in [vs[k] for k in (2, 3, len(vs) - 2, len(vs) - 1)]:
                check_constant_tree(ctx, hasher, [(8, width)], [v], lb)
    finally:
        ctx.set_lmcs("poseidon2")
        ob.set_lmcs("poseidon2")


def group_vectors(k):
    """the k-th choice of one vector per matrix of THREE_GROUPS"""
    return [cf.corner_vectors(w, 16, seed=i)[k if w > 1 else k % len(cf.CORNERS)] for i, (_, w) in enumerate(THREE_GROUPS)]


@pytest.mark.parametrize("hasher", list(WIDTHS))
def test_three_height_groups(ctx, hasher):
    ctx.set_salt(0)
    ctx.set_lmcs(hasher)
    ob.set_lmcs(hasher)
    try:
        for lb in (1, 3):
            for k in (range(16) if hasher == "poseidon2" else (2, 3, 9, 12)):
                check_constant_tree(ctx, hasher, THREE_GROUPS, group_vectors(k), lb)
    finally:
        ctx.set_lmcs("poseidon2")
        ob.set_lmcs("poseidon2")


@pytest.mark.parametrize("hasher", ["poseidon2", "blake3"])
def test_three_height_groups_salted(ctx, hasher):
    """the hiding LMCS: four salt felts per leaf, absorbed after the last matrix -- appended to the oracle's matrices as downloaded"""
    ctx.set_lmcs(hasher)
    ob.set_lmcs(hasher)
    try:
        ctx.set_salt(4, SEED)
        for lb in (1, 3):
            for k in (range(16) if hasher == "poseidon2" else (2, 3, 9, 12)):
                check_constant_tree(ctx, hasher, THREE_GROUPS, group_vectors(k), lb, salt=4)
    finally:
        ctx.set_salt(0)
        ctx.set_lmcs("poseidon2")
        ob.set_lmcs("poseidon2")
