"""GPU tests (run with -m gpu) of the Poseidon2 permutation with its round constants as product addends and with tails sized to the
caller (poseidon2_fast.cuh: p2f_body + p2f_tail<ALL | DIGEST | CAPACITY>), bit-exact against the CPU oracle:
  * the permutation itself (all twelve outputs): the addends of all eight S-box layers and of the de-scale products;
  * leaf hashing at the widths where the sponge changes shape: one DIGEST step, an exact rate boundary, a zero-padded last chunk,
    1..6 CAPACITY steps in front of the DIGEST step;
  * state carried between height groups (the ALL tail writes the canonical carried-state buffer), salted and not;
  * a level of 2^16 nodes through k_compress (DIGEST);
  * one small proof byte for byte (FRI leaves: CAPACITY between chunks, DIGEST at the end; everything else)."""
import numpy as np
import pytest
import oracle_binding as ob
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
P = ob.P
CORNERS = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 0x7FFFFFFF80000000], dtype=np.uint64)
SEED = [0x0123456789ABCDEF, 0xFFFFFFFF00000005, 7, 0xFEDCBA9876543210]


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def rnd(rng, shape):
    return rng.integers(0, P, shape, dtype=np.uint64)


def test_permutation_on_corner_states(ctx):
    rng = np.random.default_rng(31)
    n = 24000
    s = CORNERS[rng.integers(0, len(CORNERS), (n, 12))]
    s[0] = 0
    s[1] = P - 1
    s[2] = np.uint64(0xFFFFFFFFFFFFFFFF)  # non-canonical input: the permutation of its residue
    s[3:9, :] = CORNERS[3:9, None]         # one corner in all twelve elements
    s[20000:] = rnd(rng, (n - 20000, 12))
    exp_in = s.copy()
    exp_in[2] = np.uint64(0xFFFFFFFFFFFFFFFF - P)
    got = ctx.poseidon2_permute(s)
    exp = ob.permute(exp_in)
    assert (got < np.uint64(P)).all(), "outputs are canonical"
    assert (got == exp).all(), int(np.nonzero((got != exp).any(axis=1))[0][0])


def check_tree(ctx, shapes, lb, seed, corner_rows=False):
    pkg = load_package()
    rng = np.random.default_rng(seed)
    traces = [rnd(rng, (1 << lh, w)) for lh, w in shapes]
    if corner_rows:
        for t in traces:
            t[: min(4, t.shape[0])] = CORNERS[rng.integers(0, len(CORNERS), t[:4].shape)]
    exp = ob.commit_traces(traces, lb, want_lde=True)
    com = pkg.commit_traces(ctx, [ctx.upload_trace(t) for t in traces], lb)
    tree = com.tree()
    for i in range(len(traces)):
        assert (tree.download_lde(i) == exp["ldes"][i]).all(), f"LDE {i}"
    return tree, com, exp


@pytest.mark.parametrize("width", [1, 7, 8, 9, 16, 17, 51])
def test_leaf_hashing_widths(ctx, width):
    tree, com, exp = check_tree(ctx, [(3, width)], 3, 50 + width, corner_rows=True)
    root, layers = ob.lmcs_build(exp["ldes"], want_layers=True)
    got = tree.download_layers()
    assert got.shape == layers.shape and (got == layers).all(), int(np.nonzero((got != layers).any(axis=1))[0][0])
    assert (com.root() == root).all() and (com.root() == exp["root"]).all()
    tree.free()


@pytest.mark.parametrize("salt", [0, 4])
def test_carried_state(ctx, salt):
    """Three height groups: the first two launches write the carried state (all twelve elements, canonical), the last the digests."""
    ctx.set_salt(salt, SEED) if salt else ctx.set_salt(0)
    try:
        tree, com, exp = check_tree(ctx, [(3, 5), (5, 11), (5, 8)], 3, 77)
        mats = exp["ldes"] + ([tree.salt()] if salt else [])
        root, layers = ob.lmcs_build(mats, want_layers=True)
        assert (tree.download_layers() == layers).all()
        assert (com.root() == root).all()
        tree.free()
    finally:
        ctx.set_salt(0)


def test_compression_level(ctx):
    """2^17 leaves: the level of 2^16 nodes is k_compress (a state per lane, the DIGEST tail)."""
    tree, com, exp = check_tree(ctx, [(14, 3)], 3, 91)
    root, layers = ob.lmcs_build(exp["ldes"], want_layers=True)
    got = tree.download_layers()
    assert (got == layers).all(), int(np.nonzero((got != layers).any(axis=1))[0][0])
    assert (com.root() == root).all()
    tree.free()


def test_small_proof_is_byte_equal(ctx):
    pkg = load_package()
    from miden_vm_amd import dag, protocol
    air = dag.dummy_miden_air(11, 2)
    rng = np.random.default_rng(0)
    trace = rnd(rng, (64, 11))
    trace[:, 0] = 0
    params = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=2, deep_pow_bits=3, num_queries=6,
                  query_pow_bits=4)
    st, pre = protocol.challenger_state(), protocol.protocol_pre_observe(params, [])
    got = pkg.prove(ctx, [pkg.DeviceAir(ctx, air)], [ctx.upload_trace(trace)], [], params, st, pre, None)
    exp = ob.prove([air], [trace], [], params)
    assert got.fields.size == exp["fields"].size and (got.fields == exp["fields"]).all()
    assert (got.commitments == exp["commitments"]).all() and (got.digest == exp["digest"]).all()
    ok, msg = ob.verify([air], got.log_trace_heights, [], {"fields": got.fields, "commitments": got.commitments}, params)
    assert ok, msg
