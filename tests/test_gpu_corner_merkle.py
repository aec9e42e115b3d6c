"""GPU (run with -m gpu): every Merkle compression form on corner digests.  The leaf digests of a real commitment are sponge outputs --
uniform-looking whatever the trace held -- so the three device forms of the Poseidon2 compression (csrc/lmcs.hip k_compress,
k_compress_quad = poseidon2_quad.cuh, k_compress_lanes = poseidon2_lanes.cuh) and the other hashers' node kernels have only ever seen
random operands.  mh_shard_build_subtree compresses CALLER-SUPPLIED leaf digests with lmcs_compress_layers, the function every commit
uses: here the caller supplies the patterns of tests/corner_felts.py, and the root must equal the CPU oracle's tree over the same
leaves (Poseidon2: level by level with batched oracle permutations; the others: orc_lmcs_compress node by node), bit for bit.

Only the FIRST compressed level sees the chosen operands (the levels above see digests), and lmcs_compress_layers picks the form by the
size of the level, so each form gets a tree of its own -- by the thresholds in lmcs_compress_layers (n = nodes of the first level):
    n = 65536          > 32768: k_compress                     n = 32768, 16384   in [16384, 32768]: k_compress_quad
    n = 8192           <= 8192: k_compress_lanes               n = 64             k_compress_lanes; with lb = 0 the levels above it are
    n = 4, n = 1       k_compress_lanes down to the root, 16-lane groups beyond n idle (they recompute node 0)      the host's top
Each size runs with lb = 0 (natural indexing, children 2q and 2q + 1, from the first level on) and with coset indexing in the first
levels (children j' * 2N + r and + N): lb = 3, or the largest the tree allows where a trace of two rows leaves fewer coset bits.
The buffer is coset-major (mh_tree::node_slot): slot j * N + r is leaf r * B + j of the natural-order tree."""
import ctypes as C
import numpy as np
import pytest
import torch
import oracle_binding as ob
import corner_felts as cf
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
P2_CASES = [(17, 0), (17, 3), (16, 0), (16, 3), (15, 0), (15, 3), (14, 0), (14, 3), (7, 0), (7, 3), (3, 0), (3, 2), (1, 0)]
P2_PARAMS = [(ll, lb, k) for ll, lb in P2_CASES for k in range(6)]   # six patterns per case: corner_felts.digest_patterns
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    ob.set_lmcs("poseidon2")
    c.close()


def pattern(log_leaves, k):
    return cf.digest_patterns(1 << log_leaves, seed=log_leaves)[k]


def reference_root(hasher, log_leaves, k):
    """computed once per (hasher, size, pattern): lb = 0 and lb > 0 are the same natural-order tree"""
    key = (hasher, log_leaves, k)
    if key not in _REF:
        name, leaves = pattern(log_leaves, k)
        if hasher == "poseidon2":
            root = cf.merkle_levels(leaves, ob.permute)[-1][0]
        else:
            ob.set_lmcs(hasher)
            try:
                root = cf.merkle_levels_by_node(leaves, ob.lmcs_compress)[-1][0]
            finally:
                ob.set_lmcs("poseidon2")
        root.setflags(write=False)
        _REF[key] = root
    return _REF[key]


def device_root(ctx, log_leaves, lb, leaves):
    """zero trace -> shard of one rank (its leaf layer is only a size here) -> subtree over OUR digests"""
    lib = ctx.lib
    lib.mh_shard_free.argtypes = [C.c_void_p]
    log_n = log_leaves - lb
    assert log_n >= 1
    trace = ctx.upload_trace(np.zeros((1 << log_n, 1), dtype=np.uint64))
    arr = (C.c_void_p * 1)(trace.h)
    h = C.c_void_p()
    ctx.check(lib.mh_shard_commit_leaves(ctx.h, 1, arr, lb, 0, 1, C.byref(h)))
    try:
        buf = cf.coset_major(leaves, lb)
        dev = torch.from_numpy(buf.view(np.int64)).to("cuda")
        assert dev.numel() == 4 << log_leaves
        torch.cuda.synchronize()
        root = np.zeros(4, dtype=np.uint64)
        ctx.check(lib.mh_shard_build_subtree(ctx.h, h, C.c_void_p(dev.data_ptr()), root.ctypes.data_as(C.POINTER(C.c_uint64))))
        return root
    finally:
        lib.mh_shard_free(h)
        trace.free()


@pytest.mark.parametrize("log_leaves,lb,k", P2_PARAMS)
def test_poseidon2_forms(ctx, log_leaves, lb, k):
    name, leaves = pattern(log_leaves, k)
    ctx.set_lmcs("poseidon2")
    ctx.set_salt(0)
    got = device_root(ctx, log_leaves, lb, leaves)
    exp = reference_root("poseidon2", log_leaves, k)
    assert (got == exp).all(), (f"2^{log_leaves} leaves", f"lb={lb}", name, [hex(int(x)) for x in got], [hex(int(x)) for x in exp])


@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("lb", [0, 3])
@pytest.mark.parametrize("hasher", ["rpo", "rpx", "keccak", "blake3"])
def test_other_hashers(ctx, hasher, lb, k):
    """2^10 leaves: k_compress_alg (rpo, rpx), k_compress_kk, k_compress_b3 and from 256 nodes on the one-launch k_compress_b3_top.  The
    digests of the byte hashers are four arbitrary words; the corner felts are as good as any."""
    name, leaves = pattern(10, k)
    ctx.set_salt(0)
    try:
        ctx.set_lmcs(hasher)
        got = device_root(ctx, 10, lb, leaves)
    finally:
        ctx.set_lmcs("poseidon2")
    exp = reference_root(hasher, 10, k)
    assert (got == exp).all(), (hasher, f"lb={lb}", name, [hex(int(x)) for x in got], [hex(int(x)) for x in exp])
