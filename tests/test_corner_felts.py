"""CPU: the inputs and the yardsticks of the corner-operand GPU tests behind the LDE (tests/test_gpu_corner_merkle.py,
test_gpu_corner_leaves.py, test_gpu_corner_openings.py, test_gpu_corner_deep.py) are what those tests take them for.
  * tests/corner_felts.py's table is canonical and is the union it claims to be; its patterns have the shape they claim.
  * The batched level-by-level Merkle tree (one oracle permutation call per level) is the oracle's compression node by node, and the
    oracle's own lmcs_build root and layers.
  * The device's leaf-side layout: a buffer filled coset-major (slot j * N + r = leaf r * B + j) and compressed with the kernels' index
    formulas gives the root of the natural-order tree.
  * A constant column has a constant LDE (the oracle's coset LDE).
  * The hand-made openings are the oracle's own openings.
  * A Python-integer model of the DEEP quotient's six accumulators says how close the chosen case comes to the documented bound.

What the DEEP cases cannot reach through the API, for the record: the per-column coefficients are the powers of ONE alpha, so the limbs
of all columns cannot be chosen freely -- alpha = (1, 0) makes every coefficient -1 = (p - 1, 0), whose 22-bit limbs are 0, 0x3FFC00,
0xFFFFF: the low-limb accumulators and the whole c1 component stay zero while the middle-limb ones run at 0.9998 of the bound.  And the
bound the kernel documents (128 products below 2^54 stay below 2^61) is a factor of 8 below the real overflow of a 64-bit accumulator: a
kernel that flushed every 1024 columns would still pass these inputs; one that flushed every 1025 could fail only on columns this heavy."""
import numpy as np
import pytest
import oracle_binding as ob
import corner_felts as cf
import jit_corner_operands as jc

P = ob.P


def test_table_is_canonical_and_the_union():
    import test_gpu_p2_tails as tails
    table = [int(x) for x in cf.CORNERS]
    assert all(0 <= x < P for x in table) and len(set(table)) == len(table)
    assert set(table) == {int(x) for x in tails.CORNERS} | set(jc.CORNER_FELTS) | {0xFFFFFFFEFFFFFFFF}
    assert cf.HEAVY == P - 2 and cf.HEAVY & 0xFFFFFFFF == 0xFFFFFFFF and cf.HEAVY >> 32 == 0xFFFFFFFE


def test_patterns():
    pats = dict(cf.digest_patterns(64))
    assert len(pats) >= 4
    table = set(int(x) for x in cf.CORNERS)
    for name, a in pats.items():
        assert a.shape == (64, 4) and a.dtype == np.uint64 and (a < np.uint64(P)).all(), name
    assert (pats["same:p-1"] == np.uint64(P - 1)).all()
    assert (pats["left=right"][0::2] == pats["left=right"][1::2]).all()
    assert all(int(x) in table for name in ("mix:0", "mix:1", "left=right") for x in pats[name].reshape(-1))
    q = pats["quarter-random"]
    assert all(int(x) in table for k in (1, 2, 3) for x in q[k::4].reshape(-1))
    assert sum(int(x) not in table for x in q[0::4].reshape(-1)) > 48     # the control rows are not corners
    again = dict(cf.digest_patterns(64))
    assert all((pats[k] == again[k]).all() for k in pats)                 # seeded
    for width in (1, 7, 25):
        vs = cf.corner_vectors(width, 16)
        assert len(vs) == (16 if width > 1 else len(cf.CORNERS)) and len({tuple(v.tolist()) for v in vs}) == len(vs)
        assert all(v.shape == (width,) and all(int(x) in table for x in v) for v in vs)
        assert all((vs[k] == cf.CORNERS[k]).all() for k in range(len(cf.CORNERS)))   # each corner in every position comes first


def test_batched_tree_is_the_oracles_compression():
    for name, leaves in cf.digest_patterns(32):
        got = cf.merkle_levels(leaves, ob.permute)
        exp = cf.merkle_levels_by_node(leaves, ob.compress)
        assert len(got) == len(exp) == 6
        for g, e in zip(got, exp):
            assert g.shape == e.shape and (g == e).all(), name
        ob.set_lmcs("poseidon2")
        by_lmcs = cf.merkle_levels_by_node(leaves, ob.lmcs_compress)
        assert (by_lmcs[-1] == got[-1]).all()


def test_batched_tree_is_lmcs_build():
    rng = np.random.default_rng(3)
    m = rng.integers(0, P, (16, 5), dtype=np.uint64)
    root, layers = ob.lmcs_build([m], want_layers=True)
    levels = cf.merkle_levels(cf.layer(layers, 0), ob.permute)
    assert (levels[-1][0] == root).all()
    assert (np.concatenate(levels) == layers).all()
    # the leaves themselves: digest i = the sponge over row bitrev(i)
    for i in (0, 5, 15):
        assert (cf.layer(layers, 0)[i] == ob.sponge_absorb(np.zeros(12, dtype=np.uint64), m[cf.bitrev(i, 4)])[:4]).all()


@pytest.mark.parametrize("hasher", ["blake3", "keccak", "rpo", "rpx"])
def test_node_by_node_tree_is_lmcs_build_under_the_other_hashers(hasher):
    rng = np.random.default_rng(4)
    m = rng.integers(0, P, (8, 3), dtype=np.uint64)
    ob.set_lmcs(hasher)
    try:
        root, layers = ob.lmcs_build([m], want_layers=True)
        levels = cf.merkle_levels_by_node(cf.layer(layers, 0), ob.lmcs_compress)
    finally:
        ob.set_lmcs("poseidon2")
    assert (np.concatenate(levels) == layers).all() and (levels[-1][0] == root).all()


@pytest.mark.parametrize("log_height,lb", [(1, 0), (3, 0), (3, 2), (6, 3), (7, 3), (5, 5)])
def test_coset_major_slots(log_height, lb):
    """leaf r * B + j is taken from slot j * N + r, and the kernels' two index phases walk that layout to the natural-order root"""
    n, B = 1 << log_height, 1 << lb
    N = n // B
    nat = cf.mixture((n, 4), 50 + log_height)
    nat[:, 0] = np.arange(n, dtype=np.uint64)                      # every leaf distinct: a misplaced one changes the root
    buf = cf.coset_major(nat, lb)
    for r in range(N):
        for j in range(B):
            assert (buf[j * N + r] == nat[r * B + j]).all()
            assert cf.node_slot(log_height, lb, log_height, r * B + j) == j * N + r
    for d in range(log_height + 1):                                # a permutation of every layer; the identity above the coset phase
        slots = [cf.node_slot(log_height, lb, d, p) for p in range(1 << d)]
        assert sorted(slots) == list(range(1 << d))
        if d <= log_height - lb:
            assert slots == list(range(1 << d))
    root = cf.merkle_levels(nat, ob.permute)[-1][0]
    assert (cf.device_order_root(buf, lb, ob.permute) == root).all()
    if lb and log_height > lb:                                     # and the layout matters: the natural buffer read coset-major is another tree
        assert (cf.device_order_root(nat, lb, ob.permute) != root).any()


@pytest.mark.parametrize("log_n,lb", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_constant_column_has_a_constant_lde(log_n, lb):
    vec = cf.corner_vectors(9, 16)[11]
    traces = [cf.constant_rows(1 << log_n, vec), cf.constant_rows(2 << log_n, vec[:5])]
    r = ob.commit_traces(traces, lb, want_lde=True)
    for t, lde in zip(traces, r["ldes"]):
        assert lde.shape == (t.shape[0] << lb, t.shape[1]) and (lde == t[0][None, :]).all()
    # so the tree over LDE matrices written directly is the commitment
    direct = [cf.constant_rows(t.shape[0] << lb, t[0]) for t in traces]
    assert (ob.lmcs_build(direct) == r["root"]).all()


@pytest.mark.parametrize("hasher,align", [("poseidon2", 8), ("blake3", 1), ("keccak", 17)])
def test_hand_made_openings_are_the_oracles(hasher, align):
    """constant matrices, so that commit_traces (which extends its input) commits exactly the matrices lmcs_build is given"""
    lb = 1
    traces = [cf.constant_rows(4, cf.corner_vectors(9, 16)[12]), cf.constant_rows(8, cf.corner_vectors(17, 16)[13])]
    mats = [cf.constant_rows(t.shape[0] << lb, t[0]) for t in traces]
    ob.set_lmcs(hasher)
    try:
        root, layers = ob.lmcs_build(mats, want_layers=True)
        for idx in ([5], [6, 7], [9, 2, 9, 15, 2, 3], list(range(16))):
            exp = ob.commit_traces(traces, lb, sorted(set(idx)), align)
            o = cf.hand_opening(mats, root, layers, idx, align)
            assert (exp["root"] == root).all()
            assert o["fields"].shape == exp["fields"].shape and (o["fields"] == exp["fields"]).all()
            assert o["commitments"].shape == exp["commitments"].shape and (o["commitments"] == exp["commitments"]).all()
    finally:
        ob.set_lmcs("poseidon2")


def test_hand_made_opening_reads_bit_reversed_rows():
    """with distinct rows: the opened row of index i is physical row bitrev(i), the short matrix read at bitrev(i) >> 1"""
    rng = np.random.default_rng(9)
    mats = [cf.mixture((8, 9), 1), cf.mixture((16, 17), 2)]
    mats[0][:, 0], mats[1][:, 0] = np.arange(8, dtype=np.uint64), np.arange(16, dtype=np.uint64)
    root, layers = ob.lmcs_build(mats, want_layers=True)
    o = cf.hand_opening(mats, root, layers, [int(rng.integers(0, 16))], 8)
    i = o["indices"][0]
    assert int(o["fields"][0]) == cf.bitrev(i, 4) >> 1 and int(o["fields"][16]) == cf.bitrev(i, 4)
    assert o["fields"].size == 16 + 24 and o["commitments"].shape == (4, 4)
    lvl = [cf.layer(layers, l) for l in range(5)]
    assert [x.shape[0] for x in lvl] == [16, 8, 4, 2, 1] and (lvl[4][0] == root).all()
    assert all((o["commitments"][l] == lvl[l][(i >> l) ^ 1]).all() for l in range(4))


def test_deep_accumulator_model():
    """alpha = (1, 0): every coefficient is -1 = (p - 1, 0).  128 columns of 0xFFFFFFFEFFFFFFFF bring the middle-limb accumulator of the
    low half to 128 * 0x3FFC00 * 0xFFFFFFFF between two flushes: at least 0.9997 * 2^61 and below 2^61."""
    limbs = [((P - 1) >> (22 * i)) & 0x3FFFFF for i in range(3)]
    assert limbs == [0, 0x3FFC00, 0xFFFFF] and sum(l << (22 * i) for i, l in enumerate(limbs)) == P - 1
    v = cf.HEAVY
    total, peak = cf.deep_accumulators([P - 1] * 128, [v] * 128)
    assert peak == 128 * 0x3FFC00 * 0xFFFFFFFF
    assert 9997 * (1 << 61) <= 10000 * peak and peak < 1 << 61
    assert total == (P - 1) * v * 128 % P
    # one column more: the flush has happened, the peak is the same, the sum is still the sum
    for n in (129, 136, 257):
        t, pk = cf.deep_accumulators([P - 1] * n, [v] * n)
        assert pk == peak and t == (P - 1) * v * n % P
    # a kernel that forgot the flush would pass 2^61 at column 129 and still not wrap: the real overflow is 8 times further
    _, unflushed = cf.deep_accumulators([P - 1] * 257, [v] * 257, flush=1 << 30)
    assert 1 << 61 < unflushed < 1 << 64 and 8 * peak < 1 << 64 <= 9 * peak
    # the model is the plain sum on anything (it describes the kernel's arithmetic, it is not the yardstick)
    rng = np.random.default_rng(1)
    c = [int(x) for x in rng.integers(0, P, 300, dtype=np.uint64)]
    x = [int(x) for x in rng.integers(0, P, 300, dtype=np.uint64)]
    t, pk = cf.deep_accumulators(c, x)
    assert t == sum(a * b for a, b in zip(c, x)) % P and pk < 1 << 61
    # the c1 component of -alpha^k is zero for alpha = (1, 0): its six accumulators stay empty
    assert cf.deep_accumulators([0] * 128, [v] * 128) == (0, 0)
