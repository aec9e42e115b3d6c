"""Corner operands for the kernels behind the LDE (Merkle compressions, leaf sponges, the verifier's hashers, OOD / DEEP sums).  A helper
module, not a test; tests/test_corner_felts.py holds it -- and the references the GPU tests build from it -- to their word on the CPU.

`CORNERS` is the one canonical table: the union of tests/test_gpu_p2_tails.py's CORNERS and tests/jit_corner_operands.py's CORNER_FELTS,
plus 0xFFFFFFFEFFFFFFFF (canonical, both 32-bit halves at or next to 2^32 - 1; it is p - 2, which both sources already hold under
other spellings: eight distinct entries).  The lazy half sums of this code base go wrong at carries
that uniform data meets with probability ~2^-32, so a test that wants them executed picks its operands from here.

The pattern generators return uint64 arrays of a given shape; `digest_patterns` names the four kinds the Merkle tests run.  Everything is
seeded: the same arrays in every process.

`merkle_levels` is the yardstick of the compression tests: a Poseidon2 Merkle tree level by level, every level one batched oracle
permutation of the rows [left, right, 0, 0, 0, 0], lanes 0..3 kept.  `coset_major` / `node_slot` restate the device's leaf-side layout.

`deep_accumulators` restates, over Python integers, the six 64-bit accumulators of the DEEP quotient's column loop (csrc/deep.hip
k_deep_assemble, csrc/pcs_open.hip k_deep_assemble_n).  Like jit_corner_operands.mul_model it is used ONLY TO DESCRIBE INPUTS -- how close
to the documented 2^61 a chosen case comes -- never for an expected value."""
import numpy as np

P = 0xFFFFFFFF00000001
HEAVY = 0xFFFFFFFEFFFFFFFF   # = p - 2: canonical; halves 0xFFFFFFFE | 0xFFFFFFFF
CORNERS = np.array([0, 1, P - 1, HEAVY, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFE00000001, 0x7FFFFFFF80000000], dtype=np.uint64)
DEEP_FLUSH = 128             # csrc/deep.hip, csrc/pcs_open.hip: columns between two reductions of the accumulators


# ---- patterns -----------------------------------------------------------------------------------------------------------------------
def same(shape, corner):
    """every element the same corner"""
    return np.full(shape, corner, dtype=np.uint64)


def mixture(shape, seed):
    """a seeded mixture of corners"""
    rng = np.random.default_rng(seed)
    return CORNERS[rng.integers(0, len(CORNERS), shape)]


def left_equals_right(shape, seed):
    """rows 2i and 2i + 1 equal (a seeded mixture): both children of every first-level node are the same digest"""
    assert shape[0] % 2 == 0
    half = mixture((shape[0] // 2,) + tuple(shape[1:]), seed)
    return np.repeat(half, 2, axis=0)


def quarter_random(shape, seed):
    """a seeded mixture with every fourth row uniformly random below p: the control"""
    rng = np.random.default_rng(seed)
    out = mixture(shape, seed + 1)
    rows = np.arange(0, shape[0], 4)
    out[rows] = rng.integers(0, P, (rows.size,) + tuple(shape[1:]), dtype=np.uint64)
    return out


def digest_patterns(n_rows, width=4, seed=0):
    """[(name, uint64[n_rows, width])]: one of each kind, plus the heaviest corner everywhere and a second mixture -- six patterns"""
    shape = (n_rows, width)
    out = [("same:p-1", same(shape, P - 1)), (f"same:{HEAVY:#x}", same(shape, HEAVY)), (f"mix:{seed}", mixture(shape, 1000 + seed)),
           (f"mix:{seed + 1}", mixture(shape, 1001 + seed)), ("left=right", left_equals_right(shape, 2000 + seed)),
           ("quarter-random", quarter_random(shape, 3000 + seed))]
    return out


def corner_vectors(width, count, seed=0):
    """`count` distinct vectors of `width` corners: each corner in every position first, then seeded mixtures.  Width 1 has only
    len(CORNERS) vectors to give; then all of them are returned."""
    out = [tuple(int(c) for _ in range(width)) for c in CORNERS]
    rng = np.random.default_rng(7000 + 31 * width + seed)
    tries = 0
    while len(out) < count and tries < 64 * count:
        v = tuple(int(x) for x in CORNERS[rng.integers(0, len(CORNERS), width)])
        tries += 1
        if v not in out:
            out.append(v)
    return [np.array(v, dtype=np.uint64) for v in out[:max(count, 0)]]


def constant_rows(rows, vec):
    """a matrix whose column c is the constant vec[c]"""
    return np.tile(np.asarray(vec, dtype=np.uint64), (rows, 1))


# ---- Merkle trees over caller-supplied digests -----------------------------------------------------------------------------------------
def merkle_levels(leaves, permute):
    """[leaf level, ..., root level] of the Poseidon2 tree over leaves[n][4] (n a power of two, natural order): every level is ONE call of
    permute(states[k][12]) on the rows [left, right, 0, 0, 0, 0]; a node = lanes 0..3 of its row."""
    cur = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
    assert cur.shape[0] & (cur.shape[0] - 1) == 0
    levels = [cur]
    while cur.shape[0] > 1:
        st = np.zeros((cur.shape[0] // 2, 12), dtype=np.uint64)
        st[:, :8] = cur.reshape(-1, 8)
        cur = np.ascontiguousarray(permute(st)[:, :4])
        levels.append(cur)
    return levels


def merkle_levels_by_node(leaves, compress):
    """the same shape of result with compress(left[4], right[4]) -> [4] called node by node (any hasher)"""
    cur = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
    levels = [cur]
    while cur.shape[0] > 1:
        cur = np.array([compress(cur[2 * i], cur[2 * i + 1]) for i in range(cur.shape[0] // 2)], dtype=np.uint64).reshape(-1, 4)
        levels.append(cur)
    return levels


def node_slot(log_height, log_blowup, d, p):
    """csrc/kernels.hpp mh_tree::node_slot: where node p (natural position) of depth d lies in its layer.  The leaf-side layers are
    coset-major: with B = 2^cbits cosets left at depth d, p = r * B + j lies at j * (2^d / B) + r."""
    cbits = d - (log_height - log_blowup)
    if cbits <= 0:
        return p
    j, r = p & ((1 << cbits) - 1), p >> cbits
    return (j << (log_height - log_blowup)) + r


def coset_major(natural, log_blowup):
    """the leaf layer as the device stores it: slot j * N + r holds leaf r * B + j of the natural-order tree (B = 2^log_blowup)"""
    nat = np.ascontiguousarray(natural, dtype=np.uint64)
    B = 1 << log_blowup
    N = nat.shape[0] // B
    assert N * B == nat.shape[0]
    return np.ascontiguousarray(nat.reshape(N, B, -1).transpose(1, 0, 2).reshape(nat.shape[0], -1))


def device_order_root(buf, log_blowup, permute):
    """The root the way the compression kernels index it (csrc/lmcs.hip k_compress*): while the child layer still has coset bits, output q
    = j' * N + r takes its children from slots (2 j') * N + r and (2 j' + 1) * N + r; above that, from 2 q and 2 q + 1."""
    cur = np.ascontiguousarray(buf, dtype=np.uint64).reshape(-1, 4)
    log_height = cur.shape[0].bit_length() - 1
    log_n = log_height - log_blowup
    for d in range(log_height - 1, -1, -1):
        q = np.arange(1 << d)
        if (d + 1) - log_n > 0:
            left = ((2 * (q >> log_n)) << log_n) + (q & ((1 << log_n) - 1))
            right = left + (1 << log_n)
        else:
            left, right = 2 * q, 2 * q + 1
        st = np.zeros((1 << d, 12), dtype=np.uint64)
        st[:, :4], st[:, 4:8] = cur[left], cur[right]
        cur = np.ascontiguousarray(permute(st)[:, :4])
    return cur[0]


# ---- hand-made LMCS openings ---------------------------------------------------------------------------------------------------------------
def layer(layers, l):
    """level l above the leaves of the oracle's layer array (leaves first, 2 H - 1 digests)"""
    height = (layers.shape[0] + 1) // 2
    off = 2 * height - ((2 * height) >> l)
    return layers[off:off + (height >> l)]


def missing_siblings(idx, depth):
    """[(level above the leaves, position)] of the digests an opening streams: per level, bottom-up and left to right, the sibling of every
    opened node whose sibling is not opened itself -- the walk tests/test_lmcs_verify.py's expected_siblings counts."""
    level, out = sorted(set(int(i) for i in idx)), []
    for l in range(depth):
        s = set(level)
        out += [(l, x ^ 1) for x in level if (x ^ 1) not in s]
        level = sorted({x >> 1 for x in level})
    return out


def bitrev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def hand_opening(mats, root, layers, idx, alignment):
    """The dict lmcs_verify / lmcs_verify_batch take, made by hand from the matrices of an oracle tree (bit-reversed rows, ascending
    heights): per sorted unique index every matrix's row padded with zeros to `alignment`, then the missing siblings out of `layers`."""
    H = mats[-1].shape[0]
    depth = H.bit_length() - 1
    fields = []
    for i in sorted(set(int(x) for x in idx)):
        br = bitrev(i, depth)
        for m in mats:
            row = m[br >> (depth - (m.shape[0].bit_length() - 1))]
            fields += [int(v) for v in row] + [0] * (-len(row) % alignment)
    sib = [layer(layers, l)[pos] for l, pos in missing_siblings(idx, depth)]
    commitments = np.array(sib, dtype=np.uint64).reshape(-1, 4)
    return dict(root=np.array(root, dtype=np.uint64), log_height=depth, widths=[m.shape[1] for m in mats], alignment=alignment,
                indices=[int(x) for x in idx], fields=np.array(fields, dtype=np.uint64), commitments=commitments)


# ---- the DEEP quotient's delayed reduction, as a description of inputs ---------------------------------------------------------------------
def deep_accumulators(negc, values, flush=DEEP_FLUSH):
    """negc: one base-field component of the per-column coefficients, values: the column values one lane reads (both lists of ints < 2^64,
    one entry per column in loop order).  Returns (sum mod p the way the kernel reduces it, the largest value any of the six accumulators
    holds between two flushes).  Three 22-bit limbs of negc times the two 32-bit halves of v, summed by weight
    2^0, 2^22, 2^44 (x v.lo) and 2^32, 2^54, 2^76 (x v.hi); a reduction after every `flush` columns and at the end."""
    weights = [1, 1 << 22, 1 << 44, 1 << 32, 1 << 54, 1 << 76]
    w, total, peak, pending = [0] * 6, 0, 0, 0
    for cf, v in zip(negc, values):
        al = [(cf >> (22 * i)) & 0x3FFFFF for i in range(3)]
        v0, v1 = v & 0xFFFFFFFF, v >> 32
        for i in range(3):
            w[i] += al[i] * v0
            w[3 + i] += al[i] * v1
        peak = max(peak, max(w))
        pending += 1
        if pending == flush:
            total = (total + sum(a * c for a, c in zip(w, weights))) % P
            w, pending = [0] * 6, 0
    total = (total + sum(a * c for a, c in zip(w, weights))) % P
    return total, peak
