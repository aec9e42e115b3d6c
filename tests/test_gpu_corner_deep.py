"""GPU (run with -m gpu): out-of-domain evaluation and the DEEP quotient's delayed-reduction dot product on corner columns -- a sibling of
tests/test_gpu_pcs_open.py, whose Python-integer helpers it imports.  The dot product exists twice (csrc/deep.hip k_deep_assemble, the
hot two-point kernel, and csrc/pcs_open.hip k_deep_assemble_n): 22-bit by 32-bit limb products summed in six plain 64-bit accumulators
and reduced once per 128 columns, "128 products of < 2^54 stay below 2^61".  Random columns average a quarter of that.  A constant column
has a constant LDE, so a committed matrix of constant corner columns puts chosen felts into every lane of k_ood_partial*, k_deep_assemble
and k_deep_assemble_n; with alpha = (1, 0) every coefficient is -1 = (p - 1, 0), and 128 columns of 0xFFFFFFFEFFFFFFFF bring the largest
accumulator to 128 * 0x3FFC00 * 0xFFFFFFFF = 0.9998 * 2^61 right before the flush (tests/test_corner_felts.py, the model and what it
cannot reach).  References, all over Python integers:
  * evaluations: the constant (zero padding included) for a constant column, Horner of the interpolant for a random one;
  * the DEEP layer: sum_j beta^j (f_red(z_j) - f_red(x_i)) / (z_j - x_i) at every point of the LDE domain, from the downloaded LDEs;
  * the session's two-point kernel: felt-for-felt parity with the standalone opening of the session's own trees, whose DEEP layer is
    held to the same definition."""
import ctypes as C
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
import corner_felts as cf
from test_gpu_pcs_open import P, TOY, eadd, esub, emul, einv, epow2, root_of_unity, interpolate, horner, aligned_row, bitrev
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
LB = 3
HEAVY = cf.HEAVY


def flush_vec(w):
    """the first 256 columns the heaviest corner; beyond that other corners"""
    return [HEAVY] * min(w, 256) + [int(cf.CORNERS[(2 + k) % len(cf.CORNERS)]) for k in range(max(0, w - 256))]


# one tree per shape: (rows, width, constants or None = random), ascending heights
SHAPES = {f"flush{w}": [(4, w, flush_vec(w)), (4, 3, None)] for w in (128, 129, 136, 257)}   # log_N = 2 = DEEP_ONE_COSET_MIN_LOG_N: planes
SHAPES["lifted"] = [(2, 17, [int(x) for x in cf.corner_vectors(17, 16)[10]]), (8, 3, None)]   # the constants are read through nm_mask
SHAPES["tiny"] = [(2, 9, [int(x) for x in cf.corner_vectors(9, 16)[11]]), (2, 2, None)]       # log_N = 1: the all-cosets form
ALPHAS = [(1, 0), (P - 1, 0), (0, 1), (0, P - 1), (0xFFFFFFFF, 0xFFFFFFFF00000000), None]     # None: one seeded random
BETAS = [(1, 0), (P - 1, P - 1), None]
_CASES = {}


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


def case(name):
    """(matrices, log_N, points: four seeded valid ones and a base-field one, ref[j][0][matrix][col], random alpha, random beta)"""
    if name in _CASES:
        return _CASES[name]
    pkg = load_package()
    rng = np.random.default_rng(sum(map(ord, name)))
    ef = lambda: (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))  # noqa: E731
    mats = [cf.constant_rows(r, v) if v is not None else rng.integers(0, P, (r, w), dtype=np.uint64) for r, w, v in SHAPES[name]]
    log_N = max(m.shape[0] for m in mats).bit_length() - 1
    points = []
    while len(points) < 4:
        z = ef()
        if pkg.pcs_point_ok(log_N, LB, z):
            points.append(z)
    base = (int(rng.integers(0, P, dtype=np.uint64)), 0)
    while not pkg.pcs_point_ok(log_N, LB, base):
        base = (int(rng.integers(0, P, dtype=np.uint64)), 0)
    points.append(base)
    ref = []
    for z in points:
        per_mat = []
        for m, (_, _, v) in zip(mats, SHAPES[name]):
            if v is not None:
                per_mat.append([(int(c), 0) for c in v])
            else:
                y = epow2(z, log_N - (m.shape[0].bit_length() - 1))
                per_mat.append([horner(interpolate(m[:, c]), y) for c in range(m.shape[1])])
        ref.append([per_mat])
    _CASES[name] = (mats, log_N, points, ref, ef(), ef())
    return _CASES[name]


def reduced(values, alpha):
    acc = (0, 0)
    for v in values:
        acc = eadd(emul(acc, alpha), tuple(v) if isinstance(v, (tuple, list)) else (int(v), 0))
    return acc


def reduced_rows(ldes, alpha, L):
    """f_red(x_i) for every natural index i: Horner in alpha over every matrix's row, zero-padded to 8; a short matrix is read at
    i mod its height (rows are stored bit-reversed)"""
    out = []
    for i in range(1 << L):
        vals = []
        for lde in ldes:
            bits = lde.shape[0].bit_length() - 1
            row = lde[bitrev(i % lde.shape[0], bits)]
            vals += [int(v) for v in row] + [0] * (-len(row) % 8)
        out.append(reduced(vals, alpha))
    return out


def deep_definition(fred_z, fred_x, points, beta, L):
    g, wK = pow(7, 1 << (32 - L), P), root_of_unity(L)
    bpow = [(1, 0)]
    for _ in range(len(points) - 1):
        bpow.append(emul(bpow[-1], beta))
    out, x = [], g
    for i in range(1 << L):
        q = (0, 0)
        for j, z in enumerate(points):
            q = eadd(q, emul(emul(bpow[j], esub(fred_z[j], fred_x[i])), einv(esub(z, (x, 0)))))
        out.append(q)
        x = x * wK % P
    return out


def run_shape(ctx, name):
    pkg = load_package()
    mats, log_N, points, ref, rnd_alpha, rnd_beta = case(name)
    L = log_N + LB
    ctx.set_lmcs("poseidon2")
    ctx.set_salt(0)
    tree = pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in mats], LB).tree()
    ldes = [tree.download_lde(k) for k in range(len(mats))]
    for lde, (_, _, v) in zip(ldes, SHAPES[name]):
        if v is not None:
            assert (lde == np.array(v, dtype=np.uint64)[None, :]).all(), (name, "the LDE of a constant column is the constant")
    alphas = [a if a is not None else rnd_alpha for a in ALPHAS]
    betas = [b if b is not None else rnd_beta for b in BETAS]
    s0, s1, s2, s3, base = points
    index = {z: j for j, z in enumerate(points)}
    runs = [(alphas[0], [s0, base, s1, s2][:n], b) for n in (1, 2, 3, 4) for b in betas]
    runs += [(a, [s3, base, s1], b) for a in alphas[1:] for b in betas]
    fred_x = {}
    for alpha, pts, beta in runs:
        what = (name, "alpha", alpha, "beta", beta, "N", len(pts))
        op = pkg.PcsOpening(ctx, [tree], pts, dict(TOY, log_blowup=LB))
        rows = [aligned_row(ref[index[z]], 8) for z in pts]
        got = op.evals()
        for j in range(len(pts)):
            assert got[j].tolist() == rows[j], ("evaluations", j) + what
        op.deep(alpha, beta)
        layer = op.download_deep()
        if alpha not in fred_x:
            fred_x[alpha] = reduced_rows(ldes, alpha, L)
        exp = deep_definition([reduced(r, alpha) for r in rows], fred_x[alpha], pts, beta, L)
        assert layer.shape == (1 << L, 2)
        for i in range(1 << L):
            assert (int(layer[i][0]), int(layer[i][1])) == exp[i], ("DEEP layer", i) + what
        op.free()
    tree.free()


@pytest.mark.parametrize("name", list(SHAPES))
def test_corner_columns(ctx, name):
    run_shape(ctx, name)


def test_corner_columns_all_cosets_env(ctx, monkeypatch):
    """the same 129 columns through the all-cosets form of the assemble kernel (the variable is read at each call)"""
    monkeypatch.setenv("MH_DEEP_ALL_COSETS", "1")
    run_shape(ctx, "flush129")


# ---- the two-point kernel of the STARK session ----------------------------------------------------------------------------------------
def download_raw_lde(ctx, handle, rows, width):
    """mh_tree_download_lde of a borrowed tree handle (Session.trees()): matrix 0, [rows, width], physical row order"""
    buf = np.zeros(4 * rows * width + 4096, dtype=np.uint64)   # room to spare: a shape other than the expected one shows below
    ctx.check(ctx.lib.mh_tree_download_lde(ctx.h, handle, 0, buf.ctypes.data_as(C.POINTER(C.c_uint64))))
    assert not buf[rows * width:].any(), "the matrix is larger than [rows, width]"
    return buf[:rows * width].reshape(rows, width).copy()


def evaluate_from_lde(lde, L, z):
    """the column polynomials at z from their values on the coset g K (natural order = physical row bitrev(i)): interpolate u(w_K^i) =
    f(g w_K^i), then f(z) = u(z / g)"""
    g_inv = pow(pow(7, 1 << (32 - L), P), P - 2, P)
    y = emul(z, (g_inv, 0))
    nat = [bitrev(i, L) for i in range(1 << L)]
    return [horner(interpolate([int(lde[r][c]) for r in nat]), y) for c in range(lde.shape[1])]


def session_on_corner_trace(ctx, air, vec, log_n, beta, seed):
    pkg = load_package()
    ctx.set_lmcs("poseidon2")
    ctx.set_salt(0)
    rng = np.random.default_rng(seed)
    ef = lambda: (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))  # noqa: E731
    n, width = 1 << log_n, len(vec)
    trace = cf.constant_rows(n, vec)
    aux = rng.integers(0, P, (n, 4), dtype=np.uint64)
    aux_vals = [int(x) for x in rng.integers(0, P, 4, dtype=np.uint64)]
    dev_air = pkg.DeviceAir(ctx, air)
    s = pkg.Session(ctx, [dev_air], [ctx.upload_trace(trace)], [], TOY)
    sh = s.shape
    s.commit_main()
    s.commit_aux([ef() for _ in range(sh.num_randomness)], lambda i, rnd: (aux, aux_vals))
    s.commit_quotient(ef(), ef())
    z = ef()
    while not s.ood_point_ok(z):
        z = ef()
    w = root_of_unity(log_n)
    pts = [z, (z[0] * w % P, z[1] * w % P)]
    ev_s = s.ood(z)
    trees = s.trees()
    assert len(trees) == 3
    op = pkg.PcsOpening(ctx, trees, pts, TOY)
    L = sh.log_lde_height
    assert L == log_n + LB and op.shape.ood_width == sh.ood_width
    evals = op.evals()
    assert (evals.reshape(-1) == ev_s).all()
    alpha = (1, 0)
    what = (getattr(air, "name", "air"), "beta", beta)
    s.deep(alpha, beta)
    op.deep(alpha, beta)
    layer = op.download_deep()
    for _ in range(sh.num_fri_rounds):
        assert (s.fri_commit() == op.fri_commit()).all(), what
        fb = ef()
        s.fri_fold(fb)
        op.fri_fold(fb)
    assert (s.fri_final() == op.fri_final()).all(), what
    idx = [int(i) for i in rng.integers(0, 1 << L, TOY["num_queries"])]
    hs, ho = s.open(idx), op.query(idx)
    assert hs.fields.size and (hs.fields == ho.fields).all() and hs.commitments.shape == ho.commitments.shape, what
    assert (hs.commitments == ho.commitments).all(), what
    # the standalone layer of the session's own trees against the definition: main (constant), aux, quotient chunks (2 D columns)
    q_width = 2 << ctx.lib.mh_air_log_quotient_degree(dev_air.h)
    assert sh.ood_width == -(-width // 8) * 8 + 8 + -(-q_width // 8) * 8
    ldes = [download_raw_lde(ctx, t, n << LB, wd) for t, wd in zip(trees, (width, 4, q_width))]
    assert (ldes[0] == trace[0][None, :]).all(), "the LDE of a constant column is the constant"
    rows = []
    for j, zj in enumerate(pts):
        per_mat = [[(int(c), 0) for c in vec]] + [evaluate_from_lde(lde, L, zj) for lde in ldes[1:]]
        rows.append(aligned_row([[m] for m in per_mat], 8))
        assert evals[j].tolist() == rows[j], ("evaluations", j) + what
    exp = deep_definition([reduced(r, alpha) for r in rows], reduced_rows(ldes, alpha, L), pts, beta, L)
    for i in range(1 << L):
        assert (int(layer[i][0]), int(layer[i][1])) == exp[i], ("DEEP layer", i) + what
    op.free()
    s.free()


@pytest.mark.parametrize("b", range(len(BETAS)))
def test_session_parity_on_corner_trace(ctx, b):
    """the existing 12-column AIR of test_gpu_pcs_open.session_vs_standalone on a trace of constant corner columns"""
    beta = BETAS[b] or (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    air = A.synthetic_big_air(width=12, aux_width=2, n_constraints=10, seed=3)
    session_on_corner_trace(ctx, air, [int(x) for x in cf.corner_vectors(12, 16)[9 + b]], 4, beta, 60 + b)


@pytest.mark.parametrize("b", range(len(BETAS)))
def test_session_parity_across_the_flush(ctx, b):
    """136 main columns of 0xFFFFFFFEFFFFFFFF on 4 rows: k_deep_assemble's accumulators reach their largest value at column 128"""
    from miden_vm_amd import dag
    beta = BETAS[b] or (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    session_on_corner_trace(ctx, dag.dummy_miden_air(136, 2), [HEAVY] * 136, 2, beta, 70 + b)
