"""GPU (run with -m gpu): the polynomial commitment scheme on its own -- mh_pcs_* (include/midenhip.h): committed LMCS trees opened at
N = 1..4 out-of-domain points by the point-count-generic kernels of csrc/pcs_open.hip.  The CPU checker has no N-point PCS, so the
references are stated per test: plain polynomial arithmetic in Python integers (1, 3), the STARK session (2), the host verifier (4).
  1. evaluations == interpolate every column over H, evaluate at z_j^L by Horner in the quadratic extension (exact, padding included)
  2. N = 2 at (z, z * w_N) on a session's own trees == the session, felt for felt (evaluations, FRI roots, final polynomial, hints)
  3. the DEEP layer == sum_j beta^j (f_red(z_j) - f_red(x_i)) / (z_j - x_i) from the downloaded LDEs
  4. pcs_open -> pcs_verify round trip, N = 1..4 x five hashers, salted once, tampering refused
  5. refusals: MH_ERR_INVALID + a message on the host, the context stays usable
  6. examples/pcs_c_abi.c builds and runs"""
import os, subprocess
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
ROOT_2_32 = 1753635133440165772
HASHES = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
ALIGN = {"poseidon2": 8, "blake3": 1, "keccak": 17, "rpo": 8, "rpx": 8}
SEED = [0x0123456789ABCDEF, 0xFFFFFFFF00000005, 7, 0xFEDCBA9876543210]
TOY = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5, query_pow_bits=3)
# trees -> matrices (rows, width), ascending heights inside a tree; log_blowup
SHAPES = {
    "tiny": ([[(2, 1)]], 3),
    "one": ([[(32, 3)]], 3),
    "mixed": ([[(16, 2), (64, 3)]], 3),                 # mixed heights in one tree: the reference's case 3
    "two_trees": ([[(16, 9)], [(64, 17)]], 3),          # the short TREE is lifted in the query phase
    "chunks": ([[(1 << 14, 2)]], 1),                    # more than one OOD_ROWS_PER_BLOCK chunk
    "wide": ([[(16, 130)]], 3),                         # aligned width beyond DEEP_FLUSH
}


# ---- Goldilocks and its quadratic extension (x^2 = 7) in Python integers ----
def eadd(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def esub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def emul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def einv(a):
    n = pow((a[0] * a[0] - 7 * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, (P - a[1]) * n % P)


def epow2(a, k):
    for _ in range(k):
        a = emul(a, a)
    return a


def root_of_unity(log_n):
    return pow(ROOT_2_32, 1 << (32 - log_n), P)


def interpolate(vals):
    """Coefficients of the polynomial of degree < n through vals on H = <w_n> (natural order): an inverse radix-2 DFT."""
    n = len(vals)
    log_n = n.bit_length() - 1

    def fft(a, w):
        if len(a) == 1:
            return a
        e, o = fft(a[0::2], w * w % P), fft(a[1::2], w * w % P)
        half, out, x = len(a) // 2, [0] * len(a), 1
        for k in range(half):
            t = x * o[k] % P
            out[k], out[k + half] = (e[k] + t) % P, (e[k] - t) % P
            x = x * w % P
        return out

    n_inv = pow(n, P - 2, P)
    return [v * n_inv % P for v in fft([int(v) for v in vals], pow(root_of_unity(log_n), P - 2, P))]


def horner(coef, y):
    acc = (0, 0)
    for c in reversed(coef):
        acc = emul(acc, y)
        acc = ((acc[0] + c) % P, acc[1])
    return acc


_CASES = {}


def case(name):
    """(matrices per tree, log_blowup, log_N, four seeded points, reference evaluations ref[j][tree][matrix][col]) -- computed once."""
    if name in _CASES:
        return _CASES[name]
    pkg = load_package()
    shape, lb = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    mats = [[rng.integers(0, P, s, dtype=np.uint64) for s in tree] for tree in shape]
    log_N = max(int(h).bit_length() - 1 for tree in shape for h, _ in tree)
    points = []
    while len(points) < 4:
        z = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
        if pkg.pcs_point_ok(log_N, lb, z):
            points.append(z)
    coefs = [[[interpolate(m[:, c]) for c in range(m.shape[1])] for m in tree] for tree in mats]
    ref = []
    for z in points:
        ref.append([[[horner(col, epow2(z, log_N - (m.shape[0].bit_length() - 1))) for col in cm] for m, cm in zip(tree, ct)]
                    for tree, ct in zip(mats, coefs)])
    _CASES[name] = (mats, lb, log_N, points, ref)
    return _CASES[name]


def aligned_row(ref_j, align):
    """One point's evaluations in transcript order: all trees, all matrices, each zero-padded to the alignment."""
    row = []
    for tree in ref_j:
        for m in tree:
            row += [list(v) for v in m] + [[0, 0]] * (-len(m) % align)
    return row


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    ob.set_lmcs("poseidon2")
    c.close()


def commit(ctx, name, lmcs="poseidon2"):
    pkg = load_package()
    ctx.set_lmcs(lmcs)
    ctx.set_salt(0)
    mats, lb, *_ = case(name)
    return [pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in tree], lb).tree() for tree in mats]


def params_for(name):
    return dict(TOY, log_blowup=SHAPES[name][1])


# ---- 1. evaluations against plain polynomial arithmetic -----------------------------------------------------------------------
EVAL_CASES = [(s, "poseidon2") for s in SHAPES] + [("mixed", "blake3"), ("mixed", "keccak")]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("name,lmcs", EVAL_CASES)
def test_evaluations(ctx, name, lmcs, n):
    pkg = load_package()
    mats, lb, log_N, points, ref = case(name)
    trees = commit(ctx, name, lmcs)
    op = pkg.PcsOpening(ctx, trees, points[:n], params_for(name))
    align = ALIGN[lmcs]
    assert op.shape.n_points == n and op.shape.log_lde_height == log_N + lb
    assert op.shape.ood_width == sum(-(-m.shape[1] // align) * align for tree in mats for m in tree)
    got = op.evals()
    for j in range(n):
        assert got[j].tolist() == aligned_row(ref[j], align), (name, lmcs, n, j)
    op.free()


def test_duplicate_points(ctx):
    """Duplicate points are legal and need no special case: the same evaluations twice, and a DEEP layer that verifies."""
    pkg = load_package()
    _, _, _, points, ref = case("mixed")
    trees = commit(ctx, "mixed")
    pts = [points[0], points[1], points[0]]
    op = pkg.PcsOpening(ctx, trees, pts, TOY)
    got = op.evals()
    assert got[0].tolist() == got[2].tolist() == aligned_row(ref[0], 8) and got[1].tolist() == aligned_row(ref[1], 8)
    op.free()
    roots = [t.root() for t in trees]
    pre = [int(x) for r in roots for x in r]
    proof = pkg.pcs_open(ctx, trees, pts, TOY, ob.challenger_state(), pre)
    ok, digest, _ = pkg.pcs_verify(roots, [6], [[2, 3]], pts, TOY, ob.challenger_state(), pre, proof.fields, proof.commitments)
    assert ok and (digest == proof.digest).all(), digest


# ---- 2. N = 2 on the STARK's own points equals the session ---------------------------------------------------------------------
def session_vs_standalone(ctx, log_n):
    pkg = load_package()
    ctx.set_lmcs("poseidon2")
    ctx.set_salt(0)
    rng = np.random.default_rng(40 + log_n)
    ef = lambda: (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))  # noqa: E731
    air = A.synthetic_big_air(width=12, aux_width=2, n_constraints=10, seed=3)
    trace = A.dummy_trace(log_n, 12, seed=log_n)
    aux = rng.integers(0, P, (1 << log_n, 4), dtype=np.uint64)   # a committed aux matrix that is not zero
    aux_vals = [int(x) for x in rng.integers(0, P, 4, dtype=np.uint64)]
    s = pkg.Session(ctx, [pkg.DeviceAir(ctx, air)], [ctx.upload_trace(trace)], [], TOY)
    sh = s.shape
    s.commit_main()
    s.commit_aux([ef() for _ in range(sh.num_randomness)], lambda i, rnd: (aux, aux_vals))
    s.commit_quotient(ef(), ef())
    z = ef()
    while not s.ood_point_ok(z):
        z = ef()
    assert pkg.pcs_point_ok(log_n, TOY["log_blowup"], z)
    w = root_of_unity(log_n)
    ev_s = s.ood(z)
    trees = s.trees()
    assert len(trees) == 3
    op = pkg.PcsOpening(ctx, trees, [z, (z[0] * w % P, z[1] * w % P)], TOY)
    assert (op.shape.log_lde_height, op.shape.ood_width, op.shape.num_fri_rounds, op.shape.final_poly_len) == \
        (sh.log_lde_height, sh.ood_width, sh.num_fri_rounds, sh.final_poly_len)
    assert (op.evals().reshape(-1) == ev_s).all()
    alpha, beta = ef(), ef()
    s.deep(alpha, beta)
    op.deep(alpha, beta)
    for _ in range(sh.num_fri_rounds):
        assert (s.fri_commit() == op.fri_commit()).all()
        fb = ef()
        s.fri_fold(fb)
        op.fri_fold(fb)
    assert (s.fri_final() == op.fri_final()).all()
    idx = [int(i) for i in rng.integers(0, 1 << sh.log_lde_height, TOY["num_queries"])]
    hs, ho = s.open(idx), op.query(idx)
    assert hs.fields.size and (hs.fields == ho.fields).all() and hs.commitments.shape == ho.commitments.shape
    assert (hs.commitments == ho.commitments).all()
    op.free()
    s.free()


@pytest.mark.parametrize("log_n", [2, 6, 10])   # 2 = DEEP_ONE_COSET_MIN_LOG_N: the smallest one-coset size; 10 takes more than one block
def test_session_parity(ctx, log_n):
    session_vs_standalone(ctx, log_n)


def test_session_parity_tiny_all_cosets_form(ctx):
    """log_N = 1: below DEEP_ONE_COSET_MIN_LOG_N, so both sides take the all-cosets form of their assemble kernels."""
    session_vs_standalone(ctx, 1)


def test_session_parity_all_cosets_env(ctx, monkeypatch):
    monkeypatch.setenv("MH_DEEP_ALL_COSETS", "1")
    session_vs_standalone(ctx, 6)


# ---- 3. the DEEP layer against its definition -------------------------------------------------------------------------------------
def bitrev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("name", ["mixed", "two_trees"])
def test_deep_layer(ctx, name, n):
    pkg = load_package()
    mats, lb, log_N, points, ref = case(name)
    trees = commit(ctx, name)
    L = log_N + lb
    rng = np.random.default_rng(77 + n)
    alpha, beta = (tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)) for _ in range(2))
    op = pkg.PcsOpening(ctx, trees, points[:n], TOY)
    assert op.evals()[0].tolist() == aligned_row(ref[0], 8)
    op.deep(alpha, beta)
    got = op.download_deep()
    # f_red(z_j): Horner over the aligned evaluations; f_red(x_i): the same over the opened rows, a lifted matrix read at i mod its height
    fred_z = []
    for j in range(n):
        acc = (0, 0)
        for v in aligned_row(ref[j], 8):
            acc = eadd(emul(acc, alpha), tuple(v))
        fred_z.append(acc)
    ldes = [[t.download_lde(k) for k in range(len(tree))] for t, tree in zip(trees, mats)]
    g, wK = pow(7, 1 << (32 - L), P), root_of_unity(L)
    bpow = [(1, 0)]
    for _ in range(n - 1):
        bpow.append(emul(bpow[-1], beta))
    x = g
    for i in range(1 << L):
        acc = (0, 0)
        for tree in ldes:
            for lde in tree:
                bits = lde.shape[0].bit_length() - 1
                row = lde[bitrev(i % lde.shape[0], bits)]
                for v in [int(v) for v in row] + [0] * (-len(row) % 8):
                    acc = emul(acc, alpha)
                    acc = ((acc[0] + v) % P, acc[1])
        q = (0, 0)
        for j in range(n):
            q = eadd(q, emul(emul(bpow[j], esub(fred_z[j], acc)), einv(esub(points[j], (x, 0)))))
        assert (int(got[i][0]), int(got[i][1])) == q, (name, n, i)
        x = x * wK % P
    op.free()


# ---- 4. one-shot round trip ---------------------------------------------------------------------------------------------------------
def shape_args(name):
    mats, lb, log_N, points, ref = case(name)
    heights = [max(m.shape[0] for m in tree).bit_length() - 1 for tree in mats]
    widths = [[m.shape[1] for m in tree] for tree in mats]
    return heights, widths


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("lmcs", HASHES)
def test_round_trip(ctx, lmcs, n):
    pkg = load_package()
    _, _, _, points, ref = case("two_trees")
    trees = commit(ctx, "two_trees", lmcs)
    roots = [t.root() for t in trees]
    pre = [int(x) for r in roots for x in r]   # binding the roots is the caller's job
    st = ob.challenger_state()
    proof = pkg.pcs_open(ctx, trees, points[:n], TOY, st, pre)
    heights, widths = shape_args("two_trees")
    ok, digest, evals = pkg.pcs_verify(roots, heights, widths, points[:n], TOY, st, pre, proof.fields, proof.commitments, lmcs=lmcs)
    assert ok, digest
    assert (digest == proof.digest).all()
    assert proof.log_trace_heights == heights
    for j in range(n):
        assert evals[j].tolist() == aligned_row(ref[j], 1), (lmcs, n, j)
    if n in (1, 3):   # tampering: one evaluation, one point, one root
        f = proof.fields.copy()
        f[0] = (int(f[0]) + 1) % P
        bad_pts = [(points[0][0], (points[0][1] + 1) % P)] + points[1:n]
        bad_roots = [roots[0].copy(), roots[1].copy()]
        bad_roots[1][3] = (int(bad_roots[1][3]) + 1) % P if lmcs not in ("blake3", "keccak") else int(bad_roots[1][3]) ^ 1
        for kw in (dict(fields=f), dict(points=bad_pts), dict(roots=bad_roots)):
            a = dict(roots=roots, points=points[:n], fields=proof.fields)
            a.update(kw)
            ok, msg, _ = pkg.pcs_verify(a["roots"], heights, widths, a["points"], TOY, st, pre, a["fields"], proof.commitments, lmcs=lmcs)
            assert not ok and msg, (lmcs, n, list(kw))


@pytest.mark.parametrize("lmcs", ["poseidon2", "blake3"])
def test_round_trip_salted(ctx, lmcs):
    pkg = load_package()
    mats, lb, _, points, ref = case("two_trees")
    ctx.set_lmcs(lmcs)
    ctx.set_salt(4, SEED)
    try:
        trees = [pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in tree], lb).tree() for tree in mats]
        assert all(t.salt_elems == 4 for t in trees)
        roots = [t.root() for t in trees]
        pre = [int(x) for r in roots for x in r]
        st = ob.challenger_state()
        proof = pkg.pcs_open(ctx, trees, points[:3], TOY, st, pre)
        heights, widths = shape_args("two_trees")
        ok, digest, evals = pkg.pcs_verify(roots, heights, widths, points[:3], TOY, st, pre, proof.fields, proof.commitments, lmcs=lmcs, salt_elems=4)
        assert ok and (digest == proof.digest).all(), digest
        assert evals[2].tolist() == aligned_row(ref[2], 1)
        # read without the salt (or with another width) the same streams are refused
        for salt in (0, 2):
            ok, msg, _ = pkg.pcs_verify(roots, heights, widths, points[:3], TOY, st, pre, proof.fields, proof.commitments, lmcs=lmcs, salt_elems=salt)
            assert not ok and msg
        # an unsalted tree is not opened on a salted context
        ctx.set_salt(0)
        plain = commit(ctx, "two_trees", lmcs)
        ctx.set_salt(4, SEED)
        with pytest.raises(pkg.MidenHipError, match="salt width"):
            pkg.PcsOpening(ctx, plain, points[:1], TOY)
    finally:
        ctx.set_salt(0)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Each is MH_ERR_INVALID (1) with a message, decided on the host before anything is launched; a valid call follows each."""
    pkg = load_package()
    mats, lb, log_N, points, ref = case("two_trees")
    trees = commit(ctx, "two_trees")
    L = log_N + lb

    def still_usable():
        op = pkg.PcsOpening(ctx, trees, points[:1], TOY)
        assert op.evals()[0].tolist() == aligned_row(ref[0], 8)
        op.free()

    def refused(fn, match):
        with pytest.raises(pkg.MidenHipError, match=match) as e:
            fn()
        assert "error 1:" in str(e.value)
        still_usable()

    on_h = (pow(root_of_unity(log_N), 3, P), 0)
    on_gk = (pow(7, 1 << (32 - L), P) * pow(root_of_unity(L), 5, P) % P, 0)
    refused(lambda: pkg.PcsOpening(ctx, trees, [points[0], on_h], TOY), "evaluation point 1")
    refused(lambda: pkg.PcsOpening(ctx, trees, [on_gk], TOY), "evaluation point 0")
    refused(lambda: pkg.PcsOpening(ctx, trees, [(0, 0)], TOY), "evaluation point 0")
    refused(lambda: pkg.PcsOpening(ctx, trees, points + [points[0]], TOY), "n_points")
    refused(lambda: pkg.PcsOpening(ctx, trees, [], TOY), "n_points")
    refused(lambda: pkg.pcs_open(ctx, trees, points + [points[1]], TOY, ob.challenger_state(), []), "n_points")
    # a tree committed under another log_blowup
    other = pkg.commit_traces(ctx, [ctx.upload_trace(mats[0][0])], 2).tree()
    refused(lambda: pkg.PcsOpening(ctx, [other, trees[1]], points[:1], TOY), "log_blowup")
    refused(lambda: pkg.PcsOpening(ctx, trees, points[:1], dict(TOY, log_blowup=2)), "log_blowup")
    # no tree at the maximum height: the maximum IS the tallest of the trees handed over, so the only way to have none there is to hand
    # over none; and a point that is fine for the short tree alone is checked against the domain of the tallest one
    refused(lambda: pkg.PcsOpening(ctx, [], points[:1], TOY), "between 1 and 256 committed trees")
    w64 = (root_of_unity(6), 0)
    assert pkg.pcs_point_ok(4, lb, w64) and not pkg.pcs_point_ok(6, lb, w64)
    pkg.PcsOpening(ctx, trees[:1], [w64], TOY).free()
    refused(lambda: pkg.PcsOpening(ctx, trees, [w64], TOY), "evaluation point 0")
    # a tree committed under another hasher
    ctx.set_lmcs("blake3")
    refused_b3 = None
    try:
        pkg.PcsOpening(ctx, trees, points[:1], TOY)
    except pkg.MidenHipError as e:
        refused_b3 = str(e)
    ctx.set_lmcs("poseidon2")
    assert refused_b3 and "error 1:" in refused_b3 and "LMCS hasher" in refused_b3
    still_usable()
    # staged calls out of order
    op = pkg.PcsOpening(ctx, trees, points[:2], TOY)
    refused(lambda: op.deep((1, 2), (3, 4)), "out of protocol order: deep")
    refused(op.fri_commit, "out of protocol order: fri_commit")
    refused(op.download_deep, "out of protocol order: download_deep")
    op.evals()
    refused(op.evals, "out of protocol order: evals")
    refused(lambda: op.query([1]), "out of protocol order: query")
    op.deep((1, 2), (3, 4))
    refused(lambda: op.fri_fold((5, 6)), "fold before the round's commitment")
    refused(op.fri_final, "FRI rounds not finished")
    for _ in range(op.shape.num_fri_rounds):
        op.fri_commit()
        refused(op.fri_commit, "no FRI round left to commit")
        op.fri_fold((5, 6))
    refused(op.download_deep, "folded away")
    refused(op.fri_commit, "no FRI round left to commit")
    op.fri_final()
    refused(op.fri_final, "out of protocol order: fri_final")
    refused(lambda: op.query([1 << L]), "query index out of range")
    assert op.query([1, 5, 1 << (L - 1)]).fields.size
    refused(lambda: op.query([1]), "out of protocol order: query")
    op.free()
    # a session hands out its trees only once the quotient is committed
    s = pkg.Session(ctx, [pkg.DeviceAir(ctx, A.fib_air())], [ctx.upload_trace(A.fib_trace(4)[0])], A.fib_trace(4)[1], TOY)
    refused(s.trees, "trees")
    s.free()


# ---- 6. the C example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmcs", [0, 1])
def test_c_example(tmp_path, lmcs):
    exe = str(tmp_path / "pcs_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pcs_c_abi.c"),
                           "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    out = subprocess.check_output([exe, str(lmcs)], text=True)
    assert "opened 2 trees at 3 points" in out and "verified:" in out and "tampered evaluation refused: proof rejected" in out, out
