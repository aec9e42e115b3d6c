"""GPU tests of the witness form of the batch verifier (run with -m gpu): k_vfy_witness of csrc/verify_batch.hip through
mh_lmcs_witness_batch, whole proofs through mh_verify_batch_witness and mh_verify_miden_batch_witness, and the C example.

The yardstick for the device is the host call mh_lmcs_witness, array for array (tests/test_lmcs_witness.py holds that one to the CPU
checker), and the prover's own tree: its downloaded layers and its single-index openings."""
import ctypes as C
import os, subprocess, sys
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
import proof_parser as PP
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
pkg = load_package()
P = ob.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
OWN_ALIGN = {"poseidon2": 8, "blake3": 1, "keccak": 17, "rpo": 8, "rpx": 8}
SEED = [0x0123456789ABCDEF, 0xFFFFFFFF00000005, 7, 0xFEDCBA9876543210]
# (rows, width) per matrix, log_blowup: log LDE heights 1 (depth 1), 2, 6 (the shorter matrix is lifted), 10.  Depth 0 (a tree of one leaf) is
# committed on the host (commit_host): the device prover is not asked for a one-row trace anywhere else in the suite.
TREES = {"h1_w1": ([(2, 1)], 0), "h2_w8": ([(2, 8)], 1), "h6_w9_w17": ([(16, 9), (32, 17)], 1), "h10_w17": ([(512, 17)], 1)}
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    ob.set_lmcs("poseidon2")
    c.close()


def commit(ctx, name, seed=3):
    shape, lb = TREES[name]
    rng = np.random.default_rng(seed)
    mats = [rng.integers(0, P, s, dtype=np.uint64) for s in shape]
    return pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in mats], lb).tree()


def index_sets(log_height):
    """the sets of tests/test_gpu_verify_batch.py, and 300 distinct leaves of the depth-10 tree: leaf and parent loops stride past 256 lanes"""
    h = 1 << log_height
    sets = {"one": [h - 1], "two_adjacent": [2, 3] if h >= 4 else [0, 1] if h >= 2 else [0], "two_apart": [0, h - 1], "all": list(range(h))}
    if log_height == 10:
        rng = np.random.default_rng(log_height)
        for n in (65, 130, 300):
            pick = [int(i) for i in rng.choice(h, n, replace=False)]
            sets[f"{n}_leaves"] = pick + pick[:3]  # unsorted, with duplicates
    return sets


def open_tree(tree, indices, alignment):
    f, c = tree.prove_batch(indices, alignment)
    return dict(root=tree.root(), log_height=tree.log_height, widths=list(tree.widths), alignment=alignment, indices=list(indices),
                fields=f, commitments=c)


def same(a, b):
    """two LmcsWitness, array for array"""
    return (a.indices.shape == b.indices.shape and (a.indices == b.indices).all() and a.leaf_digests.shape == b.leaf_digests.shape
            and (a.leaf_digests == b.leaf_digests).all() and a.paths.shape == b.paths.shape and (a.paths == b.paths).all()
            and a.nodes.shape == b.nodes.shape and (a.nodes == b.nodes).all())


def host_witness(o, lmcs, salt):
    try:
        return pkg.lmcs_witness(o, lmcs, salt)
    except pkg.MidenHipError:
        return None


def own_openings(ctx, lmcs, salt, with_layers=False):
    """openings of the trees above made with the configuration's own alignment: (opening, tree name, layers or None)"""
    ctx.set_lmcs(lmcs)
    ctx.set_salt(salt, SEED)
    try:
        out = []
        if salt == 0:  # depth 0: the leaf digest is the root (commit_host knows no salt)
            row = np.zeros(-(-5 // OWN_ALIGN[lmcs]) * OWN_ALIGN[lmcs], dtype=np.uint64)
            row[:5] = np.random.default_rng(4).integers(0, P, 5, dtype=np.uint64)
            root = pkg.commit_host([row[:5].reshape(1, 5)], 0, lmcs=lmcs)
            out.append((dict(root=root, log_height=0, widths=[5], alignment=OWN_ALIGN[lmcs], indices=[0], fields=row,
                             commitments=np.zeros((0, 4), dtype=np.uint64)), "h0_host", np.asarray(root).reshape(1, 4)))
            if with_layers:
                out.append(("singles", "h0_host", {}))
        for name in TREES:
            tree = commit(ctx, name)
            assert tree.salt_elems == salt
            layers = tree.download_layers() if with_layers else None
            for idx in index_sets(tree.log_height).values():
                out.append((open_tree(tree, idx, OWN_ALIGN[lmcs]), name, layers))
            if with_layers:  # the prover's own single-index openings: they stream exactly the path
                out.append(("singles", name, {i: tree.prove_batch([i], OWN_ALIGN[lmcs])[1] for i in {0, (1 << tree.log_height) - 1,
                                                                                                     (1 << tree.log_height) // 3}}))
            tree.free()
        return out
    finally:
        ctx.set_salt(0)
        ctx.set_lmcs("poseidon2")


@pytest.mark.parametrize("salt", [0, 8])
@pytest.mark.parametrize("lmcs", HASHES)
def test_device_witness_equals_the_host_witness(ctx, lmcs, salt):
    ops = [o for o, _, _ in own_openings(ctx, lmcs, salt)]
    got = pkg.lmcs_witness_batch(ctx, ops, lmcs, salt)
    host = [host_witness(o, lmcs, salt) for o in ops]
    assert all(h is not None for h in host)  # the yardstick itself
    for k, (g, h) in enumerate(zip(got, host)):
        assert g is not None and same(g, h), (k, ops[k]["log_height"], len(ops[k]["indices"]))
    depths = {o["log_height"] for o in ops}
    assert ({0, 1, 10} if salt == 0 else {1, 10}) <= depths and max(len(set(o["indices"])) for o in ops) == 1024
    without = pkg.lmcs_witness_batch(ctx, ops[:6], lmcs, salt, nodes=False)  # nodes = NULL
    for g, h in zip(without, host):
        assert g.nodes is None and (g.paths == h.paths).all() and (g.leaf_digests == h.leaf_digests).all()


def layer(layers, l, height):
    off = 2 * height - ((2 * height) >> l)
    return layers[off:off + (height >> l)]


@pytest.mark.parametrize("lmcs", ["poseidon2", "blake3"])
def test_against_the_provers_own_tree(ctx, lmcs):
    made = own_openings(ctx, lmcs, 0, with_layers=True)
    ops = [m for m in made if not isinstance(m[0], str)]
    singles = {name: paths for tag, name, paths in made if isinstance(tag, str)}
    got = pkg.lmcs_witness_batch(ctx, [o for o, _, _ in ops], lmcs, 0)
    for w, (o, name, layers) in zip(got, ops):
        depth, h = o["log_height"], 1 << o["log_height"]
        at, level = 0, [int(i) for i in w.indices]
        for q, i in enumerate(level):
            assert (w.leaf_digests[q] == layer(layers, 0, h)[i]).all()
            for l in range(depth):
                assert (w.path(i)[l] == layer(layers, l, h)[(i >> l) ^ 1]).all(), (name, i, l)
            if i in singles[name]:
                assert (w.path(i) == singles[name][i]).all()  # tree.prove_batch([i]) streams exactly path(i)
        for l in range(1, depth + 1):
            level = sorted({x >> 1 for x in level})
            for pos in level:
                assert (w.nodes[at] == layer(layers, l, h)[pos]).all(), (name, l, pos)
                at += 1
        assert at == w.nodes.shape[0]


def damaged(o):
    """the damage classes of tests/test_lmcs_verify.py on one opening"""
    out = []

    def put(**kw):
        out.append(dict(o, **kw))
    f, c = o["fields"], o["commitments"]
    bad = f.copy(); bad[f.size // 2] = (int(bad[f.size // 2]) + 1) % P
    put(fields=bad)
    if c.shape[0]:
        bad = c.copy(); bad[-1, 1] = (int(bad[-1, 1]) + 1) % P
        put(commitments=bad)
        put(commitments=c[:-1])
    bad = o["root"].copy(); bad[3] = (int(bad[3]) + 1) % P
    put(root=bad)
    put(fields=f[:-1])
    put(indices=o["indices"] + [1 << o["log_height"]])
    return out


def raw_batch(ctx, ops, lmcs, salt=0):
    """mh_lmcs_witness_batch on sentinel-filled buffers sized for the largest tree here -> (ok, [(leaf, paths, nodes)])"""
    items, arr = pkg._openings(ops)
    bufs = [[np.full(n, SENTINEL, dtype=np.uint64) for n in (4 * 1024, 4 * 1024 * 10, 4 * 2047)] for _ in items]
    outs = (pkg.LmcsWitnessOut * len(items))()
    for k, b in enumerate(bufs):
        outs[k].leaf_digests, outs[k].paths, outs[k].nodes = [x.ctypes.data_as(pkg.u64p) for x in b]
    ok = (C.c_int * len(items))()
    ctx.lib.mh_lmcs_witness_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(pkg.LmcsOpening), C.POINTER(pkg.LmcsWitnessOut),
                                              C.POINTER(C.c_int)]
    ctx.check(ctx.lib.mh_lmcs_witness_batch(ctx.h, pkg.Ctx.LMCS[lmcs], salt, len(items), arr, outs, ok))
    return [int(v) for v in ok], bufs


def check_raw(ok, bufs, batch, lmcs):
    for k, (o, b) in enumerate(zip(batch, bufs)):
        h = host_witness(o, lmcs, 0)
        assert ok[k] == int(h is not None), k
        if h is None:  # untouched
            assert all((x == SENTINEL).all() for x in b), k
        else:
            for x, a in zip(b, (h.leaf_digests, h.paths, h.nodes)):
                assert (x[:a.size] == a.reshape(-1)).all() and (x[a.size:] == SENTINEL).all(), k


@pytest.mark.parametrize("lmcs", ["poseidon2", "blake3"])
def test_forty_openings_three_damaged(ctx, lmcs):
    good = [o for o, _, _ in own_openings(ctx, lmcs, 0) if len(o["indices"]) < 200]
    batch = [good[i % len(good)] for i in range(40)]
    for k, which in ((3, 0), (17, 1), (39, 3)):
        d = damaged(batch[k])
        batch[k] = d[which % len(d)]
    ok, bufs = raw_batch(ctx, batch, lmcs)
    assert [i for i, v in enumerate(ok) if not v] == [3, 17, 39]
    check_raw(ok, bufs, batch, lmcs)


PASSES_CHILD = r"""
import os, sys
import numpy as np
os.environ["MH_VERIFY_BATCH_BYTES"] = "8000"   # a few of these openings per pass
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from __graft_entry__ import load_package
pkg = load_package()
ctx = pkg.Ctx(0)
rng = np.random.default_rng(8)
tree = pkg.commit_traces(ctx, [ctx.upload_trace(rng.integers(0, pkg.P, (32, 17), dtype=np.uint64))], 1).tree()
ops = []
for k in range(24):
    idx = [int(i) for i in rng.choice(64, 1 + k % 9, replace=False)]
    f, c = tree.prove_batch(idx, 8)
    ops.append(dict(root=tree.root(), log_height=6, widths=[17], alignment=8, indices=idx, fields=f, commitments=c))
bad = ops[11]["fields"].copy(); bad[0] = (int(bad[0]) + 1) % pkg.P
ops[11] = dict(ops[11], fields=bad)
ctx.prof_enable(True)
got = pkg.lmcs_witness_batch(ctx, ops)
passes = ctx.prof()["vfy_witness"]["count"]   # one launch of the witness kernel per pass
assert passes >= 3, passes
for k, (g, o) in enumerate(zip(got, ops)):
    if k == 11:
        assert g is None
        continue
    h = pkg.lmcs_witness(o)
    assert (g.leaf_digests == h.leaf_digests).all() and (g.paths == h.paths).all() and (g.nodes == h.nodes).all(), k
ctx.close()
print("passes", passes, "ok")
"""


def test_small_passes_give_the_same_arrays(tmp_path):
    """MH_VERIFY_BATCH_BYTES small enough for at least three passes, set in a fresh child process"""
    script = tmp_path / "passes_child.py"
    script.write_text(PASSES_CHILD)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_call_level_refusals(ctx):
    lib = ctx.lib
    lib.mh_lmcs_witness_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mh_lmcs_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    for lmcs_id, salt, n in [(0, 0, 0), (0, 0, 1), (9, 0, 0), (0, 9, 0), (0, -1, 0)]:
        want = lib.mh_lmcs_verify_batch(ctx.h, lmcs_id, salt, n, None, None)
        why = lib.mh_last_error(ctx.h).decode() if want else ""
        assert lib.mh_lmcs_witness_batch(ctx.h, lmcs_id, salt, n, None, None, None) == want
        assert not want or lib.mh_last_error(ctx.h).decode() == why
    assert lib.mh_lmcs_witness_batch(None, 0, 0, 0, None, None, None) == 1
    rng = np.random.default_rng(1)
    tree = pkg.commit_traces(ctx, [ctx.upload_trace(rng.integers(0, P, (1024, 1), dtype=np.uint64))], 1).tree()
    big = open_tree(tree, list(range(1025)), 8)
    assert pkg.lmcs_witness(big).nodes.shape[0] == pkg.lmcs_witness_size(big)[1]   # the host call has no such bound
    with pytest.raises(pkg.MidenHipError, match="1024"):
        pkg.lmcs_witness_batch(ctx, [big])
    w = tree.witness([5, 9], *tree.prove_batch([5, 9], 8))
    assert (w.root() == tree.root()).all() and list(w.indices) == [5, 9]
    tree.free()


# ---- whole proofs ------------------------------------------------------------------------------------------------------------------
TOY = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5, query_pow_bits=3)
PARAMS = {"arity2": dict(TOY, log_folding_arity=1), "arity4": TOY}


def statement(name, log_n):
    if name == "logup":
        air, _ = A.logup_air()
        return [air], [A.logup_trace(log_n)], []
    t1, pub1 = A.fib_trace(log_n)               # the preprocessed tree (2^5 rows) is shorter than the maximum domain
    pair3, ptr3 = A.prep_air(5, num_public=3)
    return [A.fib_air(), pair3], [t1, ptr3()], pub1


def prove_item(ctx, lmcs, name, log_n, prm, salt=0):
    airs_, traces, pub = statement(name, log_n)
    ctx.set_lmcs(lmcs)
    ctx.set_salt(salt, SEED)
    try:
        dairs = [pkg.DeviceAir(ctx, a) for a in airs_]
        order = sorted(range(len(airs_)), key=lambda i: (traces[i].shape[0], i))
        with_prep = [i for i in order if airs_[i].preprocessed is not None]
        root = None
        if with_prep:  # the setup: commit the preprocessed matrices in proof order
            com = pkg.commit_traces(ctx, [ctx.upload_trace(airs_[i].preprocessed) for i in with_prep], prm["log_blowup"])
            for k, i in enumerate(with_prep):
                dairs[i].attach_preprocessed(com.tree(), k)
            root = com.root()

        def aux_builder(idx, rnd):
            a = airs_[idx]
            if a.build_aux is None:
                return np.zeros((traces[idx].shape[0], 2 * a.aux_width), dtype=np.uint64), [0] * (2 * a.num_aux_values)
            return a.build_aux(traces[idx], rnd[:a.num_randomness])
        pre = ob.protocol_pre_observe(prm, pub, preprocessed_root=root)
        proof = pkg.prove(ctx, dairs, [ctx.upload_trace(t) for t in traces], pub, prm, ob.challenger_state(), pre,
                          aux_builder if any(a.build_aux is not None for a in airs_) else None)
    finally:
        ctx.set_salt(0)
        ctx.set_lmcs("poseidon2")
    item = dict(log_trace_heights=proof.log_trace_heights, public_values=pub, pre_observe=pre, fields=proof.fields,
                commitments=proof.commitments, preprocessed_root=root)
    return airs_, item


def tree_widths(airs_, item, prm, alignment, n_rounds):
    """the (already aligned) widths of the matrices of every tree, proof order: [preprocessed?, main, aux, quotient], FRI rounds"""
    lhs = item["log_trace_heights"]
    order = sorted(range(len(airs_)), key=lambda i: (lhs[i], i))
    al = lambda w: (w + alignment - 1) // alignment * alignment
    logD = max(a.log_quotient_degree for a in airs_)
    out = []
    if item["preprocessed_root"] is not None:
        out.append([al(airs_[i].preprocessed_width) for i in order if airs_[i].preprocessed_width])
    out += [[al(airs_[i].main_width) for i in order], [al(2 * airs_[i].aux_width) for i in order], [al(2 << logD)]]
    return out + [[2 << prm["log_folding_arity"]]] * n_rounds


def check_trees(trees, airs_, item, prm, lmcs, salt):
    L = max(item["log_trace_heights"]) + prm["log_blowup"]
    rounds = PP.fri_num_rounds(prm, L)
    n_committed = 4 if item["preprocessed_root"] is not None else 3
    assert len(trees) == n_committed + rounds
    assert [(t.kind, t.which) for t in trees] == [(0, k) for k in range(n_committed)] + [(1, r) for r in range(rounds)]
    com = np.asarray(item["commitments"], dtype=np.uint64).reshape(-1, 4)
    roots = ([np.asarray(item["preprocessed_root"])] if n_committed == 4 else []) + [com[k] for k in range(3 + rounds)]
    widths = tree_widths(airs_, item, prm, OWN_ALIGN[lmcs], rounds)
    n_paths = 0
    for t, root, ws in zip(trees, roots, widths):
        assert (t.tree_root == root).all() and (t.root() == root).all(), (t.kind, t.which)
        assert t.rows.shape == (t.indices.size, sum(w for w in ws if w) + salt)
        for q, i in enumerate(t.indices):  # every path verifies alone
            ok, why = pkg.lmcs_verify(dict(root=root, log_height=t.depth, widths=[w for w in ws if w], alignment=1, indices=[int(i)],
                                           fields=t.rows[q], commitments=t.path(int(i))), lmcs, salt)
            assert ok, (t.kind, t.which, int(i), why)
            n_paths += 1
    # the opened rows are the tail of the proof's field stream, tree after tree
    tail = np.concatenate([t.rows.reshape(-1) for t in trees])
    assert (item["fields"][-tail.size:] == tail).all()
    return n_paths


CASES = [("poseidon2", "arity2", "logup", 0), ("poseidon2", "arity4", "prep_shorter", 0), ("blake3", "arity2", "prep_shorter", 0),
         ("blake3", "arity4", "logup", 0), ("poseidon2", "arity4", "logup", 4)]


@pytest.mark.parametrize("lmcs,params,name,salt", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_verify_batch_witness(ctx, lmcs, params, name, salt):
    prm = PARAMS[params]
    airs_, item = prove_item(ctx, lmcs, name, 7 if name == "prep_shorter" else 5, prm, salt)
    plain = pkg.verify_batch(ctx, airs_, [item], prm, ob.challenger_state(), lmcs=lmcs, salt_elems=salt)
    got, trees = pkg.verify_batch(ctx, airs_, [item], prm, ob.challenger_state(), lmcs=lmcs, salt_elems=salt, witness=True)
    assert plain[0][0] and got[0][0] and (got[0][1] == plain[0][1]).all()
    n_paths = check_trees(trees[0], airs_, item, prm, lmcs, salt)
    # one damaged opened row: the first felt of the main tree's rows, found through the good item's witness
    main = 1 if item["preprocessed_root"] is not None else 0
    pos = item["fields"].size - sum(t.rows.size for t in trees[0][main:])
    f = item["fields"].copy()
    assert int(f[pos]) == int(trees[0][main].rows[0, 0])
    f[pos] = (int(f[pos]) + 1) % P
    items = [item, dict(item, fields=f), item]
    plain = pkg.verify_batch(ctx, airs_, items, prm, ob.challenger_state(), lmcs=lmcs, salt_elems=salt)
    got, trees3 = pkg.verify_batch(ctx, airs_, items, prm, ob.challenger_state(), lmcs=lmcs, salt_elems=salt, witness=True)
    assert [g[0] for g in got] == [p[0] for p in plain] == [True, False, True]
    assert got[1][1] == plain[1][1] and "Merkle root mismatch (committed tree" in got[1][1]
    assert (got[0][1] == plain[0][1]).all() and (got[2][1] == plain[2][1]).all()
    assert trees3[1] == []
    for k in (0, 2):
        assert len(trees3[k]) == len(trees[0]) and all(same(a, b) and (a.rows == b.rows).all() for a, b in zip(trees3[k], trees[0]))
    print(lmcs, params, name, salt, "trees", len(trees[0]), "paths", n_paths)


def test_verify_miden_batch_witness(ctx):
    import ref_traces as RT
    c = min(RT.load_cases()[:8], key=lambda c: c["core"].shape[0])
    m = pkg.Miden(ctx)
    try:
        pv, aux_in = RT.public_values(c), RT.aux_inputs(c)
        data = m.prove(c["core"], c["chiplets"], c["poseidon2"], pv, aux_in, hash_fn="poseidon2").bytes
    finally:
        m.free()
    items = [(pv, aux_in, data[:-8]), (pv, aux_in, data), (pv[:16] + [(pv[16] + 1) % P] + pv[17:], aux_in, data)]
    plain = pkg.verify_miden_batch(ctx, items)
    got, trees = pkg.verify_miden_batch(ctx, items, witness=True)
    assert [g[0] for g in got] == [p[0] for p in plain] == [False, True, False]
    assert (got[1][1] == plain[1][1]).all() and got[0][1] == plain[0][1] and got[2][1] == plain[2][1]
    assert trees[0] == [] and trees[2] == [] and len(trees[1]) >= 3   # main, aux, quotient, then whatever FRI rounds a trace this short has
    assert [(t.kind, t.which) for t in trees[1]] == [(0, 0), (0, 1), (0, 2)] + [(1, r) for r in range(len(trees[1]) - 3)]
    for t in trees[1]:
        assert t.depth == t.paths.shape[1] and (t.root() == t.tree_root).all()
        host = pkg.lmcs_witness(dict(root=t.tree_root, log_height=t.depth, widths=[t.rows.shape[1]], alignment=1,
                                     indices=[int(i) for i in t.indices], fields=t.rows.reshape(-1),
                                     commitments=streamed(t)), "poseidon2")
        assert same(host, t)


def streamed(t):
    """the commitment stream of the batch opening a witness came from: per level, left to right, the path elements of the opened nodes
    whose sibling is not itself derived"""
    out, level = [], [int(i) for i in t.indices]
    leaf_of = {i: q for q, i in enumerate(level)}
    for l in range(t.depth):
        s = set(level)
        for x in level:
            if (x ^ 1) not in s:
                q = next(q for i, q in leaf_of.items() if i >> l == x)
                out.append(t.paths[q, l])
        level = sorted({x >> 1 for x in level})
    return np.array(out, dtype=np.uint64).reshape(-1, 4)


def test_c_example(tmp_path):
    exe = str(tmp_path / "witness_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "witness_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    for lmcs in ("0", "1"):
        out = subprocess.check_output([exe, lmcs], text=True, timeout=120)
        assert "paths: each verified on its own" in out and "FRI round tree 0" in out, out
