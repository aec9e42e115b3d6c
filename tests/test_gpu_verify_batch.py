"""GPU tests of the batch verifier (run with -m gpu): the two kernels of csrc/verify_batch.hip through mh_lmcs_verify_batch, whole
proofs through mh_verify_batch and mh_verify_miden_batch, and the C example.

The yardstick is always the host: mh_lmcs_verify for an opening, mh_verify_hiding / mh_verify_miden for a proof.  The device
verdict must equal it for every item, good or damaged; damage sits where the host verifier rejects in every case (opened rows,
siblings, roots, the final polynomial -- tests/test_lmcs_verify.py and tests/test_verifier_cpu.py show that on the CPU)."""
import ctypes as C
import os, subprocess
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
# (rows, width) per matrix, log_blowup: log LDE heights 1, 2, 6 (two matrices of different heights: the shorter one is lifted), 10
TREES = {"h1_w1": ([(2, 1)], 0), "h2_w8": ([(2, 8)], 1), "h6_w9_w17": ([(16, 9), (32, 17)], 1), "h10_w17": ([(512, 17)], 1)}


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
    h = 1 << log_height
    sets = {"one": [h - 1], "two_adjacent": [2, 3] if h >= 4 else [0, 1], "two_apart": [0, h - 1], "all": list(range(h))}
    if log_height == 10:
        rng = np.random.default_rng(log_height)
        for n in (65, 130):  # more than one wave of leaves; 130 also makes the pair loop stride at the lowest level
            pick = [int(i) for i in rng.choice(h, n, replace=False)]
            sets[f"{n}_leaves"] = pick + pick[:3]  # unsorted, with duplicates
    return sets


def open_tree(tree, indices, alignment):
    f, c = tree.prove_batch(indices, alignment)
    return dict(root=tree.root(), log_height=tree.log_height, widths=list(tree.widths), alignment=alignment, indices=list(indices),
                fields=f, commitments=c)


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
    put(fields=np.append(f, np.uint64(0)))
    put(commitments=np.concatenate([c.reshape(-1, 4), np.ones((1, 4), dtype=np.uint64)]))
    bad = f.copy(); bad[0] = P
    put(fields=bad)
    put(indices=o["indices"] + [1 << o["log_height"]])
    return out


def host_verdicts(ops, lmcs, salt):
    return [int(pkg.lmcs_verify(o, lmcs, salt)[0]) for o in ops]


def same_leaves(lmcs, alignment, widths):
    """Does a row padded to `alignment` hash to the tree's leaf?  The tree absorbs the raw row: a sponge fills its last block with
    zeros, so padding that adds no block changes nothing (rate 8, or 17 for Keccak: width 17 padded to 24 takes one block more);
    the Blake3 chaining hasher hashes the padding itself.  An opening that does not is well formed but belongs to another tree:
    host and device must both say so."""
    al = lambda w: (w + alignment - 1) // alignment * alignment
    if lmcs == "blake3":
        return all(al(w) == w for w in widths)
    rate = 17 if lmcs == "keccak" else 8
    return all(-(-al(w) // rate) == -(-w // rate) for w in widths)


def all_openings(ctx, lmcs, salt):
    ctx.set_lmcs(lmcs)
    ctx.set_salt(salt, SEED)
    try:
        ops, expect = [], []
        for name in TREES:
            tree = commit(ctx, name)
            assert tree.salt_elems == salt
            for alignment in (8, 1) + ((17,) if lmcs == "keccak" else ()):
                for idx in index_sets(tree.log_height).values():
                    ops.append(open_tree(tree, idx, alignment))
                    expect.append(int(same_leaves(lmcs, alignment, tree.widths)))
            tree.free()
        return ops, expect
    finally:
        ctx.set_salt(0)
        ctx.set_lmcs("poseidon2")


@pytest.mark.parametrize("salt", [0, 1, 8])
@pytest.mark.parametrize("lmcs", HASHES)
def test_openings_verify_and_damaged_ones_do_not(ctx, lmcs, salt):
    ops, expect = all_openings(ctx, lmcs, salt)
    got = pkg.lmcs_verify_batch(ctx, ops, lmcs, salt)
    host = host_verdicts(ops, lmcs, salt)
    print(lmcs, salt, "openings", len(ops), "accepted", sum(got))
    assert host == expect          # the yardstick itself
    assert got == host
    assert sum(got) >= len(ops) // 2
    good = [o for o, e in zip(ops, expect) if e]
    bad = [d for o in good[::3] for d in damaged(o)]
    got_bad = pkg.lmcs_verify_batch(ctx, bad, lmcs, salt)
    assert got_bad == [0] * len(bad)
    assert host_verdicts(bad, lmcs, salt) == got_bad


@pytest.mark.parametrize("lmcs", ["poseidon2", "blake3"])
def test_forty_openings_three_damaged(ctx, lmcs):
    ops, expect = all_openings(ctx, lmcs, 0)
    good = [o for o, e in zip(ops, expect) if e]
    batch = [good[i % len(good)] for i in range(40)]
    for k, which in ((3, 0), (17, 1), (39, 3)):
        batch[k] = damaged(batch[k])[which if batch[k]["commitments"].shape[0] else 0]
    got = pkg.lmcs_verify_batch(ctx, batch, lmcs, 0)
    assert [i for i, v in enumerate(got) if not v] == [3, 17, 39]
    assert host_verdicts(batch, lmcs, 0) == got
    old = os.environ.get("MH_VERIFY_BATCH_BYTES")
    os.environ["MH_VERIFY_BATCH_BYTES"] = "20000"  # a few openings per pass
    try:
        assert pkg.lmcs_verify_batch(ctx, batch, lmcs, 0) == got
    finally:
        os.environ.pop("MH_VERIFY_BATCH_BYTES") if old is None else os.environ.__setitem__("MH_VERIFY_BATCH_BYTES", old)


def test_call_level_refusals(ctx):
    lib = ctx.lib
    lib.mh_lmcs_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(pkg.LmcsOpening), C.POINTER(C.c_int)]
    assert lib.mh_lmcs_verify_batch(ctx.h, 0, 0, 0, None, None) == 0          # nothing to do
    assert lib.mh_lmcs_verify_batch(ctx.h, 0, 0, 1, None, None) == 1
    assert "null" in lib.mh_last_error(ctx.h).decode()
    assert pkg.verify_batch(ctx, [A.fib_air()], [], TOY, ob.challenger_state()) == []
    with pytest.raises(pkg.MidenHipError, match="unknown LMCS"):
        ctx.check(lib.mh_lmcs_verify_batch(ctx.h, 9, 0, 0, None, None))
    # more distinct leaves than the path kernel's LDS arrays hold: refused with a reason, nothing launched
    rng = np.random.default_rng(1)
    tree = pkg.commit_traces(ctx, [ctx.upload_trace(rng.integers(0, P, (1024, 1), dtype=np.uint64))], 1).tree()
    big = open_tree(tree, list(range(1025)), 8)
    assert pkg.lmcs_verify(big)[0]
    with pytest.raises(pkg.MidenHipError, match="1024"):
        pkg.lmcs_verify_batch(ctx, [big])
    assert pkg.lmcs_verify_batch(ctx, [open_tree(tree, list(range(1024)), 8)]) == [1]
    assert tree.verify_open([5, 9], *tree.prove_batch([5, 9], 8))[0]
    tree.free()


# ---- whole proofs ------------------------------------------------------------------------------------------------------------------
TOY = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5, query_pow_bits=3)
PARAMS = {"arity2": dict(TOY, log_folding_arity=1), "arity4": TOY, "arity8": dict(TOY, log_folding_arity=3, log_final_degree=1)}


def statement(name, log_n):
    if name == "logup":
        air, _ = A.logup_air()
        return [air], [A.logup_trace(log_n)], []
    t1, pub1 = A.fib_trace(log_n)               # the preprocessed tree (2^5 rows) is shorter than the maximum domain
    pair3, ptr3 = A.prep_air(5, num_public=3)
    return [A.fib_air(), pair3], [t1, ptr3()], pub1


def prove_item(ctx, lmcs, name, log_n, prm, salt=0):
    """-> the item as verify_batch takes it, plus what the host verifier and the walk over its streams need"""
    from test_gpu_prove import attach_preprocessed
    airs_, traces, pub = statement(name, log_n)
    ctx.set_lmcs(lmcs)
    ctx.set_salt(salt, SEED)
    try:
        dairs = [pkg.DeviceAir(ctx, a) for a in airs_]
        root = attach_preprocessed(ctx, airs_, dairs, traces, prm)

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
    return airs_, item, proof


def host_verify(airs_, item, prm, lmcs, salt):
    return pkg.verify(airs_, item["log_trace_heights"], item["public_values"], prm, ob.challenger_state(), item["pre_observe"],
                      item["fields"], item["commitments"], preprocessed_root=item["preprocessed_root"], lmcs=lmcs, salt_elems=salt)


def hurt(item, where, lmcs=None, airs_=None, prm=None, proof=None, salt=0):
    """one defect: "row" = an opened row of the main tree, "sibling" = a sibling of the last FRI round tree that streams one,
    "final" = the final polynomial, "last_row" = the last opened row of the last FRI round tree (needs no walk)"""
    f, c = item["fields"].copy(), np.array(item["commitments"], dtype=np.uint64).copy()
    if where == "sibling":
        c[-1, 2] = (int(c[-1, 2]) + 1) % P if lmcs not in ("blake3", "keccak") else int(c[-1, 2]) ^ 1
    elif where == "last_row":
        f[-1] = (int(f[-1]) + 1) % P
    else:
        from test_gpu_hiding_lmcs import walk
        ob.set_lmcs(lmcs)
        try:
            trees, end = walk(airs_, item["log_trace_heights"], item["public_values"], prm, proof, item["preprocessed_root"], OWN_ALIGN[lmcs], salt)
        finally:
            ob.set_lmcs("poseidon2")
        assert end == f.size
        main = trees[1 if item["preprocessed_root"] is not None else 0]
        pos = main[1] + 1 if where == "row" else trees[0][1] - 2  # "final": the last coefficient, in front of the query PoW witness
        f[pos] = (int(f[pos]) + 1) % P
    return dict(item, fields=f, commitments=c)


def compare(ctx, airs_, items, prm, lmcs, salt=0):
    got = pkg.verify_batch(ctx, airs_, items, prm, ob.challenger_state(), lmcs=lmcs, salt_elems=salt)
    host = [host_verify(airs_, it, prm, lmcs, salt) for it in items]
    for k, (g, h) in enumerate(zip(got, host)):
        assert g[0] == h[0], (k, g, h)
        if g[0]:
            assert (g[1] == h[1]).all(), k
    return got, host


CASES = [("poseidon2", "arity2", "logup", 0), ("poseidon2", "arity4", "prep_shorter", 0), ("poseidon2", "arity8", "logup", 0),
         ("blake3", "arity2", "prep_shorter", 0), ("blake3", "arity4", "logup", 0), ("blake3", "arity8", "logup", 0),
         ("poseidon2", "arity4", "logup", 4), ("blake3", "arity4", "logup", 4),
         ("keccak", "arity4", "logup", 0), ("rpo", "arity4", "logup", 0), ("rpx", "arity4", "logup", 0)]


@pytest.mark.parametrize("lmcs,params,name,salt", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_verify_batch_equals_the_host_verifier(ctx, lmcs, params, name, salt):
    prm = PARAMS[params]
    log_n = 7 if name == "prep_shorter" else 5
    airs_, item, proof = prove_item(ctx, lmcs, name, log_n, prm, salt)
    items = [item, hurt(item, "last_row"), hurt(item, "sibling", lmcs)]
    if lmcs in ("poseidon2", "blake3"):
        items += [hurt(item, w, lmcs, airs_, prm, proof, salt) for w in ("row", "final")]
    got, host = compare(ctx, airs_, items, prm, lmcs, salt)
    assert [g[0] for g in got] == [True] + [False] * (len(items) - 1)
    assert (got[0][1] == proof.digest).all()
    assert "Merkle root mismatch (FRI round" in got[1][1] and "Merkle root mismatch (FRI round" in got[2][1]
    if len(items) > 3:
        n_trees = 4 if item["preprocessed_root"] is not None else 3
        assert f"Merkle root mismatch (committed tree {n_trees - 3} of {n_trees})" in got[3][1]
        assert got[4][1] == host[4][1] and "Merkle" not in got[4][1]   # the replay's own reason


@pytest.mark.parametrize("lmcs", ["poseidon2", "blake3"])
def test_twenty_four_proofs_mixed_heights(ctx, lmcs):
    prm = TOY
    made = [prove_item(ctx, lmcs, "logup", log_n, prm) for log_n in range(3, 9)]  # 2^3 .. 2^8 rows
    airs_ = made[0][0]
    items = [made[k % 6][1] for k in range(24)]
    a, it, pr = made[0]
    items[0] = hurt(it, "row", lmcs, a, prm, pr)
    a, it, pr = made[7 % 6]
    items[7] = hurt(it, "sibling", lmcs)
    a, it, pr = made[23 % 6]
    items[23] = hurt(it, "final", lmcs, a, prm, pr)
    got, host = compare(ctx, airs_, items, prm, lmcs)
    assert [k for k, g in enumerate(got) if not g[0]] == [0, 7, 23]
    assert "Merkle root mismatch (committed tree 0 of 3)" in got[0][1]
    assert "Merkle root mismatch (FRI round" in got[7][1]
    assert got[23][1] == host[23][1]
    old = os.environ.get("MH_VERIFY_BATCH_BYTES")
    os.environ["MH_VERIFY_BATCH_BYTES"] = "4096"  # smaller than any one opening: a pass per opening
    try:
        again = pkg.verify_batch(ctx, airs_, items, prm, ob.challenger_state(), lmcs=lmcs)
    finally:
        os.environ.pop("MH_VERIFY_BATCH_BYTES") if old is None else os.environ.__setitem__("MH_VERIFY_BATCH_BYTES", old)
    assert [(g[0], g[1] if not g[0] else list(g[1])) for g in again] == [(g[0], g[1] if not g[0] else list(g[1])) for g in got]


@pytest.mark.parametrize("hash_fn", ["poseidon2", "blake3"])
def test_verify_miden_batch(ctx, hash_fn):
    import ref_traces as RT
    cases = RT.load_cases()[:8]
    m = pkg.Miden(ctx)
    try:
        items = []
        for c in cases:
            pv, aux_in = RT.public_values(c), RT.aux_inputs(c)
            items.append((pv, aux_in, m.prove(c["core"], c["chiplets"], c["poseidon2"], pv, aux_in, hash_fn=hash_fn).bytes))
    finally:
        m.free()
    pv, aux_in, data = items[5]
    items[5] = (pv[:16] + [(pv[16] + 1) % P] + pv[17:], aux_in, data)  # another statement
    items.append((pv, aux_in, data[:-8]))                              # malformed bytes reject that item alone
    got = pkg.verify_miden_batch(ctx, items, hash_fn=hash_fn)
    host = [pkg.verify_miden(*it, hash_fn=hash_fn) for it in items]
    assert [g[0] for g in got] == [h[0] for h in host] == [k not in (5, 8) for k in range(9)]
    for g, h in zip(got, host):
        assert (g[1] == h[1]).all() if g[0] else g[1] == h[1]


def test_c_example(tmp_path):
    exe = str(tmp_path / "verify_batch_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "verify_batch_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    for lmcs in ("0", "1"):
        out = subprocess.check_output([exe, lmcs, "6"], text=True, timeout=120)
        assert "batch of 6 verified: 1 rejected, 5 accepted" in out, out
        assert "proof 1 (2^5 rows): rejected: proof rejected: Merkle root mismatch (FRI round" in out, out
