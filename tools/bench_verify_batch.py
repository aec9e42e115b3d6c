"""The batch verifier against one host thread, on the real Miden statement of a 2^16-row program at the production parameters.
    python tools/bench_verify_batch.py [iterations=575] [hashes=poseidon2,blake3] [sizes=1,8,64,512] [mode=verify|witness]
Per hash function: mh_verify_miden per proof on one host thread (the yardstick), then mh_verify_miden_batch at each batch size:
wall time per proof (a host clock around the call, which ends in the read-back of the verdicts), the split into host replay, upload
and the two kernels from the mh_prof_* scopes (a separate, profiled call), and the batch size at which the batch entry first beats
the yardstick.  The batch holds the same proof n times: replay and hashing cost the same per copy, every copy has its own buffers.
mode=witness adds, per batch size, mh_verify_miden_batch_witness beside the plain call of the same build (wall time around the C
call, the set freed inside it; the vfy_* scopes of one profiled call of each), and per hash function the host-only mh_lmcs_witness
over the openings of one proof on one thread: the cost the device pass replaces.
One JSON line per measurement; needs a GPU (no fallback)."""
import ctypes as C
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import core_trace as ct  # noqa: E402


SCOPES = ("vfy_replay", "vfy_upload", "vfy_leaves", "vfy_paths", "vfy_witness", "vfy_readback")


def witness_call(ctx, items, hash_fn):
    """mh_verify_miden_batch_witness through ctypes without copying the set out: () -> number of trees of item 0"""
    n = len(items)
    arr = (pkg.MidenVerifyItem * n)()
    keep = []
    for k, (pv, aux, data) in enumerate(items):
        a, b = pkg._arr([int(x) for x in pv]), pkg._arr([int(x) for x in aux] or [0])
        buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
        keep.append((a, b, buf))
        arr[k].public_values, arr[k].aux_inputs, arr[k].n_aux_inputs = pkg._ptr(a), pkg._ptr(b), len(aux)
        arr[k].proof_bytes, arr[k].n_bytes = C.cast(buf, C.c_void_p), len(data)
    res = (pkg.VerifyResult * n)()
    lib = ctx.lib
    lib.mh_verify_miden_batch_witness.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(pkg.MidenVerifyItem), C.POINTER(pkg.VerifyResult),
                                                  C.POINTER(C.c_void_p)]
    lib.mh_witness_set_trees.restype = C.c_size_t
    lib.mh_witness_set_trees.argtypes = [C.c_void_p, C.c_size_t]
    lib.mh_witness_set_free.argtypes = [C.c_void_p]
    lib.mh_witness_set_free.restype = None

    def call():
        h = C.c_void_p()
        ctx.check(lib.mh_verify_miden_batch_witness(ctx.h, pkg.Ctx.LMCS[hash_fn], n, arr, res, C.byref(h)))
        trees = lib.mh_witness_set_trees(h, 0)
        lib.mh_witness_set_free(h)
        assert res[0].code == 0 and trees
        return trees
    call.keep = keep
    return call


def host_witness_ms(ctx, item, hash_fn):
    """mh_lmcs_witness on one thread over every opening of one proof.  A tree's leaf is re-hashed as one matrix of row_len cells: the
    same leaf under the sponges (every aligned width is a multiple of the rate); under Blake3's chaining hasher a tree of several
    matrices hashes the same bytes in one chain instead of several, so the call does the same work and then reports a root mismatch."""
    _, trees = pkg.verify_miden_batch(ctx, [item], hash_fn=hash_fn, witness=True)
    ops = []
    for t in trees[0]:
        sib = []
        level = [int(i) for i in t.indices]
        for l in range(t.depth):
            have = set(level)
            for x in level:
                if (x ^ 1) not in have:
                    sib.append(t.paths[next(q for q, i in enumerate(t.indices) if int(i) >> l == x), l])
            level = sorted({x >> 1 for x in level})
        ops.append(pkg.LmcsOpening.make(t.tree_root, t.depth, [t.rows.shape[1]], 1, [int(i) for i in t.indices], t.rows.reshape(-1),
                                        np.array(sib, dtype=np.uint64).reshape(-1, 4)))
    lib = ctx.lib
    lib.mh_lmcs_witness.argtypes = [C.c_int, C.c_int, C.POINTER(pkg.LmcsOpening), C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    bufs = [(C.c_uint64 * (4 * t.indices.size), C.c_uint64 * (4 * t.indices.size * max(1, t.depth)), C.c_uint64 * (4 * max(1, t.nodes.shape[0])))
            for t in trees[0]]
    bufs = [tuple(b() for b in bb) for bb in bufs]
    accepted = 0
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        accepted = sum(lib.mh_lmcs_witness(pkg.Ctx.LMCS[hash_fn], 0, C.byref(o), b[0], b[1], b[2], None, 0) == 0 for o, b in zip(ops, bufs))
    return (time.perf_counter() - t0) / reps * 1e3, len(ops), accepted


def main():
    mode = sys.argv[4] if len(sys.argv) > 4 else "verify"
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 575
    hashes = (sys.argv[2] if len(sys.argv) > 2 else "poseidon2,blake3").split(",")
    sizes = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,8,64,512").split(",")]
    ctx = pkg.Ctx(0)
    miden = pkg.Miden(ctx)
    r = ct.prove_inputs(ct.CoreVM(stack_inputs=list(range(16))), ct.bench_program(iters))
    pv, aux = r["public_values"], r["aux_inputs"]
    for hash_fn in hashes:
        proof = miden.prove(r["core"], r["chiplets"], r["poseidon2"], pv, aux, hash_fn=hash_fn)
        data = proof.bytes
        ok, dig = pkg.verify_miden(pv, aux, data, hash_fn=hash_fn)
        assert ok, dig
        reps = 30
        t0 = time.perf_counter()
        for _ in range(reps):
            pkg.verify_miden(pv, aux, data, hash_fn=hash_fn)
        host_ms = (time.perf_counter() - t0) / reps * 1e3
        print(json.dumps({"hash": hash_fn, "log_trace_heights": list(proof.log_trace_heights), "proof_bytes": len(data),
                          "mh_verify_miden_ms_per_proof_one_thread": round(host_ms, 3)}), flush=True)
        if mode == "witness":
            ms, n_ops, accepted = host_witness_ms(ctx, (pv, aux, data), hash_fn)
            print(json.dumps({"hash": hash_fn, "mh_lmcs_witness_ms_per_proof_one_thread": round(ms, 3), "openings": n_ops,
                              "accepted_as_single_matrix_trees": accepted}), flush=True)
        first_win = None
        for n in sizes:
            items = [(pv, aux, data)] * n
            res = pkg.verify_miden_batch(ctx, items, hash_fn=hash_fn)  # warm-up: code objects, pool, page-locked buffers
            assert all(x[0] for x in res) and (res[0][1] == dig).all()
            reps = max(3, min(30, 256 // n))
            t0 = time.perf_counter()
            for _ in range(reps):
                pkg.verify_miden_batch(ctx, items, hash_fn=hash_fn)
            wall_ms = (time.perf_counter() - t0) / reps * 1e3
            ctx.prof_reset()
            ctx.prof_enable(True)
            pkg.verify_miden_batch(ctx, items, hash_fn=hash_fn)
            prof = ctx.prof()
            ctx.prof_enable(False)
            split = {k: round(prof.get(k, {"ms": 0.0})["ms"], 3) for k in ("vfy_replay", "vfy_upload", "vfy_leaves", "vfy_paths")}
            if mode == "witness":
                call = witness_call(ctx, items, hash_fn)
                call()
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                w_ms = (time.perf_counter() - t0) / reps * 1e3
                ctx.prof_reset()
                ctx.prof_enable(True)
                call()
                wprof = ctx.prof()
                ctx.prof_enable(False)
                print(json.dumps({"hash": hash_fn, "batch": n, "witness_wall_ms_per_call": round(w_ms, 3), "witness_wall_ms_per_proof": round(w_ms / n, 4),
                                  "witness_profiled_call_ms": {k: round(wprof.get(k, {"ms": 0.0})["ms"], 3) for k in SCOPES if k != "vfy_paths"},
                                  "readback_bytes": wprof.get("vfy_readback", {"bytes": 0})["bytes"]}), flush=True)
            if first_win is None and wall_ms / n < host_ms:
                first_win = n
            print(json.dumps({"hash": hash_fn, "batch": n, "wall_ms_per_call": round(wall_ms, 3), "wall_ms_per_proof": round(wall_ms / n, 4),
                              "profiled_call_ms": split, "upload_bytes": prof.get("vfy_upload", {"bytes": 0})["bytes"]}), flush=True)
        print(json.dumps({"hash": hash_fn, "first_batch_size_that_beats_one_host_thread": first_win}), flush=True)
    miden.free()
    ctx.close()


if __name__ == "__main__":
    main()
