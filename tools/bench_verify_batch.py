"""The batch verifier against one host thread, on the real Miden statement of a 2^16-row program at the production parameters.
    python tools/bench_verify_batch.py [iterations=575] [hashes=poseidon2,blake3] [sizes=1,8,64,512]
Per hash function: mh_verify_miden per proof on one host thread (the yardstick), then mh_verify_miden_batch at each batch size:
wall time per proof (a host clock around the call, which ends in the read-back of the verdicts), the split into host replay, upload
and the two kernels from the mh_prof_* scopes (a separate, profiled call), and the batch size at which the batch entry first beats
the yardstick.  The batch holds the same proof n times: replay and hashing cost the same per copy, every copy has its own buffers.
One JSON line per measurement; needs a GPU (no fallback)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import core_trace as ct  # noqa: E402


def main():
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
            if first_win is None and wall_ms / n < host_ms:
                first_win = n
            print(json.dumps({"hash": hash_fn, "batch": n, "wall_ms_per_call": round(wall_ms, 3), "wall_ms_per_proof": round(wall_ms / n, 4),
                              "profiled_call_ms": split, "upload_bytes": prof.get("vfy_upload", {"bytes": 0})["bytes"]}), flush=True)
        print(json.dumps({"hash": hash_fn, "first_batch_size_that_beats_one_host_thread": first_win}), flush=True)
    miden.free()
    ctx.close()


if __name__ == "__main__":
    main()
