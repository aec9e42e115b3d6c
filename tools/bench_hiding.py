"""The hiding LMCS (mh_ctx_set_salt) on the bench instance miden:LOG_N:51:8 at the production parameters: proof time
and the `lmcs_leaf_absorb` / `fri_leaf_hash` profiler spans per salt width.
    python tools/bench_hiding.py [--root DIR] [--log-n 20] [--salts 0,4,8] [--reps 7] [--lmcs poseidon2]
--root DIR measures another checkout of this repository (its package and its library, e.g. the parent commit, which has no salt:
give it --salts 0).  Prints one JSON line per salt width: min / median / max milliseconds over `reps` proofs after two warm-up
proofs (wall clock around the blocking mh_prove), then, from a separate profiled proof, the spans.  A salt-off timing is compared
with the parent by running this script alternately on both checkouts (measuring-on-mi355x: interleave, look at the spread)."""
import argparse, importlib.util, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--salts", default="0,4,8")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--lmcs", default="poseidon2")
ap.add_argument("--tag", default="")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
spec = importlib.util.spec_from_file_location("__graft_entry__", os.path.join(root, "__graft_entry__.py"))
entry = importlib.util.module_from_spec(spec)
sys.modules["__graft_entry__"] = entry
spec.loader.exec_module(entry)
pkg = entry.load_package()
import numpy as np
from miden_vm_amd import dag, protocol

ctx = pkg.Ctx(0)
ctx.set_lmcs(args.lmcs)
air = dag.dummy_miden_air(51, 8)
dair = pkg.DeviceAir(ctx, air)
rng = np.random.default_rng(7)
host = rng.integers(0, pkg.P, (1 << args.log_n, 51), dtype=np.uint64)
host[:, 0] = 0
trace = ctx.upload_trace(host)
params, state = dict(protocol.PROD_PARAMS), protocol.challenger_state()
pre = protocol.protocol_pre_observe(params, [])
SEED = [1, 2, 3, 4]


def prove(salt):
    if salt:
        ctx.set_salt(salt, SEED)  # a fixed seed: every repetition makes the same proof
    return pkg.prove(ctx, [dair], [trace], [], params, state, pre, None)


for salt in [int(x) for x in args.salts.split(",")]:
    if salt == 0 and hasattr(ctx, "set_salt"):
        ctx.set_salt(0)
    for _ in range(2):
        proof = prove(salt)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        proof = prove(salt)
        ts.append((time.perf_counter() - t0) * 1e3)
    ctx.prof_enable(True)
    ctx.prof_reset()
    prove(salt)
    prof = ctx.prof()
    ctx.prof_enable(False)
    spans = {k: round(prof[k]["ms"], 3) for k in ("lmcs_leaf_absorb", "fri_leaf_hash", "lmcs_compress") if k in prof}
    print(json.dumps({"tag": args.tag, "root": os.path.basename(root), "lmcs": args.lmcs, "log_n": args.log_n, "salt": salt,
                      "proof_ms": {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)},
                      "reps": args.reps, "spans_ms_profiled_proof": spans, "fields": int(proof.fields.size),
                      "commitments": int(len(proof.commitments))}), flush=True)
ctx.close()
