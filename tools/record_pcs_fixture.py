"""Record tests/golden/pcs_open.json: three standalone PCS openings (mh_pcs_open) made on the GPU, for the CPU-only verifier test
tests/test_pcs_abi.py -- N = 1 and N = 3 points under Poseidon2, N = 2 under Blake3; toy parameters, one tree of a 2^4 x 3 matrix and a
2^3 x 2 matrix (the short one is lifted).  Everything is seeded, so a second run writes the same file.
    python tools/record_pcs_fixture.py [OUT.json]        (needs a GPU; default OUT = tests/golden/pcs_open.json)
Each proof is verified with mh_pcs_verify before it is written; the recorded evaluations are the verifier's (padding dropped)."""
import json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import protocol

P = pkg.P
PARAMS = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5, query_pow_bits=3)
SHAPE = [(8, 2), (16, 3)]
CASES = [("poseidon2", 1), ("poseidon2", 3), ("blake3", 2)]
ALIGN = {"poseidon2": 8, "blake3": 1}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pcs_open.json")
    rng = np.random.default_rng(20)
    mats = [rng.integers(0, P, s, dtype=np.uint64) for s in SHAPE]
    log_n = max(int(m.shape[0]).bit_length() - 1 for m in mats)
    points = []
    while len(points) < 3:
        z = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
        if pkg.pcs_point_ok(log_n, PARAMS["log_blowup"], z):
            points.append(z)
    state = [int(x) for x in protocol.challenger_state()]
    L = log_n + PARAMS["log_blowup"]
    steps = max(0, L - PARAMS["log_final_degree"] - PARAMS["log_blowup"])
    rounds = -(-steps // PARAMS["log_folding_arity"])
    proofs = []
    ctx = pkg.Ctx(0)
    for lmcs, n in CASES:
        ctx.set_lmcs(lmcs)
        tree = pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in mats], PARAMS["log_blowup"]).tree()
        root = [int(x) for x in tree.root()]
        pts = points[:n]
        proof = pkg.pcs_open(ctx, [tree], pts, PARAMS, state, root)
        widths = [[int(m.shape[1]) for m in mats]]
        ok, digest, evals = pkg.pcs_verify([root], [log_n], widths, pts, PARAMS, state, root, proof.fields, proof.commitments, lmcs=lmcs)
        assert ok and (digest == proof.digest).all(), digest
        a = ALIGN[lmcs]
        proofs.append(dict(lmcs=lmcs, n_points=n, points=[list(z) for z in pts], roots=[root], log_tree_heights=[log_n], widths=widths,
                           pre_observe=root, ood_width=sum(-(-w // a) * a for w in widths[0]), num_fri_rounds=rounds,
                           final_poly_len=1 << max(0, L - rounds * PARAMS["log_folding_arity"] - PARAMS["log_blowup"]),
                           fields=[int(x) for x in proof.fields], commitments=[[int(x) for x in c] for c in proof.commitments],
                           digest=[int(x) for x in proof.digest], evals=[[[int(x) for x in e] for e in row] for row in evals]))
        tree.free()
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(dict(params=PARAMS, challenger_state=state, matrices=[[[int(x) for x in r] for r in m] for m in mats], proofs=proofs), f,
                  separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
