"""CPU-only: the standalone PCS's ABI (include/midenhip.h mh_pcs_*, mh_session_trees) agrees across the header, the Rust declarations
and the Python layer; mh_pcs_point_ok against the domain's definition; mh_pcs_verify -- host code -- refuses bad arguments and any
malformed stream with a reason, accepts the recorded openings of tests/golden/pcs_open.json (made on the GPU by
tools/record_pcs_fixture.py) and refuses each of them after every kind of tampering."""
import ctypes as C
import json, os, re, subprocess
import numpy as np
import pytest
from __graft_entry__ import load_package, ROOT

P = 0xFFFFFFFF00000001
ROOT_2_32 = 1753635133440165772
FUNCS = ["mh_pcs_point_ok", "mh_pcs_begin", "mh_pcs_free", "mh_pcs_shape", "mh_pcs_evals", "mh_pcs_deep", "mh_pcs_download_deep",
         "mh_pcs_fri_commit", "mh_pcs_fri_fold", "mh_pcs_fri_final", "mh_pcs_query", "mh_pcs_open", "mh_pcs_verify", "mh_session_trees"]
TOY = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5, query_pow_bits=3)
FIXTURE = os.path.join(ROOT, "tests", "golden", "pcs_open.json")


def params(src, name, close):
    body = re.search(name + r"\s*\((.*?)\)\s*" + close, src, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", p).strip() for p in body.split(",")]


def test_symbols_in_header_rust_and_exports():
    pkg = load_package()
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midenhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    lib = pkg.load_library()
    for f in FUNCS:
        assert re.search(r"\b(int|void)\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS and hasattr(lib, f), f
        # the same number of arguments in C and in Rust
        assert len(params(h, f, ";")) == len(params(rs, "pub fn " + f, r"(->|;)")), f
    assert int(re.search(r"#define\s+MH_PCS_MAX_POINTS\s+(\d+)", h).group(1)) == 4 == pkg.MH_PCS_MAX_POINTS
    assert int(re.search(r"pub const MH_PCS_MAX_POINTS: c_int = (\d+);", rs).group(1)) == 4
    # mh_pcs_shape_t: the same fields in the same order in C, Rust and ctypes
    c_fields = re.findall(r"(\w+)\s*;", re.search(r"typedef struct mh_pcs_shape_t \{(.*?)\}", h, flags=re.S).group(1))
    r_fields = re.findall(r"pub (\w+):", re.search(r"pub struct mh_pcs_shape_t \{(.*?)\}", rs, flags=re.S).group(1))
    assert c_fields == r_fields == [n for n, _ in pkg.PcsShape._fields_] == ["log_lde_height", "n_points", "ood_width", "num_fri_rounds",
                                                                           "final_poly_len"]
    assert "mh_pcs" in re.search(r"opaque!\((.*?)\);", rs).group(1).split(", ")
    # one-shot opening and verification take the same statement arguments, in the same order
    o, v = params(h, "mh_pcs_open", ";"), params(h, "mh_pcs_verify", ";")
    assert o[1] == v[2] == "const mh_pcs_params* params" and o[4:9] == v[8:13]
    # the header says whose job the roots are, and points from mh_commit_traces to the opening
    full = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    assert "BINDING THE ROOTS IS THE CALLER'S JOB" in full and "pre_observe" in full
    assert "mh_pcs_open" in re.search(r"/\* commit_traces \(crates.*?\*/", full, flags=re.S).group(0)


def test_c_snippet_compiles(tmp_path):
    src = tmp_path / "snippet.c"
    src.write_text(r'''
#include "midenhip.h"
int staged(mh_ctx* ctx, const mh_pcs_params* prm, const mh_tree* const* trees, const uint64_t* points, uint64_t* buf, mh_proof** out) {
  mh_pcs* p = 0;
  mh_pcs_shape_t sh;
  uint64_t ch[2] = {1, 2}, root[4], idx[1] = {0};
  if (!mh_pcs_point_ok(4, prm->log_blowup, points)) return MH_ERR_INVALID;
  int rc = mh_pcs_begin(ctx, prm, 1, trees, MH_PCS_MAX_POINTS, points, &p);
  if (rc) return rc;
  rc |= mh_pcs_shape(p, &sh);
  rc |= mh_pcs_evals(p, buf);
  rc |= mh_pcs_deep(p, ch, ch);
  rc |= mh_pcs_download_deep(p, buf);
  for (int r = 0; r < sh.num_fri_rounds; r++) rc |= mh_pcs_fri_commit(p, root) | mh_pcs_fri_fold(p, ch);
  rc |= mh_pcs_fri_final(p, buf);
  rc |= mh_pcs_query(p, idx, 1, out);
  mh_pcs_free(p);
  return rc + (int)sh.ood_width + (int)sh.final_poly_len + sh.n_points + sh.log_lde_height;
}
int one_shot(mh_ctx* ctx, mh_session* s, const mh_pcs_params* prm, const uint64_t* points, const uint64_t st[12], mh_proof** out, char* err) {
  const mh_tree* trees[4];
  int n = 0;
  uint64_t roots[16], digest[4];
  uint8_t lh[4] = {4, 4, 4, 4};
  int nm[4] = {1, 1, 1, 1};
  size_t w[4] = {3, 3, 3, 3};
  int rc = mh_session_trees(s, trees, 4, &n);
  for (int i = 0; i < n && !rc; i++) rc = mh_tree_root(trees[i], roots + 4 * i);
  if (!rc) rc = mh_pcs_open(ctx, prm, n, trees, 2, points, st, roots, (size_t)(4 * n), out);
  if (!rc)
    rc = mh_pcs_verify(MH_LMCS_POSEIDON2, 0, prm, n, roots, lh, nm, w, 2, points, st, roots, (size_t)(4 * n), mh_proof_fields(*out),
                       mh_proof_num_fields(*out), mh_proof_commitments(*out), mh_proof_num_commitments(*out), 0, digest, err, 64);
  return rc;
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "snippet.o")])


# ---- field arithmetic in Python integers ----
def emul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def epow2(a, k):
    for _ in range(k):
        a = emul(a, a)
    return a


def point_ok(log_n, lb, z):
    """domain.rs:539-553: nonzero, z^N != 1, (z / g)^K != 1 with g = 7^(2^(32 - log K)), K = N * B."""
    z = (z[0] % P, z[1] % P)
    if z == (0, 0) or epow2(z, log_n) == (1, 0):
        return False
    L = log_n + lb
    g_inv = pow(pow(7, 1 << (32 - L), P), P - 2, P)
    return epow2((z[0] * g_inv % P, z[1] * g_inv % P), L) != (1, 0)


def test_point_ok():
    pkg = load_package()
    log_n, lb = 4, 3
    L = log_n + lb
    w_n, w_k, g = pow(ROOT_2_32, 1 << (32 - log_n), P), pow(ROOT_2_32, 1 << (32 - L), P), pow(7, 1 << (32 - L), P)
    generic = (0x0123456789ABCDEF, 0x0FEDCBA987654321)
    cases = [(0, 0), (1, 0), (pow(w_n, 5, P), 0), (g, 0), (g * pow(w_k, 77, P) % P, 0), generic, (5, 0), (0, 3), (P, P), (P + 1, 0)]
    for z in cases:
        assert pkg.pcs_point_ok(log_n, lb, z) == point_ok(log_n, lb, z), z
    assert not pkg.pcs_point_ok(log_n, lb, (0, 0)) and not pkg.pcs_point_ok(log_n, lb, (pow(w_n, 5, P), 0))
    assert not pkg.pcs_point_ok(log_n, lb, (g * pow(w_k, 77, P) % P, 0)) and pkg.pcs_point_ok(log_n, lb, generic)
    # an element of the SHORTER domain's coset is on gK too (K' is a subgroup of K and g' = g^2): one check covers every height
    assert not pkg.pcs_point_ok(log_n, lb, (pow(w_n, 2, P), 0))
    # a point that is fine for a 2^4 domain but lies on H of a 2^5 one
    w32 = pow(ROOT_2_32, 1 << 27, P)
    assert pkg.pcs_point_ok(4, lb, (w32, 0)) and not pkg.pcs_point_ok(5, lb, (w32, 0))
    lib = pkg.load_library()
    assert lib.mh_pcs_point_ok(4, 3, None) == 0 and lib.mh_pcs_point_ok(30, 3, (C.c_uint64 * 2)(5, 0)) == 0


# ---- mh_pcs_verify on arguments and streams that are not proofs ----
def raw_verify(lib, pkg, n_trees=1, n_points=1, fields=b"", commitments=b"", nulls=(), lmcs=0, salt=0, widths=(3,), heights=(4,), prm=TOY,
               points=None):
    u64p = C.POINTER(C.c_uint64)
    p = pkg.PcsParams.from_dict(prm)
    roots = (C.c_uint64 * (4 * max(1, n_trees)))()
    lh = (C.c_uint8 * max(1, n_trees))(*heights)
    nm = (C.c_int * max(1, n_trees))(*([len(widths)] * max(1, n_trees)))
    ws = (C.c_size_t * (len(widths) * max(1, n_trees)))(*(list(widths) * max(1, n_trees)))
    pts = (C.c_uint64 * 16)(*(points or [0x0123456789ABCDEF, 0x0FEDCBA987654321] * 8))
    st = (C.c_uint64 * 12)()
    f = np.frombuffer(fields[:len(fields) // 8 * 8], dtype=np.uint64).copy()
    cm = np.frombuffer(commitments[:len(commitments) // 32 * 32], dtype=np.uint64).copy()
    dig, err = (C.c_uint64 * 4)(), C.create_string_buffer(256)
    args = dict(params=C.byref(p), roots=roots, lh=lh, nm=nm, ws=ws, pts=pts, st=st, dig=dig)
    for k in nulls:
        args[k] = None
    rc = lib.mh_pcs_verify(lmcs, salt, args["params"], n_trees, args["roots"], args["lh"], args["nm"], args["ws"], n_points, args["pts"],
                           args["st"], None, 0, f.ctypes.data_as(u64p) if f.size else None, f.size, cm.ctypes.data_as(u64p) if cm.size else None,
                           cm.size // 4, None, args["dig"], err, 256)
    return rc, err.value.decode()


def test_verify_refuses_bad_arguments_and_garbage():
    pkg = load_package()
    lib = pkg.load_library()
    for k in ("params", "roots", "lh", "nm", "ws", "pts", "st", "dig"):
        rc, msg = raw_verify(lib, pkg, nulls=(k,))
        assert rc == 1 and "null" in msg, (k, msg)
    for n in (0, 5, -1, 1 << 20):
        rc, msg = raw_verify(lib, pkg, n_points=n)
        assert rc == 1 and "n_points" in msg, (n, msg)
    for n in (0, -3, 257):
        rc, msg = raw_verify(lib, pkg, n_trees=n)
        assert rc == 1 and "trees" in msg, (n, msg)
    assert raw_verify(lib, pkg, lmcs=9)[0] == 1 and "salt_elems" in raw_verify(lib, pkg, salt=9)[1]
    rc, msg = raw_verify(lib, pkg, prm=dict(TOY, log_blowup=0))
    assert rc == 1 and msg
    rc, msg = raw_verify(lib, pkg, heights=(40,))
    assert rc == 1 and "two-adicity" in msg
    w16 = pow(ROOT_2_32, 1 << 28, P)
    rc, msg = raw_verify(lib, pkg, points=[w16, 0] * 8)
    assert rc == 1 and "evaluation point 0" in msg
    # empty streams, then a few hundred seeded random byte strings and their truncations, under three configurations
    rc, msg = raw_verify(lib, pkg)
    assert rc == 1 and "ran out" in msg
    rng = np.random.default_rng(9)
    for i in range(300):
        nf, nc = int(rng.integers(0, 4000)), int(rng.integers(0, 2000))
        f, cm = rng.bytes(nf), rng.bytes(nc)
        if i % 3 == 0:  # canonical felts, so that the reader gets past the first word
            f = (np.frombuffer(rng.bytes(nf // 8 * 8), dtype=np.uint64) % np.uint64(P)).tobytes()
        rc, msg = raw_verify(lib, pkg, n_points=1 + i % 4, fields=f, commitments=cm, lmcs=(0, 1, 2)[i % 3], salt=(0, 0, 4)[i % 3 if i % 2 else 0],
                             prm=dict(TOY, deep_pow_bits=i % 2, folding_pow_bits=0, query_pow_bits=i % 3))
        assert rc == 1 and msg, (i, rc, msg)


# ---- the recorded openings ----
def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def verify_case(pkg, fx, pr, **over):
    a = dict(roots=pr["roots"], points=pr["points"], fields=pr["fields"], commitments=pr["commitments"], pre_observe=pr["pre_observe"])
    a.update(over)
    return pkg.pcs_verify(a["roots"], pr["log_tree_heights"], pr["widths"], a["points"], fx["params"], fx["challenger_state"], a["pre_observe"],
                          np.array(a["fields"], dtype=np.uint64), np.array(a["commitments"], dtype=np.uint64).reshape(-1, 4), lmcs=pr["lmcs"])


def test_recorded_openings_verify_and_tampering_is_refused():
    """Fails without the feature: the symbol does not exist."""
    pkg = load_package()
    fx = load_fixture()
    assert [(p["lmcs"], p["n_points"]) for p in fx["proofs"]] == [("poseidon2", 1), ("poseidon2", 3), ("blake3", 2)]
    assert os.path.getsize(FIXTURE) < 64 << 10
    for pr in fx["proofs"]:
        byte_hash = pr["lmcs"] == "blake3"
        ok, digest, evals = verify_case(pkg, fx, pr)
        assert ok, digest
        assert [int(x) for x in digest] == pr["digest"]
        assert evals.shape == (pr["n_points"], sum(pr["widths"][0]), 2) and evals.tolist() == pr["evals"]
        n, W, rounds, fpl = pr["n_points"], pr["ood_width"], pr["num_fri_rounds"], pr["final_poly_len"]
        off_final = 2 * n * W + 1 + rounds          # evaluations | DEEP witness | one witness per FRI round | final polynomial
        off_hints = off_final + 2 * fpl + 1        # | query witness | hints
        assert off_hints < len(pr["fields"]) and rounds < len(pr["commitments"])

        def bump(v, i):
            v = list(v)
            v[i] = (v[i] + 1) % P
            return v

        tampered = {
            "one evaluation": dict(fields=bump(pr["fields"], 2 * (W - 1) + 1 if W > 1 else 0)),
            "one opened felt": dict(fields=bump(pr["fields"], off_hints)),
            "the last opened felt": dict(fields=bump(pr["fields"], len(pr["fields"]) - 1)),
            "one final-poly coefficient": dict(fields=bump(pr["fields"], off_final + 1)),
            "one point": dict(points=[[(pr["points"][0][0] + 1) % P, pr["points"][0][1]]] + pr["points"][1:]),
            "a wrong root": dict(roots=[bump(pr["roots"][0], 2)]),
            "a wrong root in the transcript": dict(pre_observe=bump(pr["pre_observe"], 0)),
            "trailing data": dict(fields=pr["fields"] + [0]),
            "a truncated stream": dict(fields=pr["fields"][:-1]),
            "a non-canonical felt": dict(fields=pr["fields"][:off_hints] + [pr["fields"][off_hints] + P] + pr["fields"][off_hints + 1:])
            if pr["fields"][off_hints] + P < 1 << 64 else dict(fields=pr["fields"][:off_hints] + [P] + pr["fields"][off_hints + 1:]),
        }
        sib = [list(c) for c in pr["commitments"]]   # the first digest behind the FRI roots is a hinted sibling
        sib[rounds][0] = sib[rounds][0] ^ 1 if byte_hash else (sib[rounds][0] + 1) % P
        tampered["one sibling digest"] = dict(commitments=sib)
        if n >= 2:
            tampered["two points swapped"] = dict(points=[pr["points"][1], pr["points"][0]] + pr["points"][2:])
        for what, over in tampered.items():
            ok, msg, _ = verify_case(pkg, fx, pr, **over)
            assert not ok and isinstance(msg, str) and msg, (pr["lmcs"], n, what)
        # the verifier is deterministic: the untouched proof still verifies
        assert verify_case(pkg, fx, pr)[0]
