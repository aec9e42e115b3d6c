"""CPU-only: the hiding LMCS's ABI (include/midenhip.h mh_ctx_set_salt and friends) agrees across the header, the Rust declarations
and the Python layer, and mh_verify_hiding -- host code -- handles salt widths out of range and streams cut inside a salt row, and
is mh_verify_lmcs when the salt is off."""
import os, re
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
from __graft_entry__ import load_package, ROOT

FUNCS = ["mh_ctx_set_salt", "mh_ctx_get_salt", "mh_tree_salt_elems", "mh_tree_salt_index", "mh_tree_download_salt", "mh_verify_hiding"]
SMALL = dict(log_blowup=2, log_folding_arity=1, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=1, num_queries=6, query_pow_bits=2)


def test_symbols_in_header_rust_and_exports():
    pkg = load_package()
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midenhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    lib = pkg.load_library()
    for f in FUNCS:
        assert re.search(r"\b(int|uint64_t)\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS and hasattr(lib, f), f
    assert int(re.search(r"#define\s+MH_MAX_SALT_ELEMS\s+(\d+)", h).group(1)) == 8 == pkg.MH_MAX_SALT_ELEMS
    assert int(re.search(r"pub const MH_MAX_SALT_ELEMS: c_int = (\d+);", rs).group(1)) == 8
    # mh_verify_hiding = (lmcs, salt_elems, then exactly mh_verify_lmcs's arguments), in C and in Rust
    def params(src, name, open_, close):
        body = re.search(name + r"\s*\((.*?)\)\s*" + close, src, flags=re.S).group(1)
        return [re.sub(r"\s+", " ", p).strip() for p in body.split(",")]
    c_l, c_h = params(h, "mh_verify_lmcs", "(", ";"), params(h, "mh_verify_hiding", "(", ";")
    assert c_h[:2] == ["int lmcs", "int salt_elems"] and c_h[2:] == c_l[1:]
    r_l, r_h = params(rs, "pub fn mh_verify_lmcs", "(", "->"), params(rs, "pub fn mh_verify_hiding", "(", "->")
    assert r_h[:2] == ["lmcs: c_int", "salt_elems: c_int"] and r_h[2:] == r_l[1:]
    # the header says what the feature is not
    full = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    assert "NOT zero-knowledge" in full and "getrandom" in full and re.search(r"FRESH\s+for every proof", full)


@pytest.fixture(scope="module")
def proof():
    t, pub = A.fib_trace(6)
    airs_ = [A.fib_air()]
    p = ob.prove(airs_, [t], pub, SMALL)
    return airs_, pub, p


def test_salt_off_is_mh_verify_lmcs(proof):
    """An unsalted proof of the CPU checker: mh_verify_hiding(salt_elems = 0) and mh_verify_lmcs give the same answers, digests and
    messages, on the proof and on tampered copies; with any salt on, the same proof is refused (its leaves carry no salt)."""
    import ctypes as C
    pkg = load_package()
    lib = pkg.load_library()
    airs_, pub, p = proof
    lhs = p["log_heights"]
    u64p = C.POINTER(C.c_uint64)
    blob = np.ascontiguousarray(airs_[0].blob, dtype=np.uint64)
    bp, bl = (u64p * 1)(blob.ctypes.data_as(u64p)), (C.c_size_t * 1)(blob.size)
    lh = (C.c_uint8 * 1)(*lhs)
    pv = np.asarray(pub, dtype=np.uint64)
    st = np.asarray(ob.challenger_state(), dtype=np.uint64)
    pre = np.asarray(ob.protocol_pre_observe(SMALL, pub), dtype=np.uint64)
    prm = pkg.PcsParams.from_dict(SMALL)
    cm = np.ascontiguousarray(p["commitments"], dtype=np.uint64).reshape(-1)

    def tail(f):
        dig, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(256)
        return (dig, err, (C.byref(prm), 1, bp, bl, lh, pv.ctypes.data_as(u64p), C.c_size_t(pv.size), st.ctypes.data_as(u64p), pre.ctypes.data_as(u64p),
                           C.c_size_t(pre.size), f.ctypes.data_as(u64p), C.c_size_t(f.size), cm.ctypes.data_as(u64p), C.c_size_t(cm.size // 4), None,
                           None, None, dig.ctypes.data_as(u64p), err, C.c_size_t(256)))

    def hiding(f, salt, lmcs=0):
        dig, err, args = tail(f)
        return lib.mh_verify_hiding(C.c_int(lmcs), C.c_int(salt), *args), dig, err.value.decode()

    def plain(f, lmcs=0):
        dig, err, args = tail(f)
        return lib.mh_verify_lmcs(C.c_int(lmcs), *args), dig, err.value.decode()

    good = np.ascontiguousarray(p["fields"], dtype=np.uint64)
    rc, dig, msg = hiding(good, 0)
    assert rc == 0 and (dig == p["digest"]).all(), msg
    rng = np.random.default_rng(2)
    for f in [good, good[:-1].copy(), good[:good.size // 2].copy()] + [np.where(np.arange(good.size) == k, (good + np.uint64(1)) % np.uint64(ob.P), good)
                                                                     for k in rng.integers(0, good.size, 6)]:
        f = np.ascontiguousarray(f, dtype=np.uint64)
        a, b = hiding(f, 0), plain(f)
        assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2]
    assert hiding(good, 0, lmcs=1)[0] == plain(good, lmcs=1)[0] != 0    # another configuration: both refuse
    for salt in (1, 4, 8):
        rc, _, msg = hiding(good, salt)
        assert rc != 0 and msg
    # salt widths outside 0 .. MH_MAX_SALT_ELEMS: a code and a message, nothing is read
    for salt in (-1, 9, 1 << 20, -(1 << 31)):
        rc, _, msg = hiding(good, salt)
        assert rc != 0 and "salt_elems" in msg, (salt, msg)
    assert hiding(good, 0, lmcs=7)[0] != 0


def test_streams_cut_inside_a_salt_row(proof):
    """A fields vector that ends inside the first opened leaf's salt row (and at every length around it) is refused with a message: the
    unsalted proof read with salt 4 takes the next leaf's row for salt, so cutting it anywhere behind the transcript part exercises
    every position of the reader inside `rows + salt`."""
    pkg = load_package()
    airs_, pub, p = proof
    lhs = p["log_heights"]
    pre = ob.protocol_pre_observe(SMALL, pub)
    n = p["fields"].size
    # the first main-trace leaf's hints start behind the transcript part; walk back from the end over all hint lengths in steps, and
    # every single length across the first leaf's rows + salt (main width 2 -> 8 aligned, + 4)
    import proof_parser as PP
    t_felts = PP.parse(airs_, lhs, pub, SMALL, p["fields"], p["commitments"])["sizes"]["transcript_felts"]
    for cut in list(range(t_felts, t_felts + 14)) + list(range(t_felts + 14, n, 37)) + [n]:
        ok, msg = pkg.verify(airs_, lhs, pub, SMALL, ob.challenger_state(), pre, p["fields"][:cut], p["commitments"], salt_elems=4)
        assert not ok and isinstance(msg, str) and msg, cut
    ok, msg = pkg.verify(airs_, lhs, pub, SMALL, ob.challenger_state(), pre, p["fields"][:t_felts + 10], p["commitments"], salt_elems=4)
    assert "ran out of field elements" in msg  # 8 row felts read, the stream ends 2 felts into the salt
