"""The precompile prover's UintStoreMul and UintAdd traces built on the device (run with -m gpu): mh_uint_traces_build
(csrc/uint_traces.hip) against the in-tree generators testing/precompile_trace.uint_store_mul_trace / uint_add_trace cell for cell --
edge moduli, subtractive relations with 0, 1 and 2 moduli borrowed, wave and block boundaries, padding, all four forms of the adder --
every device refusal by section, kind, index and operand next to the generator's assertion on the same list, and sessions whose traces
1 and 2 come from the device through to a byte-equal proof.  Every build is made twice and must leave the same bytes.

The division is a restoring shift-subtract one: it has no digit estimate and hence no correction step to find operands for."""
import ctypes as C
import random
import numpy as np
import pytest
import oracle_binding as ob
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import dag, protocol, precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402
import test_precompile_uint_store_mul as USM  # noqa: E402  (its constructions, imported and not edited)
from uint_traces_cases import (EDGE_BOUNDS, K1, device_defects, edge_ledgers, generator, ledgers, mac, random_ledgers, refusal_ledgers,  # noqa: E402
                               same)

pytestmark = pytest.mark.gpu
P = pkg.P
UNTOUCHED = 0x1234


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


def _vp(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


def build(ctx, rows, muls, adds, log_usm=-1, log_add=-1):
    """mh_uint_traces_build on the ABI's own arguments, TWICE -> (rc, info, usm matrix or None, add matrix or None).  The out pointers of
    a refused call keep the value they had; an accepted call's second run leaves the same bytes."""
    lib = ctx.lib
    lib.mh_uint_traces_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(pkg.UintTracesInfo)]
    outs = []
    for _ in range(2):
        hu, ha, info = C.c_void_p(UNTOUCHED), C.c_void_p(UNTOUCHED), pkg.UintTracesInfo()
        rc = lib.mh_uint_traces_build(ctx.h, _vp(rows), rows.size, _vp(muls), muls.size, _vp(adds), adds.size, log_usm, log_add, C.byref(hu),
                                      C.byref(ha), C.byref(info))
        if rc != 0:
            assert hu.value == UNTOUCHED and ha.value == UNTOUCHED, "a refusal leaves the out pointers alone"
            return rc, info, None, None
        tu = pkg.Trace.from_handle(ctx, hu, int(info.usm_rows).bit_length() - 1, 44)
        ta = pkg.Trace.from_handle(ctx, ha, int(info.add_rows).bit_length() - 1, 30)
        outs.append((tu.download(), ta.download()))
        tu.free()
        ta.free()
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), "a second call leaves the same bytes"
    return 0, info, outs[0][0], outs[0][1]


def check(ctx, store, adds, muls, log_usm=-1, log_add=-1):
    """device == generator, cell for cell, at the least heights or the given ones -> (usm, add, info)"""
    exp_usm, exp_add = generator(store, adds, muls, (1 << log_usm) if log_usm >= 0 else 0, (1 << log_add) if log_add >= 0 else 0)
    rows, m, a = PT.uint_lists(store, adds, muls)
    rc, info, usm, add = build(ctx, rows, m, a, log_usm, log_add)
    assert rc == 0, (rc, info, ctx.lib.mh_last_error(ctx.h).decode())
    same(usm, exp_usm)
    same(add, exp_add)
    assert (info.n_store, info.n_mul, info.n_add, info.usm_rows, info.add_rows, info.defect_kind) == (rows.size, m.size, a.size, usm.shape[0], add.shape[0], 0)
    return usm, add, info


@pytest.mark.parametrize("bound", EDGE_BOUNDS, ids=[f"{b:#x}"[:12] for b in EDGE_BOUNDS])
def test_edge_moduli_one_store_and_seven_relations(ctx, bound):
    """bound + 1 = 2^256 does not fit eight limbs; bound 0 and 1; a modulus with up to 255 leading zero bits.  The six scale cases with
    every operand at the bound (0 - bound borrows one modulus), a seventh relation with every operand 0, and the adder at both ends."""
    store, adds, muls = edge_ledgers(bound)
    assert len(muls.ops) == (7 if bound else 6)  # over the modulus 1 the seventh is the first again
    usm, add, info = check(ctx, store, adds, muls)
    assert (usm.shape[0], add.shape[0]) == (64, 8)
    if bound == (1 << 256) - 1:
        assert int(add[1, PA.UA_CELL_K]) == 1


# ---- the borrow ----
@pytest.mark.parametrize("kappa_a, kappa_c, is_sub, what", USM.MAC_CASES, ids=[c[3] for c in USM.MAC_CASES])
def test_constructions_of_the_multiplier_tests(ctx, kappa_a, kappa_c, is_sub, what):
    """tests/test_precompile_uint_store_mul.py's relations: plain, scaled, kappa_c = 0, a 17-limb quotient, subtractive, two moduli borrowed"""
    rng = random.Random(0x3ac + kappa_a)
    bound = (1 << 256) - 190 if "seventeen" in what else USM.random_modulus(rng)
    ops = [1, 1, bound] if "two moduli" in what else [rng.randrange(bound + 1) for _ in range(3)]
    st = USM.Stack(bound, ops)
    a, b, c = st.ptrs
    st.req._mac(kappa_a, a, b, kappa_c, c, is_sub=is_sub)
    usm, _, _ = check(ctx, st.store, PT.UintAddRequires(), st.muls)
    blk = usm[0:8, PA.USM_MUL_OFF:]
    if "seventeen" in what:
        assert int(blk[PA.UM_ROW_Q, 16]) != 0
    if "two moduli" in what:
        assert int(blk[0, PA.UM_COL_BORROW]) == 2


def test_subtractive_relations_borrow_zero_one_and_two_moduli(ctx):
    rng = random.Random(77)
    bound = USM.random_modulus(rng)
    p_ = bound + 1
    store, adds, muls, fp = ledgers(bound)
    x = rng.randrange(2, p_)
    mac(store, muls, fp, 1, x, x, 1, 5, True)                       # x^2 - 5 >= 0: nothing borrowed
    mac(store, muls, fp, 1, 1, 1, 1, 2, True)                       # 1 - 2: one modulus, remainder p - 1
    mac(store, muls, fp, 1, 0, x, 1, bound, True)                   # 0 - (p - 1): one
    mac(store, muls, fp, 1, 1, 1, 2, bound, True)                   # 1 - 2 (p - 1): two
    mac(store, muls, fp, 0, x, x, 2, bound, True)                   # -2 (p - 1): two
    mac(store, muls, fp, 1, 0, 0, 1, 0, True)                       # 0 - 0: nothing, remainder 0
    mac(store, muls, fp, 3, 1, 1, 3, 1, True)                       # 3 - 3 = 0
    mac(store, muls, fp, 0, 1, 1, 1, 0, True)
    usm, _, _ = check(ctx, store, adds, muls)
    assert [int(usm[8 * i, PA.USM_MUL_OFF + PA.UM_COL_BORROW]) for i in range(8)] == [0, 1, 1, 2, 2, 0, 0, 0]


# ---- wave and block boundaries, heights, padding ----
@pytest.mark.parametrize("n, bound, n_extra, store_taller", [(65, 6, 0, False), (257, None, 0, True), (65, None, 700, True), (3, 6, 0, False)],
                         ids=["65-multiplier-taller", "257", "65-store-taller", "3"])
def test_wave_and_block_boundaries(ctx, n, bound, n_extra, store_taller):
    """65 and 257 relations of each kind (no multiple of a wave or of a block).  Over the modulus 7 the store stays at eight values and
    the multiplier half sets the height; over a large one, or with 700 stored values more, the store does."""
    rng = random.Random(1000 + n + n_extra)
    bound = bound if bound is not None else rng.getrandbits(rng.choice([64, 200, 256])) | 1 << 63
    store, adds, muls = random_ledgers(rng, bound, n, n, n_extra)
    usm, add, info = check(ctx, store, adds, muls)
    mul_rows, store_rows = 1 << (8 * n - 1).bit_length(), 4 << (len(store.rows) - 1).bit_length()
    assert usm.shape[0] == max(mul_rows, store_rows) == info.usm_rows_needed and add.shape[0] == 1 << (2 * n - 1).bit_length() == info.add_rows_needed
    assert (store_rows > mul_rows) == store_taller and (n < 65 or (mul_rows > store_rows) != store_taller)


def test_padding_to_larger_heights_and_refusal_of_smaller_ones(ctx):
    rng = random.Random(5)
    store, adds, muls = random_ledgers(rng, K1, 20, 9)
    usm, add, info = check(ctx, store, adds, muls, log_usm=11, log_add=7)
    n, last = len(store.rows), max(store.rows)
    need = max(256, 4 << (n - 1).bit_length())                                  # 20 relations: 256 multiplier rows; the store: four rows a value
    assert need < 2048 and (info.usm_rows_needed, info.add_rows_needed, usm.shape[0], add.shape[0]) == (need, 32, 2048, 128)
    assert [int(x) for x in usm[4 * n::4, PA.US_COL_PTR]] == list(range(last + 1, last + 1 + 512 - n))      # self-referential padding blocks
    assert (usm[4 * n + 1::4, PA.US_HUB_UINTVAL_MULT] == 1).all() and not usm[8 * 20:, PA.USM_MUL_OFF:].any() and not add[2 * 9:].any()
    rows, m, a = PT.uint_lists(store, adds, muls)
    for lu, la, section, index in ((need.bit_length() - 2, -1, 0, need), (-1, 4, 2, 32), (0, 0, 0, need)):
        rc, info, _, _ = build(ctx, rows, m, a, lu, la)
        assert rc == 1 and (info.defect_section, info.defect_kind, info.defect_index) == (section, 3, index), info
        assert (info.usm_rows_needed, info.add_rows_needed, info.n_store, info.n_mul, info.n_add) == (need, 32, rows.size, 20, 9)
        assert f"section {section}, defect 3, index {index}" in ctx.lib.mh_last_error(ctx.h).decode()


def test_empty_lists(ctx):
    rows, m, a = PT.uint_lists(PT.UintStore())
    rc, info, usm, add = build(ctx, rows, m, a)
    assert rc == 0 and usm.shape == (8, 44) and add.shape == (2, 30) and not add.any()
    assert [int(x) for x in usm[:, PA.US_COL_PTR]] == [int(x) for x in usm[:, PA.US_COL_BOUND_PTR]] == [1, 1, 1, 1, 2, 2, 2, 2]
    assert int(usm[1, PA.US_HUB_UINTVAL_MULT]) == int(usm[5, PA.US_HUB_UINTVAL_MULT]) == 1 and int(usm.sum()) == 2 * (4 * 1 + 4 * 2) + 2
    same(usm, generator(PT.UintStore(), PT.UintAddRequires(), PT.UintMulRequires())[0])


# ---- the adder ----
def test_adder_forms_k_carry_out_and_unreduced_multiplicities(ctx):
    bound = (1 << 256) - 1
    store, adds, muls, fp = ledgers(bound, ptr=7)
    small = store.pin_modulus(9, 10)                                            # a second modulus: 11
    v = lambda x, f=fp: store.intern(x, f)                                      # noqa: E731
    adds.record(v(5), v(6), v(11), fp, P + 5)                                   # k = 0; mult above p
    adds.record(v(bound), v(bound), v(bound - 1), fp, (1 << 64) - 1)            # k = 1 with a sum that carries out of bit 256
    adds.record(v((1 << 255) + 3), v(1 << 255), v(3), fp, P)                    # a + b = 2^256 + 3: only the top carry says k = 1
    adds.record_nz(v(5), v((1 << 224) + (1 << 32)), v(5 + (1 << 224) + (1 << 32)), fp, 2)      # S = 2
    adds.record_nz(v(1), v(bound), v(0), fp, 1)                                 # S = 8 (2^32 - 1)
    adds.record_to_zero(v(3), v(bound - 2), fp, 1)                              # 3 + (-3) = 0, k = 1
    adds.record_to_zero(v(0), v(0), fp, 1)                                      # k = 0
    adds.record_eq(v(77), v(77), fp, 4)
    adds.record(v(7, small), v(9, small), v(5, small), small, 1)                # 16 = 5 + 11
    adds.record(v(10, small), v(10, small), v(9, small), small, 1)
    adds.record(v(4, small), v(6, small), v(10, small), small, 1)               # a + b = the bound exactly: k = 0
    usm, add, _ = check(ctx, store, adds, muls)
    assert [int(add[2 * i + 1, PA.UA_CELL_K]) for i in range(11)] == [0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0]
    assert int(add[1, PA.UA_CELL_MULT]) == 5 and int(add[3, PA.UA_CELL_MULT]) == (1 << 64) - 1 - P and int(add[5, PA.UA_CELL_MULT]) == 0
    assert int(add[6, PA.UA_CELL_W]) == pow(2, P - 2, P) and int(add[6, PA.UA_CELL_WS]) == 1 and int(add[8, PA.UA_CELL_WS]) == 1
    # the reads above p: the external counts are 32-bit, the sums stay below p; all-ones external reads on the modulus row
    rows, m, a = PT.uint_lists(store, adds, muls)
    rows["val_reads"][0], rows["limb_reads"][0] = 0xffffffff, 0xffffffff
    rc, _, usm2, _ = build(ctx, rows, m, a)
    assert rc == 0 and int(usm2[1, PA.US_HUB_UINTVAL_MULT]) == int(usm[1, PA.US_HUB_UINTVAL_MULT]) + 0xffffffff
    assert int(usm2[1, PA.US_HUB_UINTLIMBS_MULT]) == 0xffffffff


# ---- refusals ----
def refused(ctx, store, adds, muls, section, kind, index, operand, asserts):
    """the device refuses by (section, kind, index, operand); the generator raises `asserts` on the same list (None: it has no such
    assertion and lays a trace)"""
    rows, m, a = PT.uint_lists(store, adds, muls)
    rc, info, _, _ = build(ctx, rows, m, a)
    assert rc == 1 and (info.defect_section, info.defect_kind, info.defect_index, info.defect_operand) == (section, kind, index, operand), info
    assert rows.size <= 64 and (info.n_store, info.n_mul, info.n_add, info.usm_rows_needed, info.add_rows_needed) == (rows.size, 8, 8, 256, 16)
    assert f"section {section}, defect {kind}, index {index}, operand {operand}" in ctx.lib.mh_last_error(ctx.h).decode()
    if asserts is None:
        generator(store, adds, muls)
    else:
        with pytest.raises(asserts):
            generator(store, adds, muls)


def test_device_refusals_by_section_kind_index_and_operand(ctx):
    cases = device_defects()
    assert {c[4] for c in cases} == set(range(8, 15))
    for case in cases:
        refused(ctx, *case)
    # the context goes on
    check(ctx, *refusal_ledgers()[:3])


# ---- sessions ----
def test_session_ledgers_give_the_sessions_traces(ctx):
    """uint_arith_session(40) and ec_add_session([0xb5, 77]): the ledgers after the generators have run (own reads subtracted)"""
    _, traces, (_, (store, adds, muls)) = PT.uint_arith_session(40)
    _, traces2, (_, (store2, adds2, muls2, _ec, _ec_add)) = PT.ec_add_session([0xb5, 77])
    for tr, (st, ad, mu) in ((traces, (store, adds, muls)), (traces2, (store2, adds2, muls2))):
        rows, m, a = PT.uint_lists(st, ad, mu, own_reads_recorded=True)
        rc, info, usm, add = build(ctx, rows, m, a, tr[1].shape[0].bit_length() - 1, tr[2].shape[0].bit_length() - 1)
        assert rc == 0, info
        same(usm, tr[1])
        same(add, tr[2])


def host_aux(lookup, main, randomness, preprocessed=None):
    return ob.lookup_build_aux(lookup, main, randomness, preprocessed)


def test_ec_add_session_with_device_built_uint_traces_proves_the_same_bytes(ctx):
    import test_gpu_precompile as GP
    from test_precompile_ec_add import FAST
    pairs, traces, (_, (store, adds, muls, _ec, _ec_add)) = PT.ec_add_session([5], host_aux)
    airs_, lookups = [p[0] for p in pairs], [p[1] for p in pairs]
    rows, m, a = PT.uint_lists(store, adds, muls, own_reads_recorded=True)
    assert [(int(r["ptr"]), int(r["val_reads"]), int(r["limb_reads"])) for r in rows if r["val_reads"] or r["limb_reads"]] == \
        [(ptr, 1, 0) for ptr, _, _ in PA.FIXED_UINTS]
    tu, ta, info = pkg.uint_traces(ctx, rows, m, a, log_usm=traces[1].shape[0].bit_length() - 1, log_add=traces[2].shape[0].bit_length() - 1)
    same(tu.download(), traces[1])
    same(ta.download(), traces[2])
    # the byte-pair table's three columns from zeros, from the pushes of the device-built traces (and the group law's)
    trs = [ctx.upload_trace(t) for t in traces]
    trs[0], trs[1], trs[2] = ctx.upload_trace(np.zeros_like(traces[0])), tu, ta
    rnd = [(0x1234567890abcdef % P, 0x0fedcba987654321), (3141592653589793, 2718281828459045)]
    boundary = [(PA._encode(rnd[0], rnd[1], PA.BUS_EC_GROUP, list(g)), 1) for g in PA.FIXED_EC_GROUPS] + \
               [(PA._encode(rnd[0], rnd[1], PA.BUS_UINT_VAL, [ptr, bp] + PT._limbs(v, 32, 8)), 1) for ptr, bp, v in PA.FIXED_UINTS]
    prep = [airs_[0].preprocessed] + [None] * (len(airs_) - 1)
    w, rep = pkg.fill_multiplicities(ctx, [pkg.DeviceLookup(ctx, lk) for lk in lookups], trs, [(0,) + s for s in PA.BYTE_PAIR_LUT_MULT_SLOTS], rnd,
                                     boundary=boundary, preprocessed=prep)
    assert rep == [] and w == 3 * PA.BPL_TRACE_HEIGHT
    same(trs[0].download(), traces[0])
    # prove with the device-built traces: the bytes of the proof from the uploaded generator traces

    def prove(device_traces):
        dairs = [pkg.DeviceAir(ctx, x) for x in airs_]
        raw = ctx.upload_trace(airs_[0].preprocessed)
        com = pkg.commit_traces(ctx, [raw], FAST["log_blowup"])
        dairs[0].attach_preprocessed(com.tree(), 0, raw=raw)
        for d, lk in zip(dairs, lookups):
            d.attach_lookup(pkg.DeviceLookup(ctx, lk))
        st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
        pre = protocol.protocol_pre_observe(FAST, GP.ROOT, preprocessed_root=com.root())
        return pkg.prove(ctx, dairs, device_traces, GP.ROOT, FAST, st, pre, GP.never), com.root(), st, pre

    got, root, st, pre = prove(trs)
    uploaded, _, _, _ = prove([ctx.upload_trace(t) for t in traces])
    assert bytes(got.bytes) == bytes(uploaded.bytes)
    ok, dig = pkg.verify(airs_, got.log_trace_heights, GP.ROOT, FAST, st, pre, got.fields, got.commitments, preprocessed_root=root,
                         external=PA.external_assertions(pkg, fixed_uints=True))
    assert ok and (dig == got.digest).all()
