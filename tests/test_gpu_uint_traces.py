"""The precompile prover's UintStoreMul and UintAdd traces built on the device (run with -m gpu): mh_uint_traces_build
(csrc/uint_traces.hip) against the in-tree generators testing/precompile_trace.uint_store_mul_trace / uint_add_trace cell for cell --
edge moduli, subtractive relations with 0, 1 and 2 moduli borrowed, wave and block boundaries, padding, all four forms of the adder --
every device refusal by section, kind, index and operand next to the generator's assertion on the same list, and sessions whose traces
1 and 2 come from the device through to a byte-equal proof.  Every build is made twice and must leave the same bytes.

The division is a restoring shift-subtract one: it has no digit estimate and hence no correction step to find operands for."""
import copy
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

pytestmark = pytest.mark.gpu
P = pkg.P
K1 = PA.K1_BOUND
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


def same(got, exp):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert (got == exp).all(), [(int(r), int(c), int(got[r, c]), int(exp[r, c])) for r, c in np.argwhere(got != exp)[:8]]


def generator(store, adds, muls, usm_rows=0, add_rows=0):
    """the two generators on a copy of the store (they record their reads in it) -> (usm, add)"""
    st = copy.deepcopy(store)
    add = PT.uint_add_trace(adds, st, min_height=add_rows)
    return PT.uint_store_mul_trace(st, muls, PT.BytePairLutRequires(), min_height=usm_rows), add


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


def ledgers(bound, ptr=1):
    store, adds, muls = PT.UintStore(), PT.UintAddRequires(), PT.UintMulRequires()
    return store, adds, muls, store.pin_modulus(ptr, bound)


def mac(store, muls, fp, ka, av, bv, kc, cv, sub, mult=1):
    p_ = store.value(fp) + 1
    r = (ka * av * bv + (-1 if sub else 1) * kc * cv) % p_
    muls.record(ka, store.intern(av, fp), store.intern(bv, fp), kc, store.intern(cv, fp), store.intern(r, fp), fp, mult, bool(sub))


def random_ledgers(rng, bound, n_mul, n_add, n_extra=0):
    """`n_mul` multiply-accumulates (half of them subtractive, borrowing 0, 1 or 2 moduli) and `n_add` additions in all four forms over
    one modulus, plus `n_extra` stored values nobody reads"""
    store, adds, muls, fp = ledgers(bound, ptr=rng.randrange(1, 50))
    p_ = bound + 1
    while len(muls.ops) < n_mul:
        ka, kc, sub = rng.choice([0, 1, 2, 255, 1023]), rng.choice([0, 1, 3, 255, 1023]), rng.random() < .5
        av, bv, cv = (rng.choice([0, bound, rng.randrange(p_), rng.randrange(p_) >> rng.randrange(0, 256)]) for _ in range(3))
        if sub and kc:  # the underflow stays within two moduli
            cv = min(cv, (ka * av * bv + rng.choice([0, p_, 2 * p_ - 1])) // kc)
        mac(store, muls, fp, ka, av, bv, kc, cv, sub, rng.getrandbits(64))
    while len(adds.ops) < n_add:
        av, bv = rng.randrange(p_), rng.choice([0, rng.randrange(p_)])
        a, b, c = store.intern(av, fp), store.intern(bv, fp), store.intern((av + bv) % p_, fp)
        form = rng.randrange(4)
        if form == 0 or (form == 1 and bv == 0):
            adds.record(a, b, c, fp, rng.getrandbits(64))
        elif form == 1:
            adds.record_nz(a, b, c, fp, rng.getrandbits(64))
        elif form == 2:
            adds.record_to_zero(a, store.intern(-av % p_, fp), fp, rng.getrandbits(64))
        else:
            adds.record_eq(a, a, fp, rng.getrandbits(64))
    for _ in range(n_extra):
        store.intern(rng.randrange(p_), fp)
    return store, adds, muls


# ---- edge moduli ----
EDGE_BOUNDS = [(1 << 256) - 1, (1 << 256) - 2, 0, 1, 0xffff, (1 << 64) - 1, 1 << 255, K1]
EDGE_CASES = [(1, 1, 0), (1, 1, 1), (255, 255, 0), (255, 255, 1), (1, 0, 0), (0, 1, 1)]


@pytest.mark.parametrize("bound", EDGE_BOUNDS, ids=[f"{b:#x}"[:12] for b in EDGE_BOUNDS])
def test_edge_moduli_one_store_and_seven_relations(ctx, bound):
    """bound + 1 = 2^256 does not fit eight limbs; bound 0 and 1; a modulus with up to 255 leading zero bits.  The six scale cases with
    every operand at the bound (0 - bound borrows one modulus), a seventh relation with every operand 0, and the adder at both ends."""
    store, adds, muls, fp = ledgers(bound)
    for ka, kc, sub in EDGE_CASES:
        mac(store, muls, fp, ka, bound, bound, kc, bound, sub, 3)
    mac(store, muls, fp, 1, 0, 0, 1, 0, 0)
    assert len(muls.ops) == (7 if bound else 6)  # over the modulus 1 the seventh is the first again
    zero, top = store.intern(0, fp), store.intern(bound, fp)
    adds.record(top, top, store.intern((2 * bound) % (bound + 1), fp), fp, 1)   # carries out of bit 256 under 2^256 - 1
    adds.record(zero, zero, zero, fp, 1)
    adds.record_to_zero(zero, zero, fp, 1)
    adds.record_eq(top, top, fp, 1)
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
def refusal_ledgers():
    """a clean list of eight multiply relations and eight additions over secp256k1's field, to be spoiled"""
    rng = random.Random(31)
    store, adds, muls, fp = ledgers(K1)
    p_ = K1 + 1
    for i in range(8):
        mac(store, muls, fp, 1 + i, rng.randrange(p_), rng.randrange(p_), i, rng.randrange(p_), 0)
        av, bv = rng.randrange(p_), rng.randrange(1, p_)
        adds.record(store.intern(av, fp), store.intern(bv, fp), store.intern((av + bv) % p_, fp), fp, 1)
    return store, adds, muls, fp


def spoil_mul(muls, i, **kw):
    (ka, kc, a, b, c, r, bound, sub), mult = muls.ops[i]
    f = dict(kappa_a=ka, kappa_c=kc, a=a, b=b, c=c, r=r, bound=bound, is_sub=sub)
    f.update(kw)
    muls.ops[i] = [(f["kappa_a"], f["kappa_c"], f["a"], f["b"], f["c"], f["r"], f["bound"], f["is_sub"]), mult]


def spoil_add(adds, i, **kw):
    (a, b, c, bound, nz), mult = adds.ops[i]
    f = dict(a=a, b=b, c=c, bound=bound, nz=nz)
    f.update(kw)
    adds.ops[i] = [(f["a"], f["b"], f["c"], f["bound"], f["nz"]), mult]


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
    p_ = K1 + 1
    # 8: a pointer that is not stored -- the lowest index, the first operand of it, the multiply section before the add section
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 5, c=999999)
    spoil_mul(muls, 3, r=888888, bound=777777)
    spoil_add(adds, 0, a=5)
    refused(ctx, store, adds, muls, 1, 8, 3, 3, KeyError)           # the generator has no assertion: its store lookup fails
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 6, bound=424242)
    spoil_add(adds, 2, c=555555)
    spoil_add(adds, 4, b=None, c=None)                              # pointer 0 in b and c is "absent", not a defect of kind 8
    refused(ctx, store, adds, muls, 2, 8, 2, 2, KeyError)
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 7, a=0)                                         # 0 is no pointer of a multiply relation
    refused(ctx, store, adds, muls, 1, 8, 7, 0, KeyError)
    # 9: a kappa >= 2^16; the generator only knows the carry window (13)
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 6, kappa_a=1 << 16)
    spoil_mul(muls, 1, kappa_c=70000)
    spoil_mul(muls, 0, r=muls.ops[1][0][5])                         # a kind 10 at a lower index does not come first
    refused(ctx, store, adds, muls, 1, 9, 1, 1, AssertionError)
    # 10: r is not the canonical remainder
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 6, r=muls.ops[0][0][5])
    spoil_mul(muls, 4, r=muls.ops[0][0][5])
    spoil_add(adds, 1, c=adds.ops[0][0][2])
    refused(ctx, store, adds, muls, 1, 10, 4, 0, AssertionError)
    store, adds, muls, fp = refusal_ledgers()
    big, one = store.pin_modulus(2, (1 << 256) - 1), store.intern(1, fp)         # 1 * 1 = 1 + p: the same residue, not canonical
    spoil_mul(muls, 2, kappa_a=1, kappa_c=0, a=one, b=one, r=store.intern(1 + p_, big))
    refused(ctx, store, adds, muls, 1, 10, 2, 0, AssertionError)
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 5, c=adds.ops[0][0][2])
    spoil_add(adds, 3, c=adds.ops[0][0][2])
    refused(ctx, store, adds, muls, 2, 10, 3, 0, AssertionError)
    # 10 for an addition is stricter than the generator: 25 + 30 = 0 (mod 11) under a foreign bound holds for no k in {0, 1}
    store, adds, muls, fp = refusal_ledgers()
    small = store.pin_modulus(3, 10)
    spoil_add(adds, 7, a=store.intern(25, fp), b=store.intern(30, fp), c=store.intern(0, small), bound=small)
    refused(ctx, store, adds, muls, 2, 10, 7, 0, None)
    # 11: a quotient >= 2^272 (full-size operands over a small foreign modulus)
    store, adds, muls, fp = refusal_ledgers()
    small = store.pin_modulus(3, 10)
    a = store.intern(K1, fp)
    spoil_mul(muls, 5, kappa_a=65535, a=a, b=a, kappa_c=0, r=store.intern(65535 * K1 * K1 % 11, small), bound=small)
    refused(ctx, store, adds, muls, 1, 11, 5, 0, AssertionError)
    # 12: a subtractive underflow beyond two moduli, its r the canonical remainder
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 3, kappa_a=0, kappa_c=3, c=store.intern(K1, fp), r=store.intern(-3 * K1 % p_, fp), is_sub=1)
    spoil_mul(muls, 6, kappa_a=0, kappa_c=3, c=store.intern(K1, fp), r=store.intern(-3 * K1 % p_, fp), is_sub=1)
    refused(ctx, store, adds, muls, 1, 12, 3, 0, AssertionError)
    # 13: kappas of 4095 under a full-size modulus leave the +-2^31 window (1023 does not: test_wave_and_block_boundaries)
    store, adds, muls, fp = refusal_ledgers()
    for i, cv in ((2, K1), (5, K1 - 1)):                            # a = b = the bound: every limb product is large
        spoil_mul(muls, i, kappa_a=4095, kappa_c=4095, a=store.intern(K1, fp), b=store.intern(K1, fp), c=store.intern(cv, fp),
                  r=store.intern((4095 * K1 * K1 + 4095 * cv) % p_, fp))
    refused(ctx, store, adds, muls, 1, 13, 2, 0, AssertionError)
    spoil_add(adds, 0, nz=True, b=store.intern(0, fp), c=adds.ops[0][0][0])      # the lowest kind first: 13 before 14
    refused(ctx, store, adds, muls, 1, 13, 2, 0, AssertionError)
    # 14: nz with b = 0, stored or absent
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 6, nz=True, b=None, c=adds.ops[6][0][0])
    spoil_add(adds, 4, nz=True, b=store.intern(0, fp), c=adds.ops[4][0][0])
    refused(ctx, store, adds, muls, 2, 14, 4, 1, AssertionError)
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
