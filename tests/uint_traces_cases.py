"""Ledgers, expectations and defects shared by tests/test_uint_traces_cpu.py (the per-lane bodies run lane by lane on the host) and
tests/test_gpu_uint_traces.py (mh_uint_traces_build on the device): both must give the generators' cells and the same refusals.  Not a
test module."""
import copy
import random
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

K1 = PA.K1_BOUND


def same(got, exp):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert (got == exp).all(), [(int(r), int(c), int(got[r, c]), int(exp[r, c])) for r, c in np.argwhere(got != exp)[:8]]


def generator(store, adds, muls, usm_rows=0, add_rows=0):
    """the two generators on a copy of the store (they record their reads in it) -> (usm, add)"""
    st = copy.deepcopy(store)
    add = PT.uint_add_trace(adds, st, min_height=add_rows)
    return PT.uint_store_mul_trace(st, muls, PT.BytePairLutRequires(), min_height=usm_rows), add


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


def edge_ledgers(bound):
    """The six scale cases with every operand at the bound (0 - bound borrows one modulus), a seventh relation with every operand 0, and
    the adder at both ends -> (store, adds, muls)"""
    store, adds, muls, fp = ledgers(bound)
    for ka, kc, sub in EDGE_CASES:
        mac(store, muls, fp, ka, bound, bound, kc, bound, sub, 3)
    mac(store, muls, fp, 1, 0, 0, 1, 0, 0)
    zero, top = store.intern(0, fp), store.intern(bound, fp)
    adds.record(top, top, store.intern((2 * bound) % (bound + 1), fp), fp, 1)   # carries out of bit 256 under 2^256 - 1
    adds.record(zero, zero, zero, fp, 1)
    adds.record_to_zero(zero, zero, fp, 1)
    adds.record_eq(top, top, fp, 1)
    return store, adds, muls


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


def device_defects():
    """every device kind 8..14 -> [(store, adds, muls, section, kind, index, operand, what the generator raises on the same list; None: it
    has no such assertion and lays a trace)]"""
    p_ = K1 + 1
    out = []

    def case(store, adds, muls, *expect):
        out.append(copy.deepcopy((store, adds, muls)) + expect)
    # 8: a pointer that is not stored -- the lowest index, the first operand of it, the multiply section before the add section
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 5, c=999999)
    spoil_mul(muls, 3, r=888888, bound=777777)
    spoil_add(adds, 0, a=5)
    case(store, adds, muls, 1, 8, 3, 3, KeyError)                   # the generator has no assertion: its store lookup fails
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 6, bound=424242)
    spoil_add(adds, 2, c=555555)
    spoil_add(adds, 4, b=None, c=None)                              # pointer 0 in b and c is "absent", not a defect of kind 8
    case(store, adds, muls, 2, 8, 2, 2, KeyError)
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 7, a=0)                                         # 0 is no pointer of a multiply relation
    case(store, adds, muls, 1, 8, 7, 0, KeyError)
    # 9: a kappa >= 2^16; the generator only knows the carry window (13)
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 6, kappa_a=1 << 16)
    spoil_mul(muls, 1, kappa_c=70000)
    spoil_mul(muls, 0, r=muls.ops[1][0][5])                         # a kind 10 at a lower index does not come first
    case(store, adds, muls, 1, 9, 1, 1, AssertionError)
    # 10: r is not the canonical remainder
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 6, r=muls.ops[0][0][5])
    spoil_mul(muls, 4, r=muls.ops[0][0][5])
    spoil_add(adds, 1, c=adds.ops[0][0][2])
    case(store, adds, muls, 1, 10, 4, 0, AssertionError)
    store, adds, muls, fp = refusal_ledgers()
    big, one = store.pin_modulus(2, (1 << 256) - 1), store.intern(1, fp)         # 1 * 1 = 1 + p: the same residue, not canonical
    spoil_mul(muls, 2, kappa_a=1, kappa_c=0, a=one, b=one, r=store.intern(1 + p_, big))
    case(store, adds, muls, 1, 10, 2, 0, AssertionError)
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 5, c=adds.ops[0][0][2])
    spoil_add(adds, 3, c=adds.ops[0][0][2])
    case(store, adds, muls, 2, 10, 3, 0, AssertionError)
    # 10 for an addition is stricter than the generator: 25 + 30 = 0 (mod 11) under a foreign bound holds for no k in {0, 1}
    store, adds, muls, fp = refusal_ledgers()
    small = store.pin_modulus(3, 10)
    spoil_add(adds, 7, a=store.intern(25, fp), b=store.intern(30, fp), c=store.intern(0, small), bound=small)
    case(store, adds, muls, 2, 10, 7, 0, None)
    # 11: a quotient >= 2^272 (full-size operands over a small foreign modulus)
    store, adds, muls, fp = refusal_ledgers()
    small = store.pin_modulus(3, 10)
    a = store.intern(K1, fp)
    spoil_mul(muls, 5, kappa_a=65535, a=a, b=a, kappa_c=0, r=store.intern(65535 * K1 * K1 % 11, small), bound=small)
    case(store, adds, muls, 1, 11, 5, 0, AssertionError)
    # 12: a subtractive underflow beyond two moduli, its r the canonical remainder
    store, adds, muls, fp = refusal_ledgers()
    spoil_mul(muls, 3, kappa_a=0, kappa_c=3, c=store.intern(K1, fp), r=store.intern(-3 * K1 % p_, fp), is_sub=1)
    spoil_mul(muls, 6, kappa_a=0, kappa_c=3, c=store.intern(K1, fp), r=store.intern(-3 * K1 % p_, fp), is_sub=1)
    case(store, adds, muls, 1, 12, 3, 0, AssertionError)
    # 13: kappas of 4095 under a full-size modulus leave the +-2^31 window (1023 does not: the wave and block boundary ledgers)
    store, adds, muls, fp = refusal_ledgers()
    for i, cv in ((2, K1), (5, K1 - 1)):                            # a = b = the bound: every limb product is large
        spoil_mul(muls, i, kappa_a=4095, kappa_c=4095, a=store.intern(K1, fp), b=store.intern(K1, fp), c=store.intern(cv, fp),
                  r=store.intern((4095 * K1 * K1 + 4095 * cv) % p_, fp))
    case(store, adds, muls, 1, 13, 2, 0, AssertionError)
    spoil_add(adds, 0, nz=True, b=store.intern(0, fp), c=adds.ops[0][0][0])      # the lowest kind first: 13 before 14
    case(store, adds, muls, 1, 13, 2, 0, AssertionError)
    # 14: nz with b = 0, stored or absent
    store, adds, muls, fp = refusal_ledgers()
    spoil_add(adds, 6, nz=True, b=None, c=adds.ops[6][0][0])
    spoil_add(adds, 4, nz=True, b=store.intern(0, fp), c=adds.ops[4][0][0])
    case(store, adds, muls, 2, 14, 4, 1, AssertionError)
    return out
