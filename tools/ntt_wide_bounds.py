"""Worst-case magnitude of every intermediate of the wide register DFT of csrc/ntt.hip (NTT_ASM_BFLY == 2), on exact integers.

A value inside a round is a signed 96-bit integer (three 32-bit words, the top one signed).  Butterflies are plain 96-bit adds and
subtracts; b * 2^S (S = 32 q + r) is the sub-word shift b << r followed by a word move that uses 2^64 = 2^32 - 1 and 2^96 = -1
(mod p); a fold takes a NON-NEGATIVE wide value to a representative below 2^64.  Non-negative because:
  * element 0 of the round gets Z = 2^30 p added once; it reaches every output with coefficient 1 and never passes through a shift,
    so every final fold sees value + Z >= 0;
  * the few operands that must be folded before a shift (FOLD_FWD / FOLD_INV below: the shift would leave 96 bits) get Z added first.
This file tracks an interval [min, max] for every value of the schedule, inputs anywhere in [0, 2^64), for G = 1..4 and both
directions, asserts that everything fits, and prints log2 of the largest magnitude per stage.  `model_round` is the same schedule
on concrete integers (tests/test_ntt_wide_bounds.py checks it against the plain DFT).
Usage: python tools/ntt_wide_bounds.py"""
import math

P = 0xFFFFFFFF00000001
EPS = 2**32 - 1
M32 = 2**32 - 1
WIDE = 2**95            # a wide value v satisfies -WIDE <= v < WIDE
Z = 2**30 * P           # the bias: a multiple of p, ~2^94
W16 = {False: 156, True: 36}  # log2 of w_16 (forward) and of its inverse

# Operands folded before their shift: bit j of entry m = butterfly with twiddle index j = e & (2^m - 1) of stage m.
# (mirrored by NTT_WIDE_FOLD_FWD / NTT_WIDE_FOLD_INV in csrc/ntt.hip)
FOLD_FWD = [0x00, 0x00, 0x00, 0x22]
FOLD_INV = [0x00, 0x02, 0x0C, 0x00]


def exponent(inv, m, e):
    return (W16[inv] * (8 >> m) * (e & ((1 << m) - 1))) % 192


# ---- the schedule on concrete integers ----------------------------------------------------------------------------------------
def check_wide(v):
    assert -WIDE <= v < WIDE, ("wide value out of range", v.bit_length())
    return v


def shl(b, S):
    """b * 2^S mod p as a wide value, 0 < S < 96, the way the kernel forms it."""
    q, r = S >> 5, S & 31
    y = check_wide(b << r)  # y2 = y >> 64 must fit the signed top word
    y0, y1, y2 = y & M32, (y >> 32) & M32, y >> 64
    if q == 0:
        return y
    if q == 1:   # y0 2^32 + y1 2^64 + y2 2^96 = (y1 eps + y0 2^32) - y2: one product (its carry is the top word), one subtraction
        return check_wide(y1 * EPS + (y0 << 32) - y2)
    return check_wide(y0 * EPS - (y1 + (y2 << 32)))  # y0 2^64 + y1 2^96 + y2 2^128


def fold(v):
    """Non-negative wide value -> representative < 2^64: lo + hi * eps, the carry of the product worth eps once more."""
    assert 0 <= v < WIDE, ("fold of a negative or oversized value", v)
    t = (v >> 64) * EPS + (v & (2**64 - 1))
    r = (t & (2**64 - 1)) + (t >> 64) * EPS
    assert r < 2**64
    return r


def model_round(x, G, inv):
    """One wide round on 2^G representatives < 2^64: DIT (forward, bit-reversed in) or DIF (inverse, natural in)."""
    x = list(x)
    assert len(x) == 1 << G and all(0 <= v < 2**64 for v in x)
    x[0] += Z
    masks = FOLD_INV if inv else FOLD_FWD
    for m in (range(G - 1, -1, -1) if inv else range(G)):
        for e in range(1 << G):
            if e & (1 << m):
                continue
            f = e | (1 << m)
            E = exponent(inv, m, e)
            S, j = E % 96, e & ((1 << m) - 1)
            pre = (masks[m] >> j) & 1
            if not inv:
                t = x[f]
                if S:
                    t = shl(fold(t + Z) if pre else t, S)
                s, d = check_wide(x[e] + t), check_wide(x[e] - t)
                x[e], x[f] = (d, s) if E >= 96 else (s, d)
            else:
                s = check_wide(x[e] + x[f])
                d = check_wide(x[f] - x[e] if E >= 96 else x[e] - x[f])
                if S:
                    d = shl(fold(d + Z) if pre else d, S)
                x[e], x[f] = s, d
    return [fold(v) for v in x]


def plain_dft(x, G, inv):
    """The same transform mod p: DIT takes bit-reversed input to natural output, DIF natural to bit-reversed."""
    n = 1 << G
    w = pow(2, W16[inv] * (16 >> G), P)  # w_{2^G}
    rev = [int(format(i, "0%db" % G)[::-1], 2) for i in range(n)]
    nat = list(x) if inv else [x[rev[i]] for i in range(n)]
    y = [sum(nat[j] * pow(w, j * k, P) for j in range(n)) % P for k in range(n)]
    return [y[rev[k]] for k in range(n)] if inv else y


# ---- the same schedule on intervals --------------------------------------------------------------------------------------------
class Iv:
    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def __add__(self, o):
        return Iv(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        return Iv(self.lo - o.hi, self.hi - o.lo)

    def mag(self):
        return max(abs(self.lo), abs(self.hi))

    def wide(self, what):
        assert -WIDE <= self.lo and self.hi < WIDE, (what, math.log2(self.mag()))
        return self


REP = Iv(0, 2**64 - 1)


def iv_shl(b, S, what):
    q, r = S >> 5, S & 31
    y = Iv(b.lo << r, b.hi << r).wide(what + ": b << r")
    y2 = Iv(y.lo >> 64, y.hi >> 64)
    if q == 0:
        return y
    if q == 1:
        return Iv(-y2.hi, M32 * EPS + (M32 << 32) - y2.lo).wide(what)
    return Iv(-M32 - (y2.hi << 32), M32 * EPS - (y2.lo << 32)).wide(what)


def iv_fold(v, what):
    assert 0 <= v.lo and v.hi < WIDE, (what, v.lo, math.log2(v.mag()))
    return REP


def bounds_round(G, inv, report=None):
    x = [Iv(REP.lo, REP.hi) for _ in range(1 << G)]
    x[0] = x[0] + Iv(Z, Z)
    biased = [e == 0 for e in range(1 << G)]  # carries element 0's Z (reported apart: it is not part of the signed words' size)
    masks = FOLD_INV if inv else FOLD_FWD
    name = "inverse" if inv else "forward"
    for m in (range(G - 1, -1, -1) if inv else range(G)):
        worst = 0
        for e in range(1 << G):
            if e & (1 << m):
                continue
            f = e | (1 << m)
            E = exponent(inv, m, e)
            S, j = E % 96, e & ((1 << m) - 1)
            pre = (masks[m] >> j) & 1
            what = "%s G=%d stage %d butterfly (%d, %d)" % (name, G, m, e, f)
            assert not (pre and not S), what + ": fold mask on an unshifted butterfly"
            if not inv:
                t = x[f]
                if S:
                    t = iv_shl(iv_fold(t + Iv(Z, Z), what + " pre-fold") if pre else t, S, what)
                s, d = (x[e] + t).wide(what), (x[e] - t).wide(what)
                x[e], x[f] = (d, s) if E >= 96 else (s, d)
            else:
                s = (x[e] + x[f]).wide(what)
                d = ((x[f] - x[e]) if E >= 96 else (x[e] - x[f])).wide(what)
                if S:
                    d = iv_shl(iv_fold(d + Iv(Z, Z), what + " pre-fold") if pre else d, S, what)
                x[e], x[f] = s, d
            assert not biased[f], what + ": the bias reached a shifted operand"
            biased[f] = biased[e]
            worst = max([worst] + [(v - Iv(Z, Z)).mag() if biased[i] else v.mag() for i, v in ((e, x[e]), (f, x[f]))])
        if report is not None:
            report.append((name, G, m, math.log2(worst)))
    for e, v in enumerate(x):
        iv_fold(v, "%s G=%d output %d" % (name, G, e))
    return x


def check_all(report=None):
    for inv in (False, True):
        for G in (1, 2, 3, 4):
            bounds_round(G, inv, report)


if __name__ == "__main__":
    rep = []
    check_all(rep)
    for name, G, m, lg in rep:
        print("%s G=%d after stage %d: largest |value| (without the bias Z = 2^%.2f) = 2^%.2f" % (name, G, m, math.log2(Z), lg))
    print("every wide value inside [-2^95, 2^95), every fold operand inside [0, 2^95): ok")
