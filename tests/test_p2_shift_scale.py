"""The power-of-two round scales of the device permutation (poseidon2_fast.cuh: p2f_shl_words / p2f_pm_shl, used by p2f_permute,
poseidon2_lanes.cuh and poseidon2_quad.cuh) on exact integers, no GPU: every scale constant is 2^e, y * 2^e is a signed wide pair
of 32-bit words, and the paired internal rounds built on it equal the plain 22 internal rounds with every wide part inside the
fold's bound (|part| < 2^61)."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
M32 = 2**32 - 1
BOUND = 2**61
src = open(os.path.join(ROOT, "miden-vm_amd/csrc", "p2_constants.inc")).read()
fs = open(os.path.join(ROOT, "miden-vm_amd/csrc", "p2_fast_constants.inc")).read()


def arr(text, name):
    m = re.search(name + r"\[\d+\] = \{(.*?)\};", text, re.S)
    return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1))]


def scalar(name):
    return int(re.search(name + r" = (0x[0-9a-fA-F]+|\d+)", fs).group(1), 0)


DIAG = arr(src, "P2_MAT_DIAG")
ARK = arr(src, "P2_ARK_INT")
GA, GK, FK = arr(fs, "P2G_ARK"), arr(fs, "P2G_K"), arr(fs, "P2F_INT_K")
GK_E, FK_E = arr(fs, "P2G_K_LOG2"), arr(fs, "P2F_INT_K_LOG2")
GD, FD = scalar("P2G_DESCALE"), scalar("P2F_DESCALE")
GD_E, FD_E = scalar("P2G_DESCALE_LOG2"), scalar("P2F_DESCALE_LOG2")

# p2f_shl_sign: sign of word w (u0, u1, u2) in part (0 = L, 1 = H), by q = (e mod 96) / 32
TAB = [[[1, 0, -1], [0, 1, 1]], [[0, -1, -1], [1, 1, 0]], [[-1, -1, 0], [1, 0, -1]]]


def shl_sign(e, part, w):
    sg = TAB[e % 96 // 32][part][w] * (-1 if e >= 96 else 1)
    return 0 if (w == 2 and e % 32 == 0) else sg


def shl_words(y, e):
    b = e % 96 % 32
    z = (y << b) & (2**64 - 1)
    return [z & M32, z >> 32, (y >> 32) >> (32 - b) if b else 0]


def shl_wide(y, e):
    u = shl_words(y, e)
    return [sum(shl_sign(e, part, w) * u[w] for w in range(3)) for part in (0, 1)]


def pm_shl(R, y, e, part):
    """p2f_pm_shl: (8 (R + y 2^e), 8 (R - y 2^e)) of one part, computed the way the device does."""
    u = shl_words(y, e)
    sg = [shl_sign(e, part, w) for w in range(3)]
    if sum(s > 0 for s in sg) >= sum(s < 0 for s in sg):
        s8 = (R + sum(s * x for s, x in zip(sg, u))) << 3
        return s8, (R << 4) - s8
    n = (R - sum(s * x for s, x in zip(sg, u))) << 3
    return (R << 4) - n, n


def rep(v, rng):
    """Some representative < 2^64 of v mod p (the device keeps any such value between products)."""
    v %= P
    return v + P if v + P < 2**64 and rng.random() < 0.5 else v


def check_fold(L, H):
    assert abs(L) < BOUND and abs(H) < BOUND, (L.bit_length(), H.bit_length())
    return (L + H * 2**32) % P


def test_constants_are_powers_of_two():
    assert [pow(2, e, P) for e in GK_E] == GK and [pow(2, e, P) for e in FK_E] == FK
    assert pow(2, GD_E, P) == GD and pow(2, FD_E, P) == FD
    assert all(0 <= e < 192 for e in GK_E + FK_E + [GD_E, FD_E])


def test_shift_scale_identity():
    rng = random.Random(7)
    ys = [0, 1, M32, 2**32, P - 1, P, 2**64 - 1, 2**64 - 2**32, 2**63, 2**63 - 1] + [rng.randrange(2**64) for _ in range(300)]
    ys += [2**64 - 1 - rng.randrange(2**20) for _ in range(50)]
    for e in sorted(set(GK_E + FK_E + [GD_E, FD_E] + list(range(192)))):
        for y in ys:
            L, H = shl_wide(y, e)
            assert abs(L) < 2**33 and abs(H) < 2**33
            assert (L + H * 2**32) % P == y * pow(2, e, P) % P, (e, y)
            for part, R in ((0, rng.randrange(-2**58, 2**58)), (1, rng.randrange(-2**58, 2**58))):
                s8, n = pm_shl(R, y, e, part)
                assert s8 == 8 * (R + (L, H)[part]) and n == 8 * (R - (L, H)[part])


def ref_internal(s):
    s = list(s)
    for r in range(22):
        s[0] = pow((s[0] + ARK[r]) % P, 7, P)
        t = sum(s) % P
        s = [(DIAG[i] * s[i] + t) % P for i in range(12)]
    return s


def halves(v):
    return v & M32, v >> 32


def paired_shift(s, rng):
    """p2f_permute's internal rounds with the scales as shifts: wide parts are exact signed integers, checked at every fold."""
    x = list(s)
    xs = [rep(v, rng) for v in x]
    t0 = (x[0] + GA[0]) % P
    y = rep(pow(t0, 7, P), rng)
    RL = sum(halves(v)[0] for v in xs[1:])
    RH = sum(halves(v)[1] for v in xs[1:])
    s8L, nL = pm_shl(RL << 1, y, GK_E[0], 0)
    s8H, nH = pm_shl(RH << 1, y, GK_E[0], 1)
    t0 = rep(check_fold(nL + (GA[1] & M32), nH + (GA[1] >> 32)), rng)
    h = [halves(v) for v in xs]
    X1 = [16 * h[1][p] + s8 for p, s8 in enumerate((s8L, s8H))]
    X2 = [32 * h[2][p] + s8 for p, s8 in enumerate((s8L, s8H))]
    X11 = [2 * h[11][p] + s8 for p, s8 in enumerate((s8L, s8H))]
    pairs = [(3, 6, 4), (4, 7, 24), (5, 8, 32), (9, 10, 2)]
    A = [[h[i][p] + h[j][p] for p in (0, 1)] for i, j, k in pairs]                      # h(0)
    B = [[k * h[i][p] + s8 - k * h[j][p] for p, s8 in enumerate((s8L, s8H))] for i, j, k in pairs]  # h(1)

    def refold(w):
        return list(halves(rep(check_fold(*w), rng)))

    for r in range(1, 22):
        C, Pv = (B, A) if r % 2 else (A, B)
        y = rep(pow(t0, 7, P), rng)
        R = [2 * sum(c[p] for c in C) + X1[p] + X2[p] + X11[p] for p in (0, 1)]
        (s8L, nL), (s8H, nH) = pm_shl(R[0], y, GK_E[r], 0), pm_shl(R[1], y, GK_E[r], 1)
        rc = GA[r + 1] if r < 21 else 0
        t0 = rep(check_fold(nL + (rc & M32), nH + (rc >> 32)), rng)
        s8 = (s8L, s8H)
        X1 = [8 * X1[p] + s8[p] for p in (0, 1)]
        X2 = [16 * X2[p] + s8[p] for p in (0, 1)]
        X11 = [X11[p] + s8[p] for p in (0, 1)]
        for q, (i, j, k) in enumerate(pairs):
            Pv[q] = [k * k * Pv[q][p] + s8[p] for p in (0, 1)]
        for w in [X1, X2, X11] + A + B:
            assert abs(w[0]) < BOUND and abs(w[1]) < BOUND, r
        if r % 4 == 3:
            X1, X2, X11 = refold(X1), refold(X2), refold(X11)
            A[:] = [refold(w) for w in A]
            B[:] = [refold(w) for w in B]
    # A = h(22), B = h(21)
    out = [0] * 12
    out[0] = t0
    out[1], out[2], out[11] = check_fold(*X1), check_fold(*X2), check_fold(*X11)
    for q, (i, j, k) in enumerate(pairs):
        out[i] = check_fold(A[q][0] + k * B[q][0], A[q][1] + k * B[q][1])
        out[j] = check_fold(A[q][0] - k * B[q][0], A[q][1] - k * B[q][1])
    return [v * GD % P for v in out]


def lanes_shift(s, rng):
    """poseidon2_lanes.cuh / poseidon2_quad.cuh internal rounds (state scaled by 8^r, every element wide), scales as shifts."""
    c8 = [-16, 8, 16, 4, 24, 32, -4, -24, -32, 2, -2, 1]
    xs = [rep(v, rng) for v in s]
    LH = [list(halves(v)) if i else [0, 0] for i, v in enumerate(xs)]
    t0 = rep((s[0] + arr(fs, "P2F_ARK_INT_SCALED")[0]) % P, rng)
    arks = arr(fs, "P2F_ARK_INT_SCALED")
    n = [0, 0]
    for r in range(22):
        y = rep(pow(t0, 7, P), rng)
        Y = shl_wide(y, FK_E[r])
        S = [sum(LH[i][p] for i in range(1, 12)) + Y[p] for p in (0, 1)]
        LH = [[0, 0]] + [[8 * S[p] + c8[i] * LH[i][p] for p in (0, 1)] for i in range(1, 12)]
        n = [8 * S[p] - 16 * Y[p] for p in (0, 1)]
        for w in LH + [n]:
            assert abs(w[0]) < BOUND and abs(w[1]) < BOUND, r
        if r < 21:
            t0 = rep(check_fold(n[0] + (arks[r + 1] & M32), n[1] + (arks[r + 1] >> 32)), rng)
        if r % 4 == 3:
            LH = [[0, 0]] + [list(halves(rep(check_fold(*w), rng))) for w in LH[1:]]
    out = [check_fold(*n)] + [check_fold(*w) for w in LH[1:]]
    return [v * FD % P for v in out]


def test_shift_scaled_rounds_equal_plain_rounds():
    rng = random.Random(11)
    cases = [[0] * 12, [P - 1] * 12, list(range(12)), [M32] * 12] + [[rng.randrange(P) for _ in range(12)] for _ in range(40)]
    for s in cases:
        ref = ref_internal(s)
        assert paired_shift(s, rng) == ref
        assert lanes_shift(s, rng) == ref
