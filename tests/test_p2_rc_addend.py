"""Round constants as product addends (poseidon2_fast.cuh, P2F_RC_ADDEND), on exact integers, no GPU:
  * the generated table P2F_EXT_K holds k = M_E^(-1) rc for the eight S-box layers that stand in front of a linear layer, pre-split
    into 32-bit halves, and P2F_TERM0_K the split constants of terminal round 0;
  * a word-level model of p2f_mulN<.., KA> -- the instruction sequence of the device product with Kl and Kh as the addends of its
    first two mads -- equals (a b + K) mod p, no 64-bit mad overflows and the carries cm and k2 never meet;
  * the restructured schedule (constants before the layers, ark_0 through the last initial layer, the constants of terminal round 0
    as addends of the de-scale products) equals the plain permutation, which is pinned to the stored known-answer vector.
The device code itself is compared with the CPU oracle in tests/test_gpu_p2_tails.py."""
import itertools, json, os, random, re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _arr(text, name):
    m = re.search(name + r"\[\d+\] = \{(.*?)\};", text, re.S)
    return [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]


_src = open(os.path.join(ROOT, "miden-vm_amd/csrc/p2_constants.inc")).read()
_fs = open(os.path.join(ROOT, "miden-vm_amd/csrc/p2_fast_constants.inc")).read()
DIAG, ARK = _arr(_src, "P2_MAT_DIAG"), _arr(_src, "P2_ARK_INT")
ARK_I, ARK_T = _arr(_src, "P2_ARK_EXT_INITIAL"), _arr(_src, "P2_ARK_EXT_TERMINAL")
GA, GK = _arr(_fs, "P2G_ARK"), _arr(_fs, "P2G_K")
GD = int(re.search(r"P2G_DESCALE = (0x[0-9a-f]+)", _fs).group(1), 16)
EXT_K_WORDS, TERM0_WORDS = _arr(_fs, "P2F_EXT_K"), _arr(_fs, "P2F_TERM0_K")
M4 = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
ME = [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for j in range(12)] for i in range(12)]
# the corners of the 32-bit halves used in tests/test_gpu_parity.py, and the largest non-canonical values
CORNERS = [0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 0x7FFFFFFF80000000]
WIDE = CORNERS + [M64, M64 - 1, P, P + 1, 0xFFFFFFFF00000002, 0xFFFFFFFFFFFF0000]


def external(s):
    return [sum(a * b for a, b in zip(row, s)) % P for row in ME]


def joined(words):
    assert len(words) % 2 == 0 and all(w <= M32 for w in words), "every word is one 32-bit half"
    return [words[i] | (words[i + 1] << 32) for i in range(0, len(words), 2)]


EXT_K = [joined(EXT_K_WORDS)[12 * r:12 * (r + 1)] for r in range(8)]
TERM0 = joined(TERM0_WORDS)
RC_ROWS = ([ARK_I[12 * (r + 1):12 * (r + 2)] for r in range(3)] + [[ARK[0]] + [0] * 11] +
           [ARK_T[12 * (r + 1):12 * (r + 2)] for r in range(3)] + [[0] * 12])


def test_table_is_the_preimage_of_the_round_constants():
    assert len(EXT_K_WORDS) == 8 * 12 * 2 and len(TERM0_WORDS) == 24
    for r in range(8):
        assert all(k < P for k in EXT_K[r])
        assert external(EXT_K[r]) == RC_ROWS[r], r
    assert EXT_K[7] == [0] * 12
    assert TERM0 == ARK_T[:12]


def mul_addend_model(a, b, K):
    """p2f_mulN<N, false, true>, one product, instruction by instruction (32-bit halves, carries as 0/1)."""
    a0, a1, b0, b1, Kl, Kh = a & M32, a >> 32, b & M32, b >> 32, K & M32, K >> 32
    p00 = a0 * b0 + Kl
    assert p00 <= M64
    m = a0 * b1 + Kh
    assert m <= M64
    m += a1 * b0
    cm, m = m >> 64, m & M64
    w1 = (p00 >> 32) + (m & M32)
    k1, w1 = w1 >> 32, w1 & M32
    accl = (m >> 32) + k1
    k2, accl = accl >> 32, accl & M32
    assert not (cm and k2), "cm and k2 exclude each other"
    acc = ((cm | k2) << 32) | accl
    hi = a1 * b1 + acc
    assert hi <= M64
    lo = (w1 << 32) | (p00 & M32)
    assert (hi << 64) | lo == a * b + K, "the 128-bit value is exact"
    x2, x3 = hi & M32, hi >> 32
    t = x2 * M32 + lo
    c1, t = t >> 64, t & M64
    v = (t & M32) - x3 - c1
    bb, rl = int(v < 0), v & M32
    v = (t >> 32) + c1
    assert v <= M32, "t.hi + c1 does not carry"
    rh = v
    v = rh - bb
    bw, rh = int(v < 0), v & M32
    v = rl + bw
    c3, rl = v >> 32, v & M32
    v = rh - (bw & (1 - c3))
    assert v >= 0
    return (v << 32) | rl


def test_product_with_addend_word_level():
    rng = random.Random(5)
    ks = [k for k in CORNERS if k < P] + [rng.randrange(P) for _ in range(6)] + [k for row in EXT_K for k in row][:12] + TERM0[:4]
    n = 0
    for a, b in itertools.product(WIDE, WIDE):
        for K in ks:
            r = mul_addend_model(a, b, K)
            assert r <= M64 and r % P == (a * b + K) % P, (hex(a), hex(b), hex(K))
            n += 1
    for _ in range(20000):
        a, b = (rng.choice(WIDE) if rng.random() < .3 else rng.randrange(1 << 64) for _ in range(2))
        K = rng.choice(ks) if rng.random() < .3 else rng.randrange(P)
        assert mul_addend_model(a, b, K) % P == (a * b + K) % P
    assert n == len(WIDE) ** 2 * len(ks)
    # the plain product is the K = 0 case of the same sequence
    assert mul_addend_model(M64, M64, 0) % P == M64 * M64 % P


def plain_permutation(s):
    s = external([x % P for x in s])
    for r in range(4):
        s = external([pow((s[i] + ARK_I[12 * r + i]) % P, 7, P) for i in range(12)])
    for r in range(22):
        s[0] = pow((s[0] + ARK[r]) % P, 7, P)
        t = sum(s) % P
        s = [(DIAG[i] * s[i] + t) % P for i in range(12)]
    for r in range(4):
        s = external([pow((s[i] + ARK_T[12 * r + i]) % P, 7, P) for i in range(12)])
    return s


def paired_internal(x, ark0_included, descale_addends):
    """The model of tests/test_p2_fast_schedule.py (paired internal rounds on integers) with the two changes of the new schedule: ark_0
    is already in element 0 (it came through the last initial layer), and the de-scale products add a constant each."""
    x = list(x)
    t0 = x[0] % P if ark0_included else (x[0] + GA[0]) % P
    y = GK[0] * pow(t0, 7, P) % P
    s8 = 8 * (2 * sum(x[1:]) + y)
    t0 = (s8 - 16 * y + GA[1]) % P
    X1, X2, X11 = 16 * x[1] + s8, 32 * x[2] + s8, 2 * x[11] + s8
    pairs = [(3, 6, 4), (4, 7, 24), (5, 8, 32), (9, 10, 2)]
    prv = [x[i] + x[j] for i, j, k in pairs]
    cur = [k * (x[i] - x[j]) + s8 for i, j, k in pairs]
    for r in range(1, 22):
        y = GK[r] * pow(t0, 7, P) % P
        s8 = 8 * (2 * sum(cur) + X1 + X2 + X11 + y)
        t0 = (s8 - 16 * y + (GA[r + 1] if r < 21 else 0)) % P
        X1, X2, X11 = 8 * X1 + s8, 16 * X2 + s8, X11 + s8
        for q, (i, j, k) in enumerate(pairs):
            prv[q] = k * k * prv[q] + s8
        cur, prv = prv, cur
    out = [0] * 12
    out[0], out[1], out[2], out[11] = t0, X1, X2, X11
    for q, (i, j, k) in enumerate(pairs):
        out[i], out[j] = cur[q] + k * prv[q], cur[q] - k * prv[q]
    return [(v * GD + descale_addends[i]) % P for i, v in enumerate(out)]


def restructured_permutation(s):
    """p2f_body + p2f_tail<P2F_ALL> with P2F_RC_ADDEND: every S-box layer is x^7 + k followed by a constant-free linear layer."""
    s = [(v + c) % P for v, c in zip(external([x % P for x in s]), ARK_I[:12])]  # the initial layer keeps its additions
    for r in range(4):
        s = external([(pow(x, 7, P) + k) % P for x, k in zip(s, EXT_K[r])])
    s = paired_internal(s, True, TERM0)
    for r in range(4):
        s = external([(pow(x, 7, P) + k) % P for x, k in zip(s, EXT_K[4 + r])])
    return s


def test_plain_model_matches_known_answer():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))["permutation_kat"]
    assert plain_permutation(kat["input"]) == kat["output"]


def test_restructured_schedule_equals_plain_permutation():
    rng = random.Random(9)
    cases = [[0] * 12, [P - 1] * 12, [M64] * 12, list(range(12))]
    cases += [[rng.choice(WIDE) for _ in range(12)] for _ in range(40)]
    cases += [[rng.randrange(P) for _ in range(12)] for _ in range(40)]
    for s in cases:
        assert restructured_permutation(s) == plain_permutation(s)
