"""Corner operands for the compiled constraint kernels' product (csrc/air_jit.cpp, JIT_PRELUDE: gl_mul / lz_mul_asm / lz_mulN).  A helper
module, not a test.

`mul_model` restates the 13 instructions of the asm product over Python integers and returns every carry next to the result.  It is used
ONLY TO CHOOSE INPUTS: the links k2, bw, c3 and mk = bw & ~c3 fire with probability ~2^-32 on uniformly random operands, so a test that
wants them executed has to pick its operands.  Expected values in every test come from `a * b % P` and the EF formulas over Python
integers, never from the model.

`PAIRS` is the table the GPU tests lay out over the rows of their traces (tests/test_gpu_constraint_fold.py, tests/test_gpu_lookup.py);
tests/test_jit_corner_operands.py proves on the CPU that the table, and each layout, reaches every carry."""
import functools

P = 0xFFFFFFFF00000001
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
FLAGS = ("cm", "k1", "k2", "c1", "bb", "bw", "c3", "mk")  # the carries a correct product may set
NEVER = ("d4", "d5")                                       # the carries the asm drops: they must never be set (nor cm & k2)

# tests/test_jit_prelude_arith.py's EDGE list (any-representative values; the canonical ones enter the table)
EDGE = [0, 1, 2, 7, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFE, P - 2, P - 1, P, P + 1, P + 0xFFFFFFFE, M64 - 1, M64, 1 << 63, (1 << 63) - 1,
        0xFFFFFFFF00000000, 0xFFFFFFFEFFFFFFFF, 0x00000000FFFFFFFF, 0xFFFFFFFF, 0x8000000000000000 + 0xFFFFFFFF]


def mul_model(a, b):
    """The 13 steps of gl_mul / lz_mul_asm on u64 operands -> (result: any representative < 2^64, {carry name: 0 / 1})."""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p00 = a0 * b0                                    # v_mad_u64_u32 p00 = a.lo * b.lo
    m = a0 * b1                                      # v_mad_u64_u32 m = a.lo * b.hi
    m += a1 * b0                                     # v_mad_u64_u32 m += a.hi * b.lo, carry cm
    cm, m = m >> 64, m & M64
    w1 = (p00 >> 32) + (m & M32)                     # v_add_co w1 = p00.hi + m.lo, carry k1
    k1, w1 = w1 >> 32, w1 & M32
    accl = (m >> 32) + k1                            # v_addc accl = m.hi + k1, carry k2
    k2, accl = accl >> 32, accl & M32
    acch = cm | k2                                   # v_addc acch = 0 + 0 + (cm | k2)
    hi = a1 * b1 + ((acch << 32) | accl)             # v_mad_u64_u32 hi = a.hi * b.hi + acc (no carry: the product is < 2^128)
    assert hi >> 64 == 0
    lo = (w1 << 32) | (p00 & M32)
    t = (hi & M32) * M32 + lo                        # v_mad_u64_u32 t = hi.lo * (2^32 - 1) + lo, carry c1
    c1, t = t >> 64, t & M64
    rl = (t & M32) - (hi >> 32) - c1                 # v_subb rl = t.lo - hi.hi - c1, borrow bb
    bb, rl = int(rl < 0), rl & M32
    rh = (t >> 32) + c1                              # v_addc rh = t.hi + 0 + c1, carry d4 (dropped)
    d4, rh = rh >> 32, rh & M32
    rh = rh - bb                                     # v_subb rh -= bb, borrow bw
    bw, rh = int(rh < 0), rh & M32
    rl = rl + bw                                     # v_addc rl += bw, carry c3
    c3, rl = rl >> 32, rl & M32
    mk = bw & (1 - c3)
    rh = rh - mk                                     # v_subb rh -= mk, borrow d5 (dropped)
    d5, rh = int(rh < 0), rh & M32
    return (rh << 32) | rl, dict(cm=cm, k1=k1, k2=k2, c1=c1, bb=bb, d4=d4, bw=bw, c3=c3, mk=mk, d5=d5)


def _candidates():
    """Canonical structured values: EDGE, 2^i + d and 2^i +- 2^j + d for d in {-1, 0, 1}."""
    out = {v for v in EDGE if v < P}
    for i in range(65):
        for d in (-1, 0, 1):
            out.add((1 << i) + d)
            for j in range(i):
                out.add((1 << i) + (1 << j) + d)
                out.add((1 << i) - (1 << j) + d)
    return sorted(v for v in out if 0 <= v < P)


def signature(a, b):
    f = mul_model(a, b)[1]
    return tuple(f[k] for k in FLAGS)


# the three pairs the carries k2, bw & mk, bw & c3 were first reached with
SEED_PAIRS = [(0x3ffffffff, 0xfffffffeffffffff), (1 << 63, 1 << 63), (0x200000000, 0x8000000000000000)]


# second operands of the walk below: the heavy values every rare carry pattern was found against
HEAVY = [0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF00000000, P - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 0x80000000FFFFFFFF, 1 << 62, 1 << 61,
         (1 << 56) - 1]


def _select(per_pattern=10, limit=240):
    """The seed pairs and corner x corner, then a fixed walk over (structured value) x HEAVY that keeps, for every distinct pattern of
    carries the model reports, the first `per_pattern` pairs showing it.  Deterministic: the table is the same in every process."""
    corner = [0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF00000000, 1 << 63, (1 << 63) - 1]
    pairs = list(SEED_PAIRS) + [(a, b) for a in corner for b in corner if a <= b]
    seen = {}
    for p in pairs:
        seen[signature(*p)] = seen.get(signature(*p), 0) + 1
    for a in _candidates():
        if a < 4:
            continue
        for b in HEAVY:
            s = signature(a, b)
            if seen.get(s, 0) < per_pattern:
                seen[s] = seen.get(s, 0) + 1
                pairs.append((a, b))
    out, have = [], set()
    for p in pairs:
        if p not in have:
            have.add(p)
            out.append(p)
    assert len(out) <= limit, len(out)
    return out


PAIRS = _select()
assert all(0 <= a < P and 0 <= b < P for a, b in PAIRS)


def coverage(pairs):
    """-> ({flag: number of pairs that set it} incl. 'bw&c3', 'cm&k2', d4, d5)."""
    cnt = {k: 0 for k in FLAGS + NEVER + ("bw&c3", "cm&k2")}
    for a, b in pairs:
        f = mul_model(a, b)[1]
        for k in FLAGS + NEVER:
            cnt[k] += f[k]
        cnt["bw&c3"] += f["bw"] & f["c3"]
        cnt["cm&k2"] += f["cm"] & f["k2"]
    return cnt


def covers(pairs):
    c = coverage(pairs)
    return all(c[k] > 0 for k in FLAGS + ("bw&c3",)) and not any(c[k] for k in NEVER + ("cm&k2",))


@functools.lru_cache(maxsize=None)
def small_cover(count=8):
    """`count` pairs of PAIRS that still reach every carry (greedy; for the 2^3-row traces): the seed pairs first, then whatever adds a
    carry, then filled up from the table in order."""
    out = list(SEED_PAIRS)
    need = lambda ps: [k for k, v in coverage(ps).items() if k in FLAGS + ("bw&c3",) and v == 0]
    for p in PAIRS:
        if not need(out):
            break
        if len(need(out + [p])) < len(need(out)):
            out.append(p)
    for p in PAIRS:
        if len(out) >= count:
            break
        if p not in out:
            out.append(p)
    assert len(out) == count and covers(out)
    return tuple(out)


def column_values(n, shift=0, which=0):
    """Operand `which` (0 = a, 1 = b) of the table laid out over n rows, starting at table entry `shift`: n >= len(PAIRS) shows a gate
    the whole table (cyclically), n = 8 the small cover."""
    src = PAIRS if n >= len(PAIRS) else small_cover(n)
    return [src[(r + shift) % len(src)][which] for r in range(n)]


# values for uniform operands (randomness, aux values, challenges): corner components
CORNER_FELTS = [0, 1, P - 1, (1 << 32) - 1, 1 << 32, 0xFFFFFFFEFFFFFFFF]
