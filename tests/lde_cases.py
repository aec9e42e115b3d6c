"""Inputs and shapes for the coset LDE tests (csrc/ntt.hip).  A helper module, not a test; tests/test_lde_cases.py holds it to its word on
the CPU, tests/test_gpu_lde_plans.py and tests/lde_child.py run what it describes on the device.

Patterns: `patterns(log_n, w)` names the seeded [2^log_n, w] matrices the narrow cases run -- corners from tests/corner_felts.py
everywhere, mixed, mixed with uniform rows (the control), single non-zero entries in the first and the last 16-point block of a column, and
two columns whose coefficient vectors sit on few indices (so that a wrong twiddle index is not averaged away).

Wide matrices: the LDE acts column by column, so `tiled` builds an [n, width] matrix out of at most 16 distinct columns and returns the
index map; the expected LDE is the oracle's LDE of the distinct columns gathered by the same map -- a 256-column case costs the oracle
16 columns.

The dispatch: `plan_passes`, `pass_rounds`, `coset_loop` and the predicates restate, in Python, how csrc/ntt.hip picks tile, passes,
rounds, scale tables and first-round forms for a shape.  Like corner_felts.deep_accumulators they are used ONLY TO DESCRIBE INPUTS -- which
paths a chosen shape reaches (`tags`) -- never for an expected value.  `SOURCE_CONSTANTS` ties every threshold restated here to the line
of ntt.hip it mirrors: when one moves, tests/test_lde_cases.py fails and the shapes below have to be looked at again."""
import re

import numpy as np

from corner_felts import CORNERS, HEAVY, P, mixture, quarter_random, same

# ---- patterns -------------------------------------------------------------------------------------------------------------------------
SINGLE_VALUES = (P - 1, 2**32, 2**64 - 2**32, 1)   # tests/test_gpu_ntt_wide.py's, by position % 4


def alternating(shape):
    """p-1 on the even rows, 0 on the odd ones; every odd column the other way round.  x = (p-1)/2 * (1 + (-1)^r): coefficients 0 and n/2."""
    out = np.zeros(shape, dtype=np.uint64)
    out[0::2, 0::2] = P - 1
    out[1::2, 1::2] = P - 1
    return out


def first_half(shape):
    """p-1 on the first half of the rows, 0 on the second; every odd column the other way round.  Coefficient 0 and the odd indices."""
    out = np.zeros(shape, dtype=np.uint64)
    h = shape[0] // 2
    out[:h, 0::2] = P - 1
    out[h:, 1::2] = P - 1
    return out


def singles(log_n, w):
    """Matrices with one non-zero entry per column: position 0..15 of the first 16-row block of the column, and of its last one -- 32
    (position, block) slots dealt over the columns of as many matrices as it takes."""
    n = 1 << log_n
    slots = [(pos, blk) for pos in range(16) for blk in (0, 1)]
    out = []
    for k in range(0, len(slots), w):
        m = np.zeros((n, w), dtype=np.uint64)
        for c, (pos, blk) in enumerate(slots[k:k + w]):
            m[(pos if blk == 0 else n - 16 + pos) % n, c] = SINGLE_VALUES[pos % 4]
        out.append(("single%d" % (k // w), m))
    return out


LIGHT = ("mix", "same:p-1", "alt", "half", "control")   # what the heights above 2^16 run: there the oracle is the cost


def patterns(log_n, w, seed=0, only=None):
    """[(name, uint64[2^log_n, w])], seeded by (log_n, w, seed): the same arrays in every process.  only: the names wanted (all when None;
    "single" stands for all the single-entry matrices) -- nothing else is built."""
    shape = (1 << log_n, w)
    s = 100000 * seed + 100 * log_n + w
    makers = [("same:p-1", lambda: same(shape, P - 1)), ("same:heavy", lambda: same(shape, HEAVY)), ("mix", lambda: mixture(shape, 5000 + s)),
              ("control", lambda: quarter_random(shape, 6000 + s)), ("alt", lambda: alternating(shape)), ("half", lambda: first_half(shape))]
    out = [(name, make()) for name, make in makers if only is None or name in only]
    return out + (singles(log_n, w) if only is None or "single" in only else [])


def distinct_columns(log_n, k, seed=0):
    """uint64[2^log_n, k], k <= 16: one column of each kind first (mixture, p-1, alternating, half, control, HEAVY, a single entry in the
    first block, one in the last), then further mixtures and controls"""
    assert 1 <= k <= 16
    n = 1 << log_n
    s = 100000 * seed + 100 * log_n
    first, last = np.zeros((n, 1), dtype=np.uint64), np.zeros((n, 1), dtype=np.uint64)
    first[5 % n, 0], last[n - 16 + 10 if n >= 16 else n - 1, 0] = SINGLE_VALUES[1], SINGLE_VALUES[2]
    cols = [mixture((n, 1), 7000 + s), same((n, 1), P - 1), alternating((n, 1)), first_half((n, 1)), quarter_random((n, 1), 7100 + s),
            same((n, 1), HEAVY), first, last]
    for j in range(4):
        cols += [mixture((n, 1), 7200 + s + j), quarter_random((n, 1), 7300 + s + j)]
    return np.ascontiguousarray(np.hstack(cols[:k]))


def tiled(columns, width, seed):
    """(uint64[n, width], index map[width]): column c of the matrix is columns[:, map[c]]; a seeded choice that uses every distinct column"""
    k = columns.shape[1]
    assert 1 <= k <= 16 and width >= k
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, width - k)])
    rng.shuffle(idx)
    return np.ascontiguousarray(columns[:, idx]), idx


def tiled_case(log_n, width, seed=0, distinct=16):
    """the tiled corner matrix of a wide case: (distinct columns, matrix, index map)"""
    cols = distinct_columns(log_n, min(distinct, width, 16), seed)
    m, idx = tiled(cols, width, 9000 + 100 * log_n + width + seed)
    return cols, m, idx


def non_canonical(log_n, w, seed=0):
    """uint64[2^log_n, w] with entries in [p, 2^64) next to corners, three in four of them >= p: 2^64 - 1 (= p + 0xFFFFFFFE, the largest
    second representative: p + 0xFFFFFFFF is 2^64 and has no 64-bit form), p, p + 1, p + 0xFFFFFFFD, 2^64 - 2^31 and seeded others"""
    n = 1 << log_n
    rng = np.random.default_rng(8000 + 100 * log_n + w + seed)
    fixed = np.array([2**64 - 1, P, P + 0xFFFFFFFD, P + 1, 2**64 - 2**31], dtype=np.uint64)
    out = CORNERS[rng.integers(0, len(CORNERS), (n, w))]
    hi = np.uint64(P) + rng.integers(0, 2**32 - 1, (n, w), dtype=np.uint64)
    pick = rng.integers(0, 4, (n, w))
    out = np.where(pick == 1, hi, out)
    out = np.where(pick >= 2, fixed[rng.integers(0, len(fixed), (n, w))], out)
    out.reshape(-1)[:len(fixed)] = fixed
    return np.ascontiguousarray(out.astype(np.uint64))


def reduce_mod_p(m):
    """the canonical representative of every entry (values < 2^64 < 2 p: one conditional subtraction)"""
    m = np.asarray(m, dtype=np.uint64)
    return np.where(m >= np.uint64(P), m - np.uint64(P), m)


# ---- the dispatch of csrc/ntt.hip, as a description of inputs -------------------------------------------------------------------------
NTT_TILE_LOG, NTT_TILE_LOG_BIG = 12, 14
SMALL_TILE_MAX, BIG_MAX = 20, 22      # ntt_tile_log: the 2^14 tile for SMALL_TILE_MAX < log_n <= BIG_MAX
SEGMENT_BITS = 4                      # plan_passes: max_r = T - 4
FILL_WORKGROUPS = 4096                # launch_pass: cosets go to grid.z while tiles * n_cols * zsplit < 4096
FULL_MIN_COLS, FULL_MIN_LOG, FULL_MAX_LOG = 16, 12, 24   # ntt_forward_cosets: the [z][pos] scale table
DIF_DIRECT_MIN_R = 4                  # ntt_inverse_dif: a.r_bits >= 4 && a.r_bits + a.cb == NTT_TILE_LOG
DIT_DIRECT = (4, 8, 4)                # ntt_forward_cosets: i > 0 && a.cb == 4 && a.r_bits >= 8 && a.r_bits % 4 == 0 && (the same sum)


def ntt_tile_log(log_n):
    return NTT_TILE_LOG_BIG if SMALL_TILE_MAX < log_n <= BIG_MAX else NTT_TILE_LOG


def plan_passes(log_n):
    """[(s_lo, r_bits, cb)]: one contiguous pass over the low stages, then balanced strided passes"""
    T = ntt_tile_log(log_n)
    c = min(log_n, T)
    plan, rem = [(0, c, 0)], log_n - c
    if rem > 0:
        max_r = T - SEGMENT_BITS
        n_passes = (rem + max_r - 1) // max_r
        s = c
        for i in range(n_passes):
            r = rem // n_passes + (1 if i < rem % n_passes else 0)
            plan.append((s, r, T - r))
            s += r
    return plan


def pass_rounds(r_bits):
    """[(first local stage, stages)] in ascending stage order: the remainder r_bits % 4 first, then radix-16 rounds"""
    rem, out = r_bits & 3, []
    if rem:
        out.append((0, rem))
    out += [(st, 4) for st in range(rem, r_bits, 4)]
    return out


def cosets_per_workgroup(tiles, n_cols, n_z):
    """launch_pass: a.n_z, the cosets one workgroup walks"""
    zsplit = 1
    while zsplit < n_z and tiles * n_cols * zsplit < FILL_WORKGROUPS:
        zsplit *= 2
    return n_z // zsplit


def coef_rot(log_n):
    return log_n >= NTT_TILE_LOG and ntt_tile_log(log_n) == NTT_TILE_LOG


def scale_full(log_n, n_cols):
    return n_cols >= FULL_MIN_COLS and FULL_MIN_LOG <= log_n <= FULL_MAX_LOG


def dif_direct(r_bits, cb):
    return r_bits >= DIF_DIRECT_MIN_R and r_bits + cb == NTT_TILE_LOG


def dit_direct(i, r_bits, cb):
    return i > 0 and cb == DIT_DIRECT[0] and r_bits >= DIT_DIRECT[1] and r_bits % DIT_DIRECT[2] == 0 and r_bits + cb == NTT_TILE_LOG


def coset_loop(log_n, width, added_bits):
    """a.n_z of every forward pass of the default path (the later passes walk the cosets too when there is more than one)"""
    out = []
    for s_lo, r, cb in plan_passes(log_n):
        out.append(cosets_per_workgroup(1 << (log_n - r - cb), width, 1 << added_bits))
    return out


def tags(log_n, width, added_bits):
    """The paths of csrc/ntt.hip the LDE of a [2^log_n, width] matrix by 2^added_bits takes.  "dif_direct" / "dit_direct" speak of the
    STRIDED passes (the contiguous pass of the inverse transform loads directly at every log_n >= 12)."""
    plan = plan_passes(log_n)
    T = ntt_tile_log(log_n)
    out = set()
    if plan[0][1] == T:
        out.add("full_tile")
    if coef_rot(log_n):
        out.add("rot")
    out.add("scale_full" if scale_full(log_n, width) else "two_level")
    for i, (s_lo, r, cb) in enumerate(plan):
        if i == 0:
            continue
        out.add("strided:r=%d" % r)
        out.add("rounds:" + ",".join(str(g) for _, g in pass_rounds(r)))
        if dif_direct(r, cb):
            out.add("dif_direct")
        if dit_direct(i, r, cb):
            out.add("dit_direct")
    out.update("n_z=%d" % k for k in coset_loop(log_n, width, added_bits))
    if T == NTT_TILE_LOG_BIG:
        out.add("big_tile")
    if len(plan) == 3:
        out.add("three_pass")
    return out


# every tag the shapes below have to reach between them
REQUIRED_TAGS = ({"full_tile", "rot", "scale_full", "two_level", "dif_direct", "dit_direct", "n_z=1", "n_z=2", "big_tile", "three_pass"}
                 | {"strided:r=%d" % r for r in range(2, 9)}
                 | {"rounds:2", "rounds:3", "rounds:4", "rounds:1,4", "rounds:2,4", "rounds:3,4", "rounds:4,4"})

# ---- the shapes of tests/test_gpu_lde_plans.py: (log_n, width, added_bits) -------------------------------------------------------------
NARROW = [(14, 2, 1), (15, 2, 1), (16, 2, 1), (16, 2, 3), (17, 2, 1), (18, 2, 1), (19, 2, 1), (20, 2, 1)]
ALL_PATTERNS_MAX_LOG = 16             # every pattern up to here, LIGHT above
WIDE = [(12, 16, 1), (12, 17, 3), (13, 33, 1), (16, 16, 3), (20, 16, 1)]
WIDE_BELOW = [(12, 15, 1), (11, 16, 1)]   # the neighbours just below the thresholds: the two-level tables
WIDE_DISTINCT = {20: 4}               # distinct columns of a tiled case by log_n (16 unless named): at 2^20 the oracle is the cost
COSET_LOOP = (14, 256, 3)
BIG = [(21, 1, 1), (23, 1, 1)]
COLUMN_GROUPS = [(12, 19, 3), (16, 19, 1)]   # (log_n, width, log_blowup): 19 = 8 + 8 + 3
SWITCH_CASES = [("tiled", 12, 16, 1), ("corners", 13, 3, 3), ("tiled", 16, 16, 3), ("mix", 20, 2, 1), ("tiled", 14, 256, 3)]
SWITCH_DISTINCT = {16: 8}


def shape_table():
    """every (log_n, width, added_bits) of items 1-4"""
    return NARROW + WIDE + WIDE_BELOW + [COSET_LOOP] + BIG


def switch_input(kind, log_n, width, added_bits):
    """(distinct columns the oracle extends, matrix the device extends, index map) of one case of the switch children"""
    if kind == "tiled":
        return tiled_case(log_n, width, distinct=SWITCH_DISTINCT.get(log_n, 16))
    name = {"corners": "mix", "mix": "mix"}[kind]
    m = dict(patterns(log_n, width, only=(name,)))[name]
    return m, m, np.arange(width)


# ---- the lines of csrc/ntt.hip the constants above mirror ------------------------------------------------------------------------------
SOURCE_CONSTANTS = [
    ("NTT_TILE_LOG", r"static constexpr int NTT_TILE_LOG = (\d+);", (NTT_TILE_LOG,)),
    ("NTT_TILE_LOG_BIG", r"static constexpr int NTT_TILE_LOG_BIG = (\d+);", (NTT_TILE_LOG_BIG,)),
    ("NTT_THREADS", r"static constexpr int NTT_THREADS = (\d+);", (256,)),
    ("NTT_SWZ", r"#ifndef NTT_SWZ\n#define NTT_SWZ (\d+)", (1,)),
    ("big_max", r"getenv\(\"MH_NTT_BIG_MAX\"\);[^\n]*\n\s*return e \? atoi\(e\) : (\d+);", (BIG_MAX,)),
    ("ntt_tile_log", r"return log_n > (\d+) && log_n <= big_max \? NTT_TILE_LOG_BIG : NTT_TILE_LOG;", (SMALL_TILE_MAX,)),
    ("rot", r"return on && log_n >= NTT_TILE_LOG && ntt_tile_log\(log_n\) == (NTT_TILE_LOG);", ("NTT_TILE_LOG",)),
    ("max_r", r"const int max_r = T - (\d+);", (SEGMENT_BITS,)),
    ("balanced passes", r"int np = \(rem \+ max_r - 1\) / max_r;\s*int s = c;\s*for \(int i = 0; i < np; i\+\+\) \{\s*"
                        r"int r = rem / np \+ \(i < rem % np \? 1 : 0\);\s*p\.push_back\(\{s, r, T - r\}\);", ()),
    ("pass_rounds", r"const int rem = r_bits & (\d+);\s*int st = 0;\s*if \(rem\) \{\s*r\.push_back\(\{0, rem\}\);\s*st = rem;\s*\}\s*"
                    r"for \(; st < r_bits; st \+= (\d+)\) r\.push_back\(\{st, (\d+)\}\);", (3, 4, 4)),
    ("zsplit", r"while \(zsplit < n_z && \(one_coset_per_workgroup \|\| tiles \* n_cols \* zsplit < (\d+)\)\) zsplit \*= 2;", (FILL_WORKGROUPS,)),
    ("scale_full", r"if \(fullscale && !group_cols && \(n_cols >= (\d+) \|\| inside\) && log_n >= (\d+) && log_n <= (\d+)\) a\.scale_full =",
     (FULL_MIN_COLS, FULL_MIN_LOG, FULL_MAX_LOG)),
    ("dif direct_first", r"a\.direct_first = direct && NTT_SWZ && a\.r_bits >= (\d+) && a\.r_bits \+ a\.cb == NTT_TILE_LOG;", (DIF_DIRECT_MIN_R,)),
    ("dit direct_first", r"a\.direct_first = direct && i > 0 && NTT_SWZ && a\.cb == (\d+) && a\.r_bits >= (\d+) && a\.r_bits % (\d+) == 0 && "
                         r"a\.r_bits \+ a\.cb == NTT_TILE_LOG;", DIT_DIRECT),
    ("kernel direct_first", r"const bool direct_first = MODE == 0 && THREADS == NTT_THREADS && a\.direct_first && tile_n == (\d+)u \* THREADS;", (16,)),
    ("zloop", r"if \(zloop && nz > (\d+)\) \{", (1,)),
]


def check_source(src):
    """[what differs] between `src` (the text of csrc/ntt.hip) and the restatement above; empty when they agree"""
    bad = []
    for name, rx, want in SOURCE_CONSTANTS:
        found = re.findall(rx, src)
        if len(found) != 1:
            bad.append("%s: the line this module mirrors occurs %d times in csrc/ntt.hip" % (name, len(found)))
            continue
        got = found[0] if isinstance(found[0], tuple) else ((found[0],) if want else ())
        if tuple(str(g) for g in got) != tuple(str(w) for w in want):
            bad.append("%s: csrc/ntt.hip has %s, tests/lde_cases.py %s" % (name, got, want))
    return bad
