"""tests/lde_cases.py held to its word, no GPU: the patterns are canonical, shaped and seeded; the tiling shortcut (oracle LDE of the distinct
columns, gathered) equals the oracle LDE of the tiled matrix; the shapes of tests/test_gpu_lde_plans.py reach every path the restated
dispatch names; and the restated thresholds are the ones csrc/ntt.hip compiles -- move one and this file says to look at the shapes again."""
import os
import re

import numpy as np
import pytest

import lde_cases as lc
import oracle_binding as ob
from corner_felts import CORNERS, HEAVY, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "miden-vm_amd", "csrc", "ntt.hip")).read()


@pytest.mark.parametrize("log_n,w", [(1, 1), (4, 2), (5, 3), (12, 2), (14, 1)])
def test_patterns_are_canonical_shaped_and_seeded(log_n, w):
    n = 1 << log_n
    a, b = lc.patterns(log_n, w), lc.patterns(log_n, w)
    names = [name for name, _ in a]
    assert len(set(names)) == len(names) and set(lc.LIGHT) <= set(names) and "same:heavy" in names
    assert sum(name.startswith("single") for name in names) == -(-32 // w)
    for (name, m), (_, m2) in zip(a, b):
        assert m.dtype == np.uint64 and m.shape == (n, w), name
        assert (m < np.uint64(P)).all(), name
        assert (m == m2).all(), name
    d = dict(a)
    assert (d["same:p-1"] == np.uint64(P - 1)).all() and (d["same:heavy"] == np.uint64(HEAVY)).all()
    assert np.isin(d["mix"], CORNERS).all()
    assert not (d["mix"] == dict(lc.patterns(log_n, w, seed=1))["mix"]).all() or n * w < 4
    if n >= 8:
        ctl = d["control"]
        assert np.isin(ctl[np.arange(n) % 4 != 0], CORNERS).all() and not np.isin(ctl[0::4], CORNERS).all()
    assert (d["alt"][0::2, 0] == np.uint64(P - 1)).all() and (d["alt"][1::2, 0] == 0).all()
    assert (d["half"][:n // 2, 0] == np.uint64(P - 1)).all() and (d["half"][n // 2:, 0] == 0).all()
    if w > 1:
        assert (d["alt"][:, 1] == np.uint64(P - 1) - d["alt"][:, 0]).all() and (d["half"][:, 1] == np.uint64(P - 1) - d["half"][:, 0]).all()


def test_single_entries_cover_both_blocks():
    log_n, w = 6, 2
    n = 1 << log_n
    seen = set()
    for name, m in lc.singles(log_n, w):
        for c in range(w):
            (rows,) = np.nonzero(m[:, c])
            assert rows.size == 1, name
            r = int(rows[0])
            assert r < 16 or r >= n - 16
            assert int(m[r, c]) == lc.SINGLE_VALUES[r % 16 % 4]
            seen.add(r)
    assert seen == set(range(16)) | set(range(n - 16, n))


def test_non_canonical_inputs_are_what_they_say():
    for log_n in (5, 12):
        m = lc.non_canonical(log_n, 3)
        assert m.dtype == np.uint64 and m.shape == (1 << log_n, 3) and (m == lc.non_canonical(log_n, 3)).all()
        flat = set(int(v) for v in m.reshape(-1)[:64]) | set(int(v) for v in np.unique(m)[-8:])
        assert {2**64 - 1, P, P + 0xFFFFFFFD} <= flat and P + 0xFFFFFFFE == 2**64 - 1
        assert (m >= np.uint64(P)).mean() > 0.5
        red = lc.reduce_mod_p(m)
        assert (red < np.uint64(P)).all()
        assert all(int(a) % P == int(b) for a, b in zip(m.reshape(-1)[:512], red.reshape(-1)[:512]))


def test_tiled_uses_every_distinct_column():
    for log_n, k, width in [(4, 16, 40), (4, 15, 15), (6, 16, 16), (5, 16, 256), (3, 4, 16)]:
        cols = lc.distinct_columns(log_n, k)
        assert cols.shape == (1 << log_n, k) and (cols < np.uint64(P)).all()
        assert len({cols[:, j].tobytes() for j in range(k)}) == k or (1 << log_n) < 16   # distinct (tiny columns may coincide)
        m, idx = lc.tiled(cols, width, 3)
        assert m.shape == (1 << log_n, width) and idx.shape == (width,)
        assert set(int(i) for i in idx) == set(range(k))
        assert (m == cols[:, idx]).all()
        m2, idx2 = lc.tiled(cols, width, 3)
        assert (idx == idx2).all() and (m == m2).all()
    with pytest.raises(AssertionError):
        lc.tiled(lc.distinct_columns(4, 16), 15, 0)


def test_tiling_shortcut_equals_the_oracle_on_the_whole_matrix():
    """the one place the shortcut is held to its word: LDE(tiled) == gather(LDE(distinct))"""
    log_n, width = 4, 40
    for ab in (1, 3):
        cols, m, idx = lc.tiled_case(log_n, width)
        assert cols.shape[1] == 16
        shift = ob.lib().orc_canonical_lde_shift(log_n + ab)
        whole = ob.coset_lde_bitrev(m, ab, shift)
        assert whole.shape == (16 << ab, width)
        assert (whole == ob.coset_lde_bitrev(cols, ab, shift)[:, idx]).all()


def test_restated_plans():
    """the plans the comments of csrc/ntt.hip describe"""
    assert lc.plan_passes(5) == [(0, 5, 0)] and lc.plan_passes(12) == [(0, 12, 0)]
    assert lc.plan_passes(13) == [(0, 12, 0), (12, 1, 11)]
    assert lc.plan_passes(20) == [(0, 12, 0), (12, 8, 4)]
    assert lc.plan_passes(21) == [(0, 14, 0), (14, 7, 7)] and lc.plan_passes(22) == [(0, 14, 0), (14, 8, 6)]
    assert lc.plan_passes(23) == [(0, 12, 0), (12, 6, 6), (18, 5, 7)]
    assert lc.plan_passes(24) == [(0, 12, 0), (12, 6, 6), (18, 6, 6)]
    for log_n in range(1, 31):
        plan = lc.plan_passes(log_n)
        assert sum(r for _, r, _ in plan) == log_n and all(s == sum(r for _, r, _ in plan[:i]) for i, (s, _, _) in enumerate(plan))
        assert all(r + cb == lc.ntt_tile_log(log_n) and cb >= lc.SEGMENT_BITS for _, r, cb in plan[1:])
    assert [lc.pass_rounds(r) for r in (1, 4, 6, 8, 12)] == [[(0, 1)], [(0, 4)], [(0, 2), (2, 4)], [(0, 4), (4, 4)], [(0, 4), (4, 4), (8, 4)]]
    # launch_pass: 2^16 x 51 columns keeps one coset per workgroup, 2^18 x 51 with blowup 8 does not
    assert lc.coset_loop(16, 51, 3) == [1, 1] and lc.coset_loop(18, 51, 3) == [4, 4]
    assert lc.coset_loop(*lc.COSET_LOOP) == [2, 2]


def test_shape_table_reaches_every_path():
    union = set()
    for shape in lc.shape_table():
        union |= lc.tags(*shape)
    assert union >= lc.REQUIRED_TAGS, sorted(lc.REQUIRED_TAGS - union)
    # ... and the sections reach what the issue gives them
    narrow = set().union(*(lc.tags(*s) for s in lc.NARROW))
    assert narrow >= {"strided:r=%d" % r for r in range(2, 9)} | {"rounds:2", "rounds:3", "rounds:4", "rounds:1,4", "rounds:2,4", "rounds:3,4",
                                                                 "rounds:4,4", "dif_direct", "dit_direct", "two_level"}
    assert lc.tags(20, 2, 1) >= {"dit_direct", "strided:r=8"} and not any("dit_direct" in lc.tags(n, 2, 1) for n in range(1, 20))
    assert [n for n in range(13, 21) if "dif_direct" in lc.tags(n, 2, 1)] == [16, 17, 18, 19, 20]
    for s in lc.WIDE:
        assert lc.tags(*s) >= {"scale_full", "rot", "full_tile"}, s
    for s in lc.WIDE_BELOW:
        assert "two_level" in lc.tags(*s) and "scale_full" not in lc.tags(*s), s
    assert "rot" not in lc.tags(11, 16, 1) and "full_tile" not in lc.tags(11, 16, 1)
    assert lc.tags(*lc.COSET_LOOP) >= {"n_z=2", "scale_full", "rot", "strided:r=2"} and "n_z=1" not in lc.tags(*lc.COSET_LOOP)
    # (2^20 x 16 by 2 is exactly 4096 workgroups: it walks its two cosets as well)
    assert [s for s in lc.NARROW + lc.WIDE + lc.WIDE_BELOW if "n_z=1" not in lc.tags(*s)] == [(20, 16, 1)]
    assert lc.tags(21, 1, 1) >= {"big_tile", "strided:r=7"} and "rot" not in lc.tags(21, 1, 1)
    assert lc.tags(23, 1, 1) >= {"three_pass", "strided:r=6", "strided:r=5", "dif_direct"} and "big_tile" not in lc.tags(23, 1, 1)
    # the switch children: the MODE = 1 kernel of MH_NTT_STEP needs a coset loop over a full contiguous tile
    assert [c for c in lc.SWITCH_CASES if "n_z=2" in lc.tags(*c[1:])] == [("tiled", 14, 256, 3)]
    assert set().union(*(lc.tags(*c[1:]) for c in lc.SWITCH_CASES)) >= {"scale_full", "two_level", "rot", "dif_direct", "dit_direct", "n_z=2"}


def test_restated_constants_are_the_ones_ntt_hip_compiles():
    bad = lc.check_source(SRC)
    assert not bad, "csrc/ntt.hip moved a threshold tests/lde_cases.py restates -- revisit its shapes (shape_table, REQUIRED_TAGS): " + "; ".join(bad)


EDITS = [("NTT_TILE_LOG = 12;", "NTT_TILE_LOG = 11;"), ("NTT_TILE_LOG_BIG = 14;", "NTT_TILE_LOG_BIG = 13;"), ("atoi(e) : 22;", "atoi(e) : 21;"),
         ("log_n > 20 && log_n <= big_max", "log_n > 19 && log_n <= big_max"), ("max_r = T - 4;", "max_r = T - 5;"),
         ("zsplit < 4096", "zsplit < 2048"), ("(n_cols >= 16 || inside)", "(n_cols >= 32 || inside)"),
         ("inside) && log_n >= 12 && log_n <= 24", "inside) && log_n >= 13 && log_n <= 24"),
         ("inside) && log_n >= 12 && log_n <= 24", "inside) && log_n >= 12 && log_n <= 22"),
         ("direct && NTT_SWZ && a.r_bits >= 4 &&", "direct && NTT_SWZ && a.r_bits >= 5 &&"),
         ("a.cb == 4 && a.r_bits >= 8 && a.r_bits % 4 == 0", "a.cb == 4 && a.r_bits >= 4 && a.r_bits % 4 == 0"),
         ("#define NTT_SWZ 1", "#define NTT_SWZ 0"), ("if (zloop && nz > 1)", "if (zloop && nz > 2)")]


@pytest.mark.parametrize("old,new", EDITS, ids=[re.sub(r"\W+", "_", new)[:40] for _, new in EDITS])
def test_a_moved_threshold_is_noticed(old, new):
    assert SRC.count(old) == 1, old
    assert lc.check_source(SRC.replace(old, new)), new
