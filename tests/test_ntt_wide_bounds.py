"""The wide register DFT of csrc/ntt.hip (NTT_ASM_BFLY == 2) on exact integers, no GPU: the bound computation of
tools/ntt_wide_bounds.py holds for G = 1..4 in both directions, its fold masks are the ones the kernel compiles, and an
exact-integer model of one wide round equals the plain DFT mod p."""
import importlib.util
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("ntt_wide_bounds", os.path.join(ROOT, "tools", "ntt_wide_bounds.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)
P = B.P
SRC = open(os.path.join(ROOT, "miden-vm_amd", "csrc", "ntt.hip")).read()


def test_every_intermediate_fits_its_registers():
    rep = []
    B.check_all(rep)
    assert len(rep) == 2 * (1 + 2 + 3 + 4)
    # without element 0's bias the signed words stay well inside 96 bits, and with it below 2^95
    assert all(lg < 94 for _, _, _, lg in rep)
    assert B.Z % P == 0 and B.Z + 2**94 <= B.WIDE


def test_kernel_compiles_the_checked_fold_masks():
    for name, masks in (("NTT_WIDE_FOLD_FWD", B.FOLD_FWD), ("NTT_WIDE_FOLD_INV", B.FOLD_INV)):
        packed = int(re.search(r"#define %s (0x[0-9A-Fa-f]+)u" % name, SRC).group(1), 16)
        assert [(packed >> (8 * m)) & 0xFF for m in range(4)] == masks, name
    # the bias constant of ntt_w_bias
    w = [int(x, 16) for x in re.search(r"\+ Z = 2\^30 p = .* = \((0x[0-9A-F]+), (0x[0-9A-F]+), (0x[0-9A-F]+)\)", SRC).groups()]
    assert w[0] + (w[1] << 32) + (w[2] << 64) == B.Z


def test_a_fold_mask_less_does_not_fit():
    """The masks are needed, not decoration: without them a shift leaves 96 bits."""
    for name in ("FOLD_FWD", "FOLD_INV"):
        keep = getattr(B, name)
        setattr(B, name, [0, 0, 0, 0])
        try:
            with pytest.raises(AssertionError):
                B.bounds_round(4, name == "FOLD_INV")
        finally:
            setattr(B, name, keep)


@pytest.mark.parametrize("inv", [False, True], ids=["dit", "dif"])
@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_wide_round_equals_plain_dft(G, inv):
    n = 1 << G
    rng = random.Random(100 * G + inv)
    corners = [0, 1, 2**32 - 1, 2**32, 2**64 - 2**32, P - 1, P, 2**64 - 1]
    cases = [[2**64 - 1] * n, [P - 1] * n, [0] * n]
    cases += [[(2**64 - 1) if i == k else 0 for i in range(n)] for k in range(n)]
    cases += [[rng.choice(corners) for _ in range(n)] for _ in range(200)]
    cases += [[rng.randrange(2**64) for _ in range(n)] for _ in range(300)]
    for x in cases:
        out = B.model_round(x, G, inv)
        assert all(0 <= v < 2**64 for v in out)
        assert [v % P for v in out] == B.plain_dft(x, G, inv)
