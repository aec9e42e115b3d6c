"""GPU (run with -m gpu on an MI355X): the radix-16 passes of csrc/ntt.hip against the CPU oracle on inputs that sit on the carry
paths of the register DFT -- the coset LDE, which is the inverse transform (DIF rounds) followed by the forward one (DIT rounds), so a
wrong coefficient of either shows in the result.  Heights 2^1..2^5 run the partial rounds G = 1..4 and one full round, 2^12 one full
tile of three rounds, 2^13 a tile plus the strided pass.  Every stored output must be canonical and equal to the oracle's."""
import numpy as np
import pytest
import oracle_binding as ob
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
P = ob.P
CORNERS = np.array([0, 1, 2**32 - 1, 2**32, 2**64 - 2**32, P - 1], dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def inputs(log_n, w):
    n = 1 << log_n
    rng = np.random.default_rng(1000 + 10 * log_n + w)
    yield "zero", np.zeros((n, w), dtype=np.uint64)
    yield "p-1", np.full((n, w), P - 1, dtype=np.uint64)
    yield "corners", CORNERS[rng.integers(0, len(CORNERS), (n, w))]
    # a single non-zero entry at each position of a 16-point block (first block, and the last one of a longer column)
    vals = [P - 1, 2**32, 2**64 - 2**32, 1]
    for p0 in range(0, 16, w):
        m = np.zeros((n, w), dtype=np.uint64)
        for c in range(w):
            pos = p0 + c
            if pos < 16:
                m[(pos if c % 2 == 0 else n - 16 + pos) % n, c] = vals[pos % 4]
        yield "single%d" % p0, m
    yield "random", rng.integers(0, P, (n, w), dtype=np.uint64)


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("ab", [1, 3])
@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5, 12, 13])
def test_coset_lde_on_carry_path_inputs(ctx, log_n, ab, w):
    shift = ob.lib().orc_canonical_lde_shift(log_n + ab)
    for name, m in inputs(log_n, w):
        got = ctx.coset_lde_batch(m, ab, shift)
        assert (got < np.uint64(P)).all(), name
        assert (got == ob.coset_lde_bitrev(m, ab, shift)).all(), name
