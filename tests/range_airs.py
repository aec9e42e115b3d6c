"""Inputs of the range-table tests (tests/test_range_table_cpu.py, tests/test_gpu_range_table.py): the three-column test AIR's lookup
programs and the Miden statement's challenges and boundary pushes.  Test infrastructure only."""
import numpy as np
import oracle_binding as ob
from __graft_entry__ import load_package

load_package()
from miden_vm_amd import chiplets_air as CA, core_air as CO, dag, miden_statement as MS, protocol  # noqa: E402
from miden_vm_amd.testing import core_trace as CV  # noqa: E402

P = dag.P
JUNK = 0xDEADBEEF
RND = [(0x1234567890abcdef % P, 0x0fedcba987654321), (3141592653589793, 2718281828459045)]  # full extension-field challenges
V, M, C = 0, 1, 2           # columns of the test AIR: table value, multiplicity, the consumer's looked-up value
SLOT = (0, 0, 1, V, M)      # its provider: LogUp column 0, fraction 1


def _key(lb, x):
    return lb.randomness(0) + x * lb.randomness(1)


def table_lookup(kind="good"):
    """One bus over (V, M, C): the consumer 1 / (r0 + r1 C) and the provider -M / (r0 + r1 V).  The refused variants: `rowwise_g` (the
    coefficient of the cell is C, which differs from row to row), `rowwise_d0` (d0 takes C along), `reader` (the consumer's denominator
    reads V too), `mult` (the provider's multiplicity reads V)."""
    lb = dag.LookupBuilder(3, num_cols=1, num_randomness=2)
    v, m, c = lb.main(V), lb.main(M), lb.main(C)
    lb.fraction(0, 1, _key(lb, c + v) if kind == "reader" else _key(lb, c))
    if kind == "rowwise_g":
        lb.fraction(0, -m, _key(lb, v * c))
    elif kind == "rowwise_d0":
        lb.fraction(0, -m, _key(lb, v) + c)
    elif kind == "mult":
        lb.fraction(0, -(m + v), _key(lb, v))
    else:
        lb.fraction(0, -m, _key(lb, v))
    return dag.Lookup(lb, "range_" + kind)


def consumer_lookup():
    """A second instance on the same bus: one column, 1 / (r0 + r1 C) per row."""
    lb = dag.LookupBuilder(1, num_cols=1, num_randomness=2)
    lb.fraction(0, 1, _key(lb, lb.main(0)))
    return dag.Lookup(lb, "range_consumer")


def table_trace(lookups, n):
    """[n, 3] with both range columns junk; `lookups` (any length <= n) are cycled over the consumer column."""
    t = np.full((n, 3), JUNK, dtype=np.uint64)
    t[:, C] = np.resize(np.asarray(lookups, dtype=np.uint64), n)
    return t


def e_key(x, rnd=RND):
    """r0 + r1 x: the bus's encoding of value x, for boundary pushes."""
    return ((rnd[0][0] + rnd[1][0] * x) % P, (rnd[0][1] + rnd[1][1] * x) % P)


# ---- the Miden statement ----
def junked(core):
    """A core trace with both range columns overwritten: a different word per row in RANGE_V, one junk word in RANGE_M."""
    t = core.copy()
    t[:, CO.RANGE_V] = np.arange(7, 7 + t.shape[0], dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    t[:, CO.RANGE_M] = JUNK
    return t


def u32_memory_program(iters):
    """A loop of u32 operations (AND, ADD, MUL) and one memory store / load per iteration; stack at loop entry [counter, x, y, ...]."""
    S = CV.Span
    body = S(["DUP1", "DUP3", "U32AND", "DROP", "DUP1", ("PUSH", 0x9E3779B9), "U32ADD", "DROP", "MOVDN2", "SWAP", "DROP",
              "DUP1", "DUP3", "U32MUL", "DROP", "DROP", "DUP0", ("PUSH", 4), "MUL", "DUP2", "SWAP", "MSTORE", "DROP",
              "DUP0", ("PUSH", 4), "MUL", "MLOAD", "DROP", ("PUSH", 1), "NEG", "ADD", "DUP0", "EQZ", "NOT"])
    return CV.Join(S([("PUSH", 0x1234), ("PUSH", 0xABCDEF), ("PUSH", iters)]), CV.Join(CV.Loop(body), S(["DROP", "DROP", "DROP"])))


def miden_challenges(mats, pv, aux_in):
    """The debug challenges of mh_check_* / mh_fill_* for this statement (tests/test_gpu_check_balance.py debug_challenges)."""
    state = np.zeros(12, dtype=np.uint64)
    load_package().load_library().mh_miden_challenger_state(ob.ptr(state))
    pre = MS.statement_pre_observe(protocol.PROD_PARAMS, pv, aux_in)
    lh = [int(m.shape[0]).bit_length() - 1 for m in mats]
    ch = ob.Challenger([int(x) for x in state])
    ch.observe([int(x) for x in pre] + [len(lh)] + lh)
    return [ch.sample_ef() for _ in range(2)]


def miden_boundary(rnd, aux_in):
    ch = MS.Challenges(rnd[0], rnd[1])
    bnd = [(ch.encode(CA.BUS_BLOCK_HASH_TABLE, list(aux_in[0:4]) + [0, 0, 0]), 1), (ch.encode(CA.BUS_LOG_DEFERRED_ROOT, [0, 0, 0, 0]), 1),
           (ch.encode(CA.BUS_LOG_DEFERRED_ROOT, list(aux_in[4:8])), -1)]
    return bnd + [(ch.encode(CA.BUS_KERNEL_ROM_INIT, list(aux_in[i:i + 4])), 1) for i in range(8, len(aux_in), 4)]
