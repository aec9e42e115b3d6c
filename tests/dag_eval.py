"""An independent evaluation of a constraint DAG: the blob's nodes over Python integers, EF = F_p[x] / (x^2 - 7).  Shared by the checker
tests (tests/test_gpu_check_constraints.py) and the fold tests (tests/test_gpu_constraint_fold.py); no device code, no oracle."""
from __graft_entry__ import load_package

load_package()
from miden_vm_amd import dag  # noqa: E402

P = dag.P
W = 7
ROOT_2_32 = 1753635133440165772  # two-adic generator of order 2^32


def ef(v):
    return v if isinstance(v, tuple) else (v % P, 0)


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def parse(blob):
    w = [int(x) for x in blob]
    n_periodic, n_nodes, n_cons = w[6], w[8], w[9]
    k, periodic = 12, []
    for _ in range(n_periodic):
        ln = w[k]
        periodic.append(w[k + 1:k + 1 + ln])
        k += 1 + ln
    nodes = []
    for _ in range(n_nodes):
        x, c = w[k], w[k + 1]
        nodes.append((x & 0xFF, (x >> 8) & ((1 << 28) - 1), x >> 36, c))
        k += 2
    return periodic, nodes, w[k:k + n_cons]


def debug_selectors(r, n):
    """The reference's debug selectors (the checker's exact stage): (is_first, is_last, is_transition)."""
    return int(r == 0), int(r == n - 1), int(r != n - 1)


def screen_selectors(r, n):
    """The selector values of the constraint program on the trace domain (mh_constraint_fold, the checker's screen):
    is_first = [r == 0], is_last = [r == n-1], is_transition = w_n^r - w_n^-1 (zero on the last row only)."""
    w = pow(ROOT_2_32, (1 << 32) // n, P)
    return int(r == 0), int(r == n - 1), (pow(w, r, P) - pow(w, n - 1, P)) % P


def constraint_values(air, main, aux, prep, publics, rnd, aux_values, selectors=debug_selectors):
    """-> [n][K] the value (an EF pair) of every constraint on every row."""
    periodic, nodes, cons = parse(air.blob)
    n = main.shape[0]
    out = []
    for r in range(n):
        rows = (r, (r + 1) % n)
        first, last, trans = selectors(r, n)
        val = []
        for op, a, b, c in nodes:
            if op == dag.OP_CONST: v = ef(c)
            elif op == dag.OP_MAIN: v = ef(int(main[rows[b], a]))
            elif op == dag.OP_AUX: v = (int(aux[rows[b], 2 * a]) % P, int(aux[rows[b], 2 * a + 1]) % P)
            elif op == dag.OP_PREPROCESSED: v = ef(int(prep[rows[b], a]))
            elif op == dag.OP_PUBLIC: v = ef(publics[a])
            elif op == dag.OP_PERIODIC: v = ef(periodic[a][r % len(periodic[a])])
            elif op == dag.OP_IS_FIRST: v = ef(first)
            elif op == dag.OP_IS_LAST: v = ef(last)
            elif op == dag.OP_IS_TRANSITION: v = ef(trans)
            elif op == dag.OP_RANDOMNESS: v = tuple(x % P for x in rnd[a])
            elif op == dag.OP_AUX_VALUE: v = tuple(x % P for x in aux_values[a])
            elif op == dag.OP_ADD: v = e_add(val[a], val[b])
            elif op == dag.OP_SUB: v = e_sub(val[a], val[b])
            elif op == dag.OP_MUL: v = e_mul(val[a], val[b])
            elif op == dag.OP_NEG: v = e_sub((0, 0), val[a])
            else: raise AssertionError(op)
            val.append(v)
        out.append([val[nid] for nid in cons])
    return out


def evaluate(air, main, aux, prep, publics, rnd, aux_values):
    """-> {constraint: (rows, first_row, value at first_row)} of every constraint that does not vanish somewhere (debug selectors)."""
    out = {}
    for r, row in enumerate(constraint_values(air, main, aux, prep, publics, rnd, aux_values)):
        for k, v in enumerate(row):
            if v != (0, 0):
                cnt, first, fv = out.get(k, (0, r, v))
                out[k] = (cnt + 1, first, fv)
    return out


def alpha_fold(values, alpha):
    """[n][K] constraint values -> [n] F(r) = sum_k alpha^(K-1-k) C_k(r) (Horner: F = F * alpha + C_k)."""
    alpha = (int(alpha[0]) % P, int(alpha[1]) % P)
    out = []
    for row in values:
        f = (0, 0)
        for v in row:
            f = e_add(e_mul(f, alpha), v)
        out.append(f)
    return out
