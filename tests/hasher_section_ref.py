"""The rule csrc/hasher_section.hip implements (include/midenhip.h mh_hasher_section_build), restated on numpy: the controller rows of
an op list, the perm_id ledger, the per-op results and the defects.  The permutations of all chains are taken level by level through
miden_air.permute_batch, which is what makes lists of a few thousand permutations cheap; tests/test_hasher_section_cpu.py holds this
file to testing/chiplets_trace.Hasher (the executable form of the reference's rule) and to the reference processor's snapshots."""
import numpy as np
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import miden_air as MA  # noqa: E402
from miden_vm_amd.testing import chiplets_trace as CT  # noqa: E402

P = MA.P
DT = pkg.HASH_OP_DTYPE
RES = pkg.HASH_RESULT_DTYPE
MAX_PERMS = 1 << 24
PERMUTE, CONTROL, BASIC, VERIFY, UPDATE = range(5)


class Defect(Exception):
    def __init__(self, kind, index):
        super().__init__(f"defect {kind} at op {index}")
        self.kind, self.index = kind, index


class TooMany(Exception):
    pass


def records(ops):
    ops = np.asarray(ops, dtype=DT).reshape(-1)
    return [(int(o["kind"]), int(o["count"]), int(o["index"]), int(o["payload"])) for o in ops]


def plan_op(kind, count, index, payload, n_felts):
    """-> (permutations, mrupdate increment, first defect of the op in the order 1, 2, 3, 4)"""
    if kind > 4:
        return 0, 0, 1
    if kind == PERMUTE:
        perms, need = 1, 12
    elif kind == CONTROL:
        perms, need = 1, 8
    elif kind == BASIC:
        if count == 0:
            return 0, 0, 2
        perms, need = count, 8 * count
    else:
        if count == 0 or count > 64:
            return 0, 0, 2
        legs = 2 if kind == UPDATE else 1
        perms, need = legs * count, 4 * legs + 4 * count
        if index >= P or (count < 64 and index >> count):
            return perms, int(kind == UPDATE), 3
    return perms, int(kind == UPDATE), 4 if payload > n_felts or need > n_felts - payload else 0


def min_log_n(n_rows):
    return max(6, (max(n_rows, 1) - 1).bit_length())


def section(ops, felts, cap_rows=None):
    """-> (rows uint64 [n_rows, 20], results HASH_RESULT_DTYPE [n_ops], info dict).  Raises TooMany, or Defect with the lowest defective
    op (kinds 1..4; the op's first kind), or Defect(5, first op without its rows) for a target of cap_rows rows."""
    ops = records(ops)
    felts = np.asarray(felts, dtype=np.uint64).reshape(-1)
    n_ops = len(ops)
    plans = [plan_op(*o, len(felts)) for o in ops]
    if sum(min(p[0], 2 * MAX_PERMS) for p in plans) > MAX_PERMS:
        raise TooMany()
    for i, p in enumerate(plans):
        if p[2]:
            raise Defect(p[2], i)
    first, mru, n_perms, updates = [], [], 0, 0
    for perms, inc, _ in plans:
        first.append(n_perms)
        n_perms += perms
        updates += inc
        mru.append(updates)
    n_rows = -(-2 * n_perms // 8) * 8
    if cap_rows is not None:
        for i in range(n_ops):
            if 2 * (first[i] + plans[i][0]) > cap_rows:
                raise Defect(5, i)
        if n_rows > cap_rows:
            raise Defect(5, n_ops)
    canon = felts % np.uint64(P)
    # chains: (op, leg, first permutation, permutations)
    chains = []
    for i, (kind, count, index, payload) in enumerate(ops):
        if kind == UPDATE:
            chains += [(i, 0, first[i], count), (i, 1, first[i] + count, count)]
        else:
            chains.append((i, 0, first[i], count if kind >= BASIC else 1))
    pre = np.zeros((n_perms, 12), dtype=np.uint64)
    post = np.zeros((n_perms, 12), dtype=np.uint64)
    state = np.zeros((len(chains), 12), dtype=np.uint64)
    for c, (i, leg, _, _) in enumerate(chains):
        kind, count, index, payload = ops[i]
        if kind >= VERIFY:
            state[c, 0:4] = canon[payload + 4 * leg:payload + 4 * leg + 4]
        elif kind == PERMUTE:
            state[c, 8:12] = canon[payload + 8:payload + 12]
        elif kind == CONTROL:
            state[c, 9] = index % P
    t = 0
    while True:
        live = [c for c, ch in enumerate(chains) if ch[3] > t]
        if not live:
            break
        for c in live:
            i, leg, _, _ = chains[c]
            kind, count, index, payload = ops[i]
            if kind >= VERIFY:
                at = payload + (8 if kind == UPDATE else 4) + 4 * t
                sib, root = canon[at:at + 4], state[c, 0:4].copy()
                state[c, 0:8] = np.concatenate([sib, root] if (index >> t) & 1 else [root, sib])
                state[c, 8:12] = 0
            else:
                state[c, 0:8] = canon[payload + 8 * t:payload + 8 * t + 8]
        at = np.array([chains[c][2] + t for c in live])
        pre[at] = state[live]
        state[live] = MA.permute_batch(state[live])
        post[at] = state[live]
        t += 1
    # perm ids: first appearance of the canonical pre-state
    ids, ledger, mult = np.zeros(n_perms, dtype=np.uint64), {}, []
    for p in range(n_perms):
        key = pre[p].tobytes()
        if key not in ledger:
            ledger[key] = len(ledger)
            mult.append(0)
        ids[p] = ledger[key]
        mult[ledger[key]] += 1
    rows = np.zeros((n_rows, 20), dtype=np.uint64)
    rows[2 * n_perms:, 1] = 1
    rows[2 * n_perms:, 16] = updates
    for i, leg, p0, n in chains:
        kind, count, index, payload = ops[i]
        merkle = kind >= VERIFY
        sel = {PERMUTE: (1, 0, 0), CONTROL: (1, 0, 0), BASIC: (1, 0, 0), VERIFY: (1, 0, 1), UPDATE: (1, 1, 1) if leg else (1, 1, 0)}[kind]
        for t in range(n):
            last = t == n - 1
            r = 2 * (p0 + t)
            node_in = index >> t if merkle else 0
            node_out = index >> (t + 1) if merkle else 0
            rows[r, 0:3] = sel
            rows[r, 15:19] = np.array([node_in, mru[i], int(t == 0), node_in & 1], dtype=np.uint64)
            rows[r + 1, 0:3] = (0, 0, 1) if kind == PERMUTE or not last else (0, 0, 0)
            rows[r + 1, 15:19] = np.array([node_out, mru[i], int(last), 0 if last else node_out & 1], dtype=np.uint64)
    rows[0:2 * n_perms:2, 3:15] = pre
    rows[1:2 * n_perms:2, 3:15] = post
    rows[0:2 * n_perms:2, 19] = ids
    rows[1:2 * n_perms:2, 19] = ids
    results = np.zeros(n_ops, dtype=RES)
    for i, leg, p0, n in chains:
        if ops[i][0] == UPDATE and leg == 0:
            results["old_root"][i] = post[p0 + n - 1, 0:4]
        else:
            results["addr"][i] = 2 * first[i] + 1
            results["state"][i] = post[p0 + n - 1]
    info = dict(n_rows=n_rows, n_permutations=n_perms, n_requests=len(ledger), mrupdate_id=updates, multiplicities=mult,
                request_states=pre[[int(np.argmax(ids == k)) for k in range(len(ledger))]] if n_perms else pre)
    return rows, results, info


def replay(ops, felts):
    """The op list played into a fresh testing/chiplets_trace.Hasher -> (hasher, [what each call returned])."""
    felts = [int(x) for x in np.asarray(felts, dtype=np.uint64).reshape(-1)]
    h, out = CT.Hasher(), []
    for kind, count, index, payload in records(ops):
        f = felts[payload:payload + 12 + 8 * count]
        words = lambda at, n: [f[at + 4 * j:at + 4 * j + 4] for j in range(n)]  # noqa: E731
        if kind == PERMUTE:
            out.append(h.permute(f[0:12]))
        elif kind == CONTROL:
            out.append(h.hash_control_block(f[0:4], f[4:8], index))
        elif kind == BASIC:
            out.append(h.hash_basic_block([f[8 * b:8 * b + 8] for b in range(count)]))
        elif kind == VERIFY:
            out.append(h.build_merkle_root(f[0:4], words(4, count), index))
        else:
            out.append(h.update_merkle_root(f[0:4], f[4:8], words(8, count), index))
    return h, out


def random_list(seed, n_ops=12, max_depth=5, max_batches=4, repeat=0.25, kinds=(0, 1, 2, 3, 4), big=True):
    """A seeded mixed list: 64-bit operands (non-canonical ones among them), now and then an op listed again or a state used twice."""
    rng = np.random.default_rng(seed)
    ops, felts = [], []

    def take(n):
        hi = 1 << 64 if big else P
        return [int(x) for x in rng.integers(0, hi, n, dtype=np.uint64)]

    for _ in range(n_ops):
        if ops and rng.random() < repeat:
            k, c, ix, pay = ops[int(rng.integers(0, len(ops)))]
            ops.append((k, c, ix, pay))                     # the same operands again: a memoised replay, repeated requests
            continue
        kind = int(rng.choice(kinds))
        count = 0
        index = int(rng.integers(0, 1 << 64, dtype=np.uint64)) if kind == CONTROL else 0
        if kind == PERMUTE:
            operands = take(12)
        elif kind == CONTROL:
            operands = take(8)
        elif kind == BASIC:
            count = int(rng.integers(1, max_batches + 1))
            operands = take(8 * count)
        else:
            count = int(rng.integers(1, max_depth + 1))
            index = int(rng.integers(0, 1 << count))
            operands = take((8 if kind == UPDATE else 4) + 4 * count)
        ops.append((kind, count, index, len(felts)))
        felts += operands
    return np.array(ops, dtype=DT), np.array(felts, dtype=np.uint64)
