"""The rule of mh_memory_section_build / mh_miden_memory_section (csrc/memory_section.hip), restated in plain Python.  A helper module,
not a test: tests/test_memory_section_cpu.py holds it to testing/chiplets_trace.Memory.section() (the restatement of Memory::fill_trace),
tests/test_gpu_memory_section.py holds the kernels to it.

A list is a sequence of (ctx, addr, clk, kind, value[4]) records (MEM_ACCESS_DTYPE, or tuples): kind bit 0 = read, bit 1 = word access,
addr the element address.  Rows are ordered by (ctx, addr >> 2, clk), ties keep arrival order; the word is carried by a plain overlay
scan; row 0 has delta 1 and f_scw 1."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
WIDTH = 17
COLS = ["rw", "ew", "ctx", "word_addr", "idx0", "idx1", "clk", "v0", "v1", "v2", "v3", "d0", "d1", "d_inv", "f_scw", "w0", "w1"]
MAX_N = 1 << 24


class Defect(Exception):
    def __init__(self, kind, index):
        super().__init__(f"defect {kind} at access {index}")
        self.kind, self.index = kind, index


def records(accesses):
    """-> [(ctx, addr, clk, kind, (v0, v1, v2, v3))] of Python ints"""
    return [(int(a[0]), int(a[1]), int(a[2]), int(a[3]), tuple(int(x) for x in a[4])) for a in accesses]


def min_log_n(n):
    return max(6, (n - 1).bit_length()) if n else 6


def order(acc):
    """the arrival indices in row order"""
    return sorted(range(len(acc)), key=lambda i: (acc[i][0], acc[i][1] >> 2, acc[i][2], i))


def section(accesses, capacity=None):
    """-> (rows uint64 [n, 17], row_of [n], n_words, n_contexts); raises Defect.  capacity: the rows the target has (defect 4)."""
    acc = records(accesses)
    n = len(acc)
    if capacity is not None and n > capacity:
        raise Defect(4, capacity)
    # 1, 2: the lowest arrival index of either kind
    for i, (ctx, addr, clk, kind, value) in enumerate(acc):
        if kind > 3:
            raise Defect(1, i)
        if kind & 2 and addr & 3:
            raise Defect(2, i)
    srt = order(acc)
    # 3: each row against its predecessor; the later access is reported, the lowest of them
    clash = [i for p, i in zip(srt, srt[1:])
             if (acc[p][0], acc[p][1] >> 2, acc[p][2]) == (acc[i][0], acc[i][1] >> 2, acc[i][2]) and not (acc[p][3] & 1 and acc[i][3] & 1)]
    if clash:
        raise Defect(3, min(clash))
    out = np.zeros((n, WIDTH), dtype=np.uint64)
    row_of = np.zeros(n, dtype=np.uint32)
    word, prev, n_words, n_contexts = None, None, 0, 0
    for r, i in enumerate(srt):
        ctx, addr, clk, kind, value = acc[i]
        is_read, is_word = kind & 1, (kind >> 1) & 1
        waddr, idx = addr & ~3, 0 if is_word else addr & 3
        first = prev is None or (prev[0], prev[1]) != (ctx, waddr)
        if first:
            word = [0, 0, 0, 0]
            n_words += 1
        if prev is None or prev[0] != ctx:
            n_contexts += 1
        if not is_read:
            if is_word:
                word = [v % P for v in value]
            else:
                word[idx] = value[0] % P
        if prev is None:
            delta, same = 1, 1
        elif prev[0] != ctx:
            delta, same = ctx - prev[0], 0
        elif prev[1] != waddr:
            delta, same = waddr - prev[1], 0
        else:
            delta, same = clk - prev[2], 1
        assert 0 <= delta < 1 << 32
        widx = waddr >> 2
        out[r] = [is_read, is_word, ctx, waddr, idx & 1, idx >> 1, clk] + word + [delta & 0xFFFF, delta >> 16,
                                                                                 pow(delta, P - 2, P) if delta else 0, same,
                                                                                 widx & 0xFFFF, widx >> 16]
        row_of[i] = r
        prev = (ctx, waddr, clk)
    return out, row_of, n_words, n_contexts


def replay(accesses):
    """The list played into a fresh testing/chiplets_trace.Memory -> that object (an AssertionError of the generator passes through)."""
    from miden_vm_amd.testing import chiplets_trace as CT
    m = CT.Memory()
    for ctx, addr, clk, kind, value in records(accesses):
        if kind == 0:
            m.write(ctx, addr, clk, value[0])
        elif kind == 1:
            m.read(ctx, addr, clk)
        elif kind == 2:
            m.write_word(ctx, addr, clk, value)
        else:
            m.read_word(ctx, addr, clk)
    return m


def random_list(seed, n_max=60, big=True):
    """A seeded list a processor could emit: clocks never decrease, several reads may share a cycle, element and word accesses mix on
    one word, no access meets a write of its word in its cycle.  big: contexts up to 2^32 - 1, words up to 2^32 - 4, a first clock
    of 0."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, n_max + 1))
    ctxs = [0, 1, 7] + ([(1 << 32) - 1, 1 << 31] if big else [])
    words = [0, 4, 8, 1 << 18] + ([(1 << 32) - 4, 1 << 31] if big else [])
    ctxs = ctxs[:int(rng.integers(1, len(ctxs) + 1))] if seed % 3 else ctxs
    clk = 0 if seed % 2 == 0 else int(rng.integers(0, 1000))
    last = {}   # (ctx, word) -> (clk, was a write)
    out = []
    while len(out) < n:
        ctx, w = ctxs[int(rng.integers(0, len(ctxs)))], words[int(rng.integers(0, len(words)))]
        kind = int(rng.integers(0, 4))
        seen = last.get((ctx, w))
        if seen and seen[0] == clk and (seen[1] or not kind & 1):
            clk += 1
        addr = w if kind & 2 else w + int(rng.integers(0, 4))
        value = tuple(int(x) for x in rng.integers(0, 1 << 64, 4, dtype=np.uint64))
        out.append((ctx, addr, clk, kind, value))
        last[(ctx, w)] = (clk, not kind & 1)
        step = int(rng.integers(0, 4))
        clk += 0 if step < 2 else (1 if step == 2 else int(rng.integers(1, 1 << 20)))
    return out
