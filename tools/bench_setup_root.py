#!/usr/bin/env python3
"""First-call time of mh_precompile_setup_root (host only: the 2^16 x 4 byte-pair table, coset LDE x 8 + LMCS tree on the CPU) per hash
function, next to the CPU checker's commit_traces of the same table timed the same way (one call, wall clock, same process).
    python tools/bench_setup_root.py > profiles/setup_root_host.txt"""
import os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_binding as ob  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
i = np.arange(1 << 16, dtype=np.uint64)
a, b = i >> np.uint64(8), i & np.uint64(0xff)
table = np.stack([a, b, (~a & np.uint64(0xff)) & b, a ^ b], axis=1)
print(f"# host threads: min(16, {os.cpu_count()} hardware threads); checker OpenMP threads: {ob.omp_threads()}")
print(f"# {'hasher':<10} {'mh_precompile_setup_root, first call (s)':>42} {'checker commit_traces (s)':>28} {'equal':>6}")
for h in ("poseidon2", "blake3", "keccak", "rpo", "rpx"):
    t0 = time.perf_counter()
    got = pkg.precompile_setup_root(h)
    t1 = time.perf_counter()
    ob.set_lmcs(h)
    t2 = time.perf_counter()
    exp = ob.commit_traces([table], 3)["root"]
    t3 = time.perf_counter()
    ob.set_lmcs("poseidon2")
    print(f"  {h:<10} {t1 - t0:>42.3f} {t3 - t2:>28.3f} {str(bool((got == exp).all())):>6}")
