"""Times mh_fill_range_table_miden_traces on a Miden program of 2^16 core rows, next to the fill it ends with and the ledger it replaces.

The shape of tools/bench_fill.py's Miden part (testing/core_trace.py bench_program(500)):
  (a) Miden.fill_range_table on device-resident traces whose two range columns are junk,
  (b) Miden.fill_multiplicities (RANGE_M alone) on the same traces once the table is laid,
  (c) the host ledger's table: range_table(range_lookups) of testing/core_trace.py over lookups that are already collected (the
      collection inside the trace generator is not timed).
Each figure is the median of `--steps` calls after one warm-up call, host wall clock around calls that end in a synchronise; the
device's columns are checked against the host generator's first.  Nothing is asserted about speed.

  python tools/bench_range_table.py [--steps 7] > profiles/range_table.txt"""
import argparse, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def median_ms(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def line(name, t):
    print(f"  {name:<58s} median {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=500)
    args = ap.parse_args()
    pkg = load_package()
    from miden_vm_amd import core_air as CO
    from miden_vm_amd.testing import core_trace
    ctx = pkg.Ctx(0)
    print(f"mh_fill_range_table_miden_traces, measured: median of {args.steps} calls after a warm-up, host wall clock around the call")
    vm = core_trace.CoreVM(stack_inputs=list(range(16)))
    r = core_trace.prove_inputs(vm, core_trace.bench_program(args.iters))
    mats = [r["core"], r["chiplets"], r["poseidon2"]]
    pv, aux_in = r["public_values"], r["aux_inputs"]
    m = pkg.Miden(ctx)
    core = mats[0].copy()
    core[:, CO.RANGE_V] = np.arange(core.shape[0], dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    core[:, CO.RANGE_M] = 0xDEADBEEF
    trs = [ctx.upload_trace(t) for t in (core, mats[1], mats[2])]
    rep, info = m.fill_range_table(trs, pv, aux_in)
    assert rep == [] and (trs[0].download() == mats[0]).all(), "the call does not reproduce the host generator's range columns"
    print(f"\nMiden program (bench_program({args.iters})): core 2^{core.shape[0].bit_length() - 1}, chiplets 2^{mats[1].shape[0].bit_length() - 1}, "
          f"poseidon2 2^{mats[2].shape[0].bit_length() - 1} rows; {info.n_values} values in {info.rows_needed} table rows, "
          f"{sum(vm.range_lookups.values())} lookups")
    line("(a) Miden.fill_range_table", median_ms(lambda: m.fill_range_table(trs, pv, aux_in), args.steps))
    slots = [(0,) + s for s in CO.RANGE_M_MULT_SLOTS]
    line("(b) Miden.fill_multiplicities (RANGE_M), same traces", median_ms(lambda: m.fill_multiplicities(trs, pv, aux_in, slots), args.steps))
    lookups = dict(vm.range_lookups)
    assert core_trace.range_table(lookups) == [(int(a), int(b)) for a, b in mats[0][core.shape[0] - info.rows_needed:, [CO.RANGE_M, CO.RANGE_V]]]
    line("(c) range_table(range_lookups), the host ledger's table", median_ms(lambda: core_trace.range_table(lookups), args.steps))
    ctx.close()


if __name__ == "__main__":
    main()
