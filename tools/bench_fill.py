"""Times mh_fill_multiplicities on two shipped statements, next to what it is made of and what it replaces.

For the Keccak hashing session (miden-vm_amd/testing/precompile_trace.py precompile_session; the byte-pair table's three columns, 2^16
rows) and for a Miden program of 2^16 core rows (testing/core_trace.py bench_program; RANGE_M):
  (a) the fill call on device-resident traces (Precompile.fill_multiplicities / Miden.fill_multiplicities),
  (b) the exact balance check (check_balance(exact=True)) of the same statement in the same run,
  (c) the numpy counting call of the same size: np.bincount (and np.add.at) over as many lookups as the filled columns count, one
      call per column.  Only the counting call: the Python-side collection of the lookups inside the trace generators is not timed.
Each figure is the median of `--steps` calls after one warm-up call; the fill is checked against the builder's columns first.
Nothing is asserted about speed.

  python tools/bench_fill.py [--steps 7] > profiles/fill_multiplicities.txt"""
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


def numpy_ledger(columns, steps):
    """columns: the filled multiplicity columns (counts per table row).  -> timings of np.bincount / np.add.at over a shuffled list of
    that many lookups per column."""
    rng = np.random.default_rng(1)
    lists = [rng.permutation(np.repeat(np.arange(len(c)), c.astype(np.int64))) for c in columns]

    def bincount():
        return [np.bincount(ix, minlength=len(c)) for ix, c in zip(lists, columns)]

    def add_at():
        out = [np.zeros(len(c), dtype=np.uint64) for c in columns]
        for o, ix in zip(out, lists):
            np.add.at(o, ix, 1)
        return out

    assert all((a == c).all() for a, c in zip(bincount(), columns)) and all((a == c).all() for a, c in zip(add_at(), columns))
    return sum(len(ix) for ix in lists), median_ms(bincount, steps), median_ms(add_at, steps)


def line(name, t):
    print(f"  {name:<58s} median {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    args = ap.parse_args()
    pkg = load_package()
    from miden_vm_amd import core_air as CO, precompile_airs as PA
    from miden_vm_amd.testing import core_trace, precompile_trace as PT
    ctx = pkg.Ctx(0)
    print(f"mh_fill_multiplicities, measured: median of {args.steps} calls after a warm-up, host wall clock around the call")

    # ---- the Keccak hashing session ----
    inputs = [bytes((7 * i + j) & 0xff for j in range(200)) for i in range(16)]
    pairs, traces, info = PT.precompile_session(inputs, permute_batch=ctx.poseidon2_permute)
    root = info["public_root"]
    pc = pkg.Precompile(ctx)
    zeroed = [t.copy() for t in traces]
    zeroed[3][:] = 0
    trs = [ctx.upload_trace(t) for t in zeroed]
    slots = [(3,) + s for s in PA.BYTE_PAIR_LUT_MULT_SLOTS]
    w, rep = pc.fill_multiplicities(trs, root, slots)
    assert rep == [] and (trs[3].download() == traces[3]).all(), "the fill does not reproduce the builder's ledger"
    rows = sum(t.shape[0] for t in traces)
    print(f"\nKeccak hashing session: {len(inputs)} inputs of 200 bytes, 12 chiplets, {rows} rows in all (log heights "
          f"{[int(t.shape[0]).bit_length() - 1 for t in traces]}); byte-pair table 2^16 rows x 3 columns, {w} cells written")
    line("(a) Precompile.fill_multiplicities", median_ms(lambda: pc.fill_multiplicities(trs, root, slots), args.steps))
    line("(b) Precompile.check_balance(exact=True), same traces", median_ms(lambda: pc.check_balance(trs, root, exact=True), args.steps))
    n_lk, tb, ta = numpy_ledger([traces[3][:, c] for c in range(3)], args.steps)
    line(f"(c) np.bincount x 3 over {n_lk} lookups", tb)
    line(f"(c) np.add.at x 3 over {n_lk} lookups", ta)

    # ---- a Miden program of 2^16 core rows ----
    r = core_trace.prove_inputs(core_trace.CoreVM(stack_inputs=list(range(16))), core_trace.bench_program(500))
    mats = [r["core"], r["chiplets"], r["poseidon2"]]
    pv, aux_in = r["public_values"], r["aux_inputs"]
    m = pkg.Miden(ctx)
    core = mats[0].copy()
    core[:, CO.RANGE_M] = 0
    trs = [ctx.upload_trace(t) for t in (core, mats[1], mats[2])]
    slots = [(0,) + s for s in CO.RANGE_M_MULT_SLOTS]
    w, rep = m.fill_multiplicities(trs, pv, aux_in, slots)
    out = trs[0].download()
    v = mats[0][:, CO.RANGE_V]
    per_value = lambda col: np.bincount(v.astype(np.int64), weights=col.astype(np.float64), minlength=1 << 16)  # noqa: E731
    assert rep == [] and (per_value(out[:, CO.RANGE_M]) == per_value(mats[0][:, CO.RANGE_M])).all(), \
        "the fill does not reproduce the range checker's counts"
    print(f"\nMiden program (bench_program(500)): core 2^{core.shape[0].bit_length() - 1}, chiplets 2^{mats[1].shape[0].bit_length() - 1}, "
          f"poseidon2 2^{mats[2].shape[0].bit_length() - 1} rows; RANGE_M, {w} cells written")
    line("(a) Miden.fill_multiplicities", median_ms(lambda: m.fill_multiplicities(trs, pv, aux_in, slots), args.steps))
    line("(b) Miden.check_balance(exact=True), same traces", median_ms(lambda: m.check_balance(*trs, pv, aux_in, exact=True), args.steps))
    n_lk, tb, ta = numpy_ledger([mats[0][:, CO.RANGE_M]], args.steps)
    line(f"(c) np.bincount over {n_lk} lookups", tb)
    line(f"(c) np.add.at over {n_lk} lookups", ta)
    ctx.close()


if __name__ == "__main__":
    main()
