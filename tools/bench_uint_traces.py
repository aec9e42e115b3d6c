"""Times the precompile prover's UintStoreMul and UintAdd traces built on the device (mh_uint_traces_build, csrc/uint_traces.hip) next to
the upload they replace and the generator that lays them today.

The workload is the ledger of testing/precompile_trace.uint_arith_session(2^14): 2^14 multiply-accumulates and 2^14 additions over the
secp256k1 base field -- a 2^17 x 44 and a 2^15 x 30 trace.

  (a) uint_traces from the three lists + a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise); the fence alone;
  (b) the device time of (a) per kernel, from the context's event profiler;
  (c) ctx.upload_trace of the two finished matrices (pageable numpy arrays: what a caller without this entry does);
  (d) Trace.upload_async + wait of the two matrices from page-locked memory: the fastest upload the library has;
  (e) the generators uint_add_trace + uint_store_mul_trace on the same ledgers (Python integers), --gen-steps runs.
All medians of --steps runs after a warm-up, host wall clock.  The device's traces are compared with the generator's cell for cell.

  python tools/bench_uint_traces.py [--steps 7] [--log-n 14] > profiles/uint_traces.txt"""
import argparse, copy, os, random, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PHASES = ("ut_self", "ut_mul_witness", "ut_add_witness", "ut_usm_rows", "ut_add_rows")


def median_ms(fn, steps):
    ts = []
    for i in range(steps + 1):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i:
            ts.append(dt)
    return statistics.median(ts), min(ts), max(ts)


def line(name, t):
    print(f"  {name:<86s} median {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def ledgers(PT, PA, n_steps, seed=7):
    """uint_arith_session's ledgers without its traces: acc <- acc x + c_i, s_i = acc + c_i (mod p) over the fixed environment"""
    rng = random.Random(seed)
    store, adds, muls = PT.UintStore().install_fixed_uints(), PT.UintAddRequires(), PT.UintMulRequires()
    fp, m = PA.K1_BASE_BOUND_PTR, PA.K1_BOUND + 1
    req = PT.EcRequire(None, store, muls, adds, None)
    x = store.intern(rng.randrange(2, m), fp)
    acc = store.intern(rng.randrange(m), fp)
    for _ in range(n_steps):
        c = store.intern(rng.randrange(m), fp)
        acc = req._mac(1, acc, x, 1, c)
        req._uint_add(acc, c)
    return store, adds, muls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--gen-steps", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=14, help="log2 of the multiply-accumulates (and of the additions)")
    args = ap.parse_args()
    assert args.steps >= 5 and args.gen_steps >= 1
    pkg = load_package()
    from miden_vm_amd import precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    t0 = time.perf_counter()
    store, adds, muls = ledgers(PT, PA, 1 << args.log_n)
    t_ledger = (time.perf_counter() - t0) * 1e3
    rows, m, a = PT.uint_lists(store, adds, muls)
    print(f"mh_uint_traces_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    tu, ta_, info = pkg.uint_traces(ctx, rows, m, a)
    got_usm, got_add = tu.download(), ta_.download()
    tu.free()
    ta_.free()
    list_bytes, matrix_bytes = rows.nbytes + m.nbytes + a.nbytes, got_usm.nbytes + got_add.nbytes
    print(f"uint_arith_session(2^{args.log_n}): {info.n_store} stored values, {info.n_mul} multiply-accumulates, {info.n_add} additions; traces "
          f"{got_usm.shape[0]} x 44 and {got_add.shape[0]} x 30; lists {list_bytes / 1e6:.2f} MB ({rows.nbytes} + {m.nbytes} + {a.nbytes} B) against matrices "
          f"{matrix_bytes / 1e6:.2f} MB; interning the ledgers (host, sequential, not part of the build) {t_ledger:.0f} ms", flush=True)

    def build():
        x, y, _ = pkg.uint_traces(ctx, rows, m, a)
        ctx.poseidon2_permute(one)
        x.free()
        y.free()

    ta = median_ms(build, args.steps)
    line("(a) uint_traces from the lists + fence", ta)
    line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.steps):
        build()
    prof = ctx.prof()
    ctx.prof_enable(False)
    print("  (b) device time per call of (a), event profiler: " + ", ".join(f"{k} {prof[k]['ms'] / args.steps:.3f} ms" for k in PHASES if k in prof)
          + f"; sum {sum(prof[k]['ms'] for k in PHASES if k in prof) / args.steps:.3f} ms", flush=True)
    gen = []
    for i in range(args.gen_steps):
        st = copy.deepcopy(store)
        t0 = time.perf_counter()
        exp_add = PT.uint_add_trace(adds, st)
        exp_usm = PT.uint_store_mul_trace(st, muls, PT.BytePairLutRequires())
        gen.append((time.perf_counter() - t0) * 1e3)
    assert got_usm.shape == exp_usm.shape and (got_usm == exp_usm).all(), "the device's UintStoreMul trace differs from the generator's"
    assert got_add.shape == exp_add.shape and (got_add == exp_add).all(), "the device's UintAdd trace differs from the generator's"
    print("  both traces equal the generator's, cell for cell", flush=True)

    def upload():
        x, y = ctx.upload_trace(exp_usm), ctx.upload_trace(exp_add)
        ctx.poseidon2_permute(one)
        x.free()
        y.free()

    tc = median_ms(upload, args.steps)
    line("(c) ctx.upload_trace of the two finished matrices + fence", tc)
    pins = [pkg.pinned_array(ctx.lib, e.shape) for e in (exp_usm, exp_add)]
    for (pin, _), e in zip(pins, (exp_usm, exp_add)):
        pin[:] = e

    def upload_pinned():
        hs = [pkg.Trace.upload_async(ctx, pin) for pin, _ in pins]
        for h in hs:
            h.wait()
        for h in hs:
            h.free()

    td = median_ms(upload_pinned, args.steps)
    line("(d) Trace.upload_async + wait of the two matrices, page-locked", td)
    te = (statistics.median(gen), min(gen), max(gen))
    line(f"(e) the generators uint_add_trace + uint_store_mul_trace ({args.gen_steps} runs)", te)
    print(f"  (a) / (c) = {ta[0] / tc[0]:.3f}, (a) / (d) = {ta[0] / td[0]:.3f}: the build is {'BELOW' if ta[0] < td[0] else 'NOT below'} the page-locked upload; "
          f"(a) / (e) = {ta[0] / te[0]:.5f}", flush=True)
    del pins
    ctx.close()


if __name__ == "__main__":
    main()
