"""Times the precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces built on the device (mh_ec_traces_build,
csrc/ec_traces.hip) next to the upload they replace and the generators that lay them today.

The workload is the ledger of testing/precompile_trace.ec_msm_session on --terms points with --bits-bit scalars (Straus' interleaved
double-and-add over the expressions; the defaults give more than 2^17 MSM rows), recorded here without laying the session's other traces.

  (a) ec_traces from the five lists + a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise); the fence alone;
  (b) the device time of (a) per kernel, from the context's event profiler, in a pass of its own;
  (c) ctx.upload_trace of the four finished matrices (pageable numpy arrays: what a caller without this entry does);
  (d) Trace.upload_async + wait of the four matrices from page-locked memory: the fastest upload the library has;
  (e) the generators ec_msm_trace + ec_group_add_trace + ec_store_traces on the same ledgers, --gen-steps runs.
All medians of --steps runs after a warm-up, host wall clock.  The device's traces are compared with the generators' cell for cell.

  python tools/bench_ec_traces.py [--steps 7] [--terms 64] [--bits 72] > profiles/ec_traces.txt"""
import argparse, copy, os, random, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PHASES = ("ec_point_check", "ec_add_check", "ec_expr_check", "ec_term_check", "ec_groups_rows", "ec_points_rows", "ec_add_rows", "ec_msm_rows")
NAMES = ("groups", "points", "add", "msm")


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


def ledgers(PT, PA, n_terms, bits, seed=7):
    """ec_msm_session's ledgers without its traces: sum_i k_i (i G) as an MSM expression over the fixed environment"""
    rng = random.Random(seed)
    store, adds, muls, ec, ec_add = PT.UintStore().install_fixed_uints(), PT.UintAddRequires(), PT.UintMulRequires(), PT.EcStore(), PT.EcAddRequires()
    req = PT.EcRequire(ec, store, muls, adds, ec_add)
    group, _pai = req.create_group(0, 7, PA.K1_BASE_BOUND_PTR)
    msm = PT.EcMsmRequires(req)
    scalars = [rng.getrandbits(bits) | 1 << (bits - 1) for _ in range(n_terms)]
    intros = [msm.intro(req.add_point(group, *xy)) for xy in PT.k1_multiples(n_terms)]
    acc = None
    for bit in range(bits - 1, -1, -1):
        if acc is not None:
            acc = msm.combine(acc, acc)
        for k, e in zip(scalars, intros):
            if (k >> bit) & 1:
                acc = e if acc is None else msm.combine(acc, e)
    ec.require_ecpoint(msm.resolve(acc))
    ec.require_fixed_groups()
    return store, ec, ec_add, msm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--gen-steps", type=int, default=1)
    ap.add_argument("--terms", type=int, default=64)
    ap.add_argument("--bits", type=int, default=72)
    args = ap.parse_args()
    assert args.steps >= 5 and args.gen_steps >= 1
    pkg = load_package()
    from miden_vm_amd import precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    t0 = time.perf_counter()
    store, ec, ec_add, msm = ledgers(PT, PA, args.terms, args.bits)
    t_ledger = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    lists = PT.ec_lists(ec, ec_add, msm)
    t_lists = (time.perf_counter() - t0) * 1e3
    print(f"mh_ec_traces_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    built, info = ctx.ec_traces(*lists)
    got = [t.download() for t in built]
    for t in built:
        t.free()
    list_bytes, matrix_bytes = sum(x.nbytes for x in lists), sum(g.nbytes for g in got)
    print(f"ec_msm_session on {args.terms} points, {args.bits}-bit scalars: {info.n_groups} group, {info.n_points} points, {info.n_add} additions, "
          f"{info.n_exprs} expressions, {info.n_terms} term rows; traces " + ", ".join(f"{g.shape[0]} x {g.shape[1]}" for g in got) +
          f"; lists {list_bytes / 1e6:.2f} MB (" + " + ".join(str(x.nbytes) for x in lists) + f" B) against matrices {matrix_bytes / 1e6:.2f} MB; "
          f"recording the ledgers (host, sequential, 256-bit group law in Python integers; not part of the build) {t_ledger:.0f} ms, "
          f"ec_lists {t_lists:.0f} ms", flush=True)

    def build():
        trs, _ = ctx.ec_traces(*lists)
        ctx.poseidon2_permute(one)
        for t in trs:
            t.free()

    ta = median_ms(build, args.steps)
    line("(a) ec_traces from the lists + fence", ta)
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
        st, e2 = copy.deepcopy(store), copy.deepcopy(ec)
        bpl = PT.BytePairLutRequires()
        t0 = time.perf_counter()
        exp_msm = PT.ec_msm_trace(msm, st, bpl)
        exp_add = PT.ec_group_add_trace(ec_add, e2, bpl)
        exp_groups, exp_points = PT.ec_store_traces(e2)
        gen.append((time.perf_counter() - t0) * 1e3)
    exp = (exp_groups, exp_points, exp_add, exp_msm)
    for name, g, e in zip(NAMES, got, exp):
        assert g.shape == e.shape and (g == e).all(), f"the device's {name} trace differs from the generator's"
    print("  all four traces equal the generators', cell for cell", flush=True)

    def upload():
        trs = [ctx.upload_trace(e) for e in exp]
        ctx.poseidon2_permute(one)
        for t in trs:
            t.free()

    tc = median_ms(upload, args.steps)
    line("(c) ctx.upload_trace of the four finished matrices + fence", tc)
    pins = [pkg.pinned_array(ctx.lib, e.shape) for e in exp]
    for (pin, _), e in zip(pins, exp):
        pin[:] = e

    def upload_pinned():
        hs = [pkg.Trace.upload_async(ctx, pin) for pin, _ in pins]
        for h in hs:
            h.wait()
        for h in hs:
            h.free()

    td = median_ms(upload_pinned, args.steps)
    line("(d) Trace.upload_async + wait of the four matrices, page-locked", td)
    te = (statistics.median(gen), min(gen), max(gen))
    line(f"(e) the generators ec_msm_trace + ec_group_add_trace + ec_store_traces ({args.gen_steps} run{'s' if args.gen_steps > 1 else ''})", te)
    print(f"  (a) / (c) = {ta[0] / tc[0]:.3f}, (a) / (d) = {ta[0] / td[0]:.3f}: the build is {'BELOW' if ta[0] < td[0] else 'NOT below'} the page-locked upload; "
          f"(a) / (e) = {ta[0] / te[0]:.5f}", flush=True)
    del pins
    ctx.close()


if __name__ == "__main__":
    main()
