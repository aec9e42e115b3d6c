"""Times the precompile prover's Poseidon2 chiplet trace built on the device (mh_poseidon2_chiplet_trace_build,
csrc/poseidon2_chiplet.hip) next to the upload it replaces and the generator bench.py runs today.

Workloads:
  chunk   the ledger of bench.py's chunk_poseidon2_session_probe (seed 4: 63 distinct inputs of up to 32 768 bytes, chains of up to 1023
          blocks, 34 332 cycles, 2^20 rows x 32 = 268 MB), literal blocks;
  wide    2^15 one-block absorptions (2^19 rows), literal blocks;
  fold    a fold chain 1024 deep: absorption k absorbs the digest of absorption k - 1 by reference (1024 levels of one chain, 2^14 rows).
Per workload:
  (a) poseidon2_chiplet_trace + a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise); the fence alone;
  (b) the device time of its two phases from the library's event profiler (mh_prof_*), in a pass of its own, and the chains phase per
      block of the longest chain;
  (c) Trace.upload_async + wait of the finished, page-locked matrix: the transfer (a) replaces;
  (d) the generator testing/precompile_trace.poseidon2_chiplet_trace with permute_batch=ctx.poseidon2_permute: what bench.py does today.
Medians of `--steps` runs after one warm-up run, host wall clock.  The device's trace is compared with the generator's first.  Nothing is
asserted about speed.  At the end the (a) and (b) lines are taken again in two child processes whose chains phase runs one kernel form on
every level (MH_P2C_GROUP_MAX_CHAINS=0: a lane a chain; =1048576: 16 lanes a chain): the A/B behind the choice of form by level width.

  python tools/bench_poseidon2_chiplet.py [--steps 7] > profiles/poseidon2_chiplet.txt"""
import argparse, os, statistics, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PHASES = ("p2c_chains", "p2c_cycles")


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


def workloads(pkg, PT):
    rng = np.random.default_rng(4)
    ledger = PT.Poseidon2Requires()
    req = PT.ChunkRequires(ledger)
    inputs = [bytes(rng.integers(0, 256, int(rng.integers(0, 32769)), dtype=np.uint8)) for _ in range(63)]
    inputs.append(inputs[0])
    for data in inputs:
        req.require(data)
        ledger.require_digest(req.last)
    yield "chunk", "bench.py's chunk probe", ledger, False
    rng = np.random.default_rng(5)
    wide = PT.Poseidon2Requires()
    felts = rng.integers(0, pkg.P, (1 << 15, 12), dtype=np.uint64)
    for row in felts:                                        # the ledger's own fields, without interning 2^15 random blocks one by one
        r = [int(x) for x in row]
        wide.absorptions.append([tuple(r[8:12]), [(tuple(r[0:4]), tuple(r[4:8]))], wide.next_seq, 1, 1])
        wide.next_seq += 1
    yield "wide", "2^15 one-block absorptions", wide, False
    rng = np.random.default_rng(6)
    fold = PT.Poseidon2Requires()
    prev = fold.require_absorption([1, 2, 3, 4], [([5, 6, 7, 8], [9, 10, 11, 12])])
    for _ in range(1023):
        prev = fold.require_absorption([1, 2, 3, 4], [(fold.digest(prev), [int(x) for x in rng.integers(0, pkg.P, 4, dtype=np.uint64)])])
    yield "fold", "a fold chain 1024 deep, by reference", fold, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--build-only", action="store_true", help="only the (a) and (b) lines (the child of the A/B)")
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    from miden_vm_amd.testing import precompile_trace as PT
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    if not args.build_only:
        print(f"mh_poseidon2_chiplet_trace_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    for key, title, ledger, refs in workloads(pkg, PT):
        absorptions, blocks, r = ledger.lists(refs=refs)
        rec = np.array(absorptions, dtype=pkg.P2C_ABSORPTION_DTYPE)
        r = r if refs else None
        longest = max(a[1] for a in absorptions)
        t, info = pkg.poseidon2_chiplet_trace(ctx, rec, blocks, r)
        got = t.download()
        t.free()
        print(f"{key}: {title}: {info.n_absorptions} absorptions, {info.n_cycles} cycles, {info.n_levels} levels, longest chain {longest} blocks, "
              f"trace {got.shape[0]} x 32 ({got.nbytes / 1e6:.1f} MB)", flush=True)

        def build():
            tr, _ = pkg.poseidon2_chiplet_trace(ctx, rec, blocks, r)
            ctx.poseidon2_permute(one)
            tr.free()

        ta = median_ms(build, args.steps)
        line("(a) poseidon2_chiplet_trace from the ledger + fence", ta)
        line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(args.steps):
            build()
        prof = ctx.prof()
        ctx.prof_enable(False)
        chains = prof["p2c_chains"]["ms"] / args.steps
        serial = info.n_levels if refs else longest                    # dependent permutations of the chains phase
        print("  (b) device time per call of (a), event profiler: " + ", ".join(f"{k} {prof[k]['ms'] / args.steps:.3f} ms" for k in PHASES if k in prof)
              + f"; p2c_chains {1e3 * chains / serial:.2f} us per block of the longest chain ({serial} dependent permutations)", flush=True)
        if args.build_only:
            continue
        t0 = time.perf_counter()
        exp, _ = PT.poseidon2_chiplet_trace(ledger, permute_batch=ctx.poseidon2_permute)
        first = (time.perf_counter() - t0) * 1e3
        assert got.shape == exp.shape and (got == exp).all(), "the device's trace differs from the generator's"
        pin, own = pkg.pinned_array(ctx.lib, exp.shape)
        pin[:] = exp

        def upload():
            a = pkg.Trace.upload_async(ctx, pin)
            a.wait()
            a.free()

        tc = median_ms(upload, args.steps)
        line("(c) Trace.upload_async + wait of the finished matrix, page-locked", tc)
        td = median_ms(lambda: PT.poseidon2_chiplet_trace(ledger, permute_batch=ctx.poseidon2_permute), args.steps)
        line("(d) the generator, permute_batch=ctx.poseidon2_permute (first run %.0f ms)" % first, td)
        print(f"  (a) / (c) = {ta[0] / tc[0]:.2f}: the build is {'BELOW' if ta[0] < tc[0] else 'NOT below'} the upload; (a) / (d) = {ta[0] / td[0]:.4f}", flush=True)
        del own, pin
    ctx.close()
    if not args.build_only:
        for value, what in (("0", "the lane-a-chain kernel on every level"), ("1048576", "the 16-lanes-a-chain kernel on every level")):
            print(f"the same with {what} (MH_P2C_GROUP_MAX_CHAINS={value}), a process of its own:", flush=True)
            env = dict(os.environ, MH_P2C_GROUP_MAX_CHAINS=value)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--build-only"], env=env, capture_output=True, text=True)
            print(out.stdout + (out.stderr[-2000:] if out.returncode else ""), flush=True)


if __name__ == "__main__":
    main()
