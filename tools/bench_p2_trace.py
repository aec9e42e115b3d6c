"""Times the Poseidon2 permutation trace built on the device (mh_miden_poseidon2_trace, csrc/p2_trace.hip) next to the upload it replaces.

Setup: chiplets_trace.bulk_chiplets(20, 20) -- 2^20 chiplets rows whose hasher controller requests 65 535 distinct permutations, and
the 2^20 x 16 Poseidon2 permutation trace that holds them (128 MB).
  (a) Trace.upload_async + wait of the page-locked 2^20 x 16 matrix: existing code, the baseline;
  (b) Miden.poseidon2_trace from the resident chiplets trace.  The call returns after its one read-back with the cycles kernel
      enqueued, so the wall clock is taken around the call plus a fence (a one-state mh_poseidon2_permute, which ends in a stream
      synchronise; timed alone as well).  The scan / check / cycles split comes from the library's event profiler (mh_prof_*) in a
      pass of its own;
  (c) Miden.prove from three host matrices (mh_prove_miden) against two uploads + the derived trace + mh_prove_miden_traces, under
      Poseidon2 and Blake3.  The core matrix is 2^20 x 51 uniform felts: no executed program with 2^20 Poseidon2 rows is at hand, the
      prover does not look at what a trace means, and the work is that of a real statement of this shape (the proof is not verified);
  (d) the numpy generator of the same trace (miden_air.poseidon2_permutation_trace) on the host: the TEST generator, not the
      reference's Rust.
Each figure is the median of `--steps` runs after one warm-up run.  The derived trace is compared with the generator's first.
Nothing is asserted about speed.

  python tools/bench_p2_trace.py [--steps 7] > profiles/p2_trace.txt"""
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
    print(f"  {name:<74s} median {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--no-prove", action="store_true", help="skip (c)")
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    from miden_vm_amd import miden_air as MA
    from miden_vm_amd.testing import chiplets_trace as CT
    log_n = args.log_n
    chip, p2 = CT.bulk_chiplets(log_n, log_n, seed=5)
    chip = np.ascontiguousarray(chip)
    k = (1 << log_n) // 16 - 1
    states, mults = p2[0::16][:k, MA.COL_STATE:MA.COL_STATE + 12].copy(), p2[0::16][:k, MA.COL_WITNESS].copy()
    print(f"mh_miden_poseidon2_trace, measured: median of {args.steps} runs after a warm-up, host wall clock")
    print(f"chiplets 2^{log_n} x 22, Poseidon2 permutation trace 2^{log_n} x 16 ({p2.nbytes / 1e6:.0f} MB), {k} requests\n")
    t_host = median_ms(lambda: MA.poseidon2_permutation_trace(log_n, states, mults), 5)

    ctx = pkg.Ctx(0)
    m = pkg.Miden(ctx)
    pin_p2, own_p2 = pkg.pinned_array(ctx.lib, p2.shape)
    pin_p2[:] = p2
    d_chip = ctx.upload_trace(chip)
    derived, info = m.poseidon2_trace(d_chip, log_n)
    assert (derived.download() == p2).all() and info.n_requests == k, "the derived trace differs from the generator's"
    derived.free()
    one = np.zeros((1, 12), dtype=np.uint64)

    def upload():
        t = pkg.Trace.upload_async(ctx, pin_p2)
        t.wait()
        t.free()

    def derive(fence=True):
        t, _ = m.poseidon2_trace(d_chip, log_n)
        if fence:
            ctx.poseidon2_permute(one)
        t.free()

    line("(a) Trace.upload_async + wait, page-locked 2^%d x 16" % log_n, median_ms(upload, args.steps))
    line("(b) Miden.poseidon2_trace + fence, chiplets resident", median_ms(derive, args.steps))
    line("    the call alone (returns with the cycles kernel enqueued)", median_ms(lambda: derive(False), args.steps))
    line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.steps):
        derive()
    prof = ctx.prof()
    ctx.prof_enable(False)
    print("    device time per call, event profiler: " + ", ".join(
        f"{name} {prof.get(name, {'ms': float('nan')})['ms'] / args.steps:.3f} ms" for name in ("p2t_scan", "p2t_check", "p2t_cycles")), flush=True)

    if not args.no_prove:
        try:
            core = np.random.default_rng(11).integers(0, pkg.P, (1 << log_n, 51), dtype=np.uint64)
            pv, aux_in = list(range(32)), [1, 2, 3, 4, 0, 0, 0, 0]

            def from_two(hash_fn):
                trs = [ctx.upload_trace(core), ctx.upload_trace(chip)]
                trs.append(m.poseidon2_trace(trs[1], log_n)[0])
                proof = m.prove(*trs, pv, aux_in, hash_fn=hash_fn)
                for t in trs:
                    t.free()
                return proof

            for hash_fn in ("poseidon2", "blake3"):
                assert m.prove(core, chip, p2, pv, aux_in, hash_fn=hash_fn).bytes == from_two(hash_fn).bytes
                line(f"(c) Miden.prove, three host matrices, {hash_fn}", median_ms(lambda: m.prove(core, chip, p2, pv, aux_in, hash_fn=hash_fn), args.steps))
                line(f"(c) two uploads + Miden.poseidon2_trace + Miden.prove, {hash_fn}", median_ms(lambda: from_two(hash_fn), args.steps))
        except Exception as e:  # (a), (b) and (d) stand without it
            print(f"  (c) not measured: {e!r}"[:300])
    line("(d) numpy miden_air.poseidon2_permutation_trace on the host (test generator)", t_host)
    del own_p2
    ctx.close()


if __name__ == "__main__":
    main()
