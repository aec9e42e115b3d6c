"""Times the hasher controller's trace section built on the device (mh_hasher_section_build, mh_miden_hasher_section,
csrc/hasher_section.hip) next to the upload it replaces.

Setup: lists whose sections have 2^20 controller rows (2^19 permutations; 2^20 x 20 felts = 168 MB):
  permutes     2^19 permute ops, all states distinct;
  merkle32     2^14 Merkle verifies of depth 32;
  mix          permutes, control blocks, basic blocks of 1..8 batches, verifies of depth 1..32 and updates of depth 1..16 in a seeded
               order, topped up with permutes to 2^19 permutations; a quarter of the ops is an earlier op listed again, so the share
               of repeated pre-states is known and printed;
  mix, sorted  the ops of `mix` ordered by their permutation count (ANOTHER section: its rows come in another order).  It shows
               whether the chains kernel depends on the order the chains arrive in: before k_hs_order laid them out by length on the
               device it did (2.98 ms against 1.91 ms), with it the two lists take the same time.
For each list:
  (a) hasher_section from the host list.  The call returns after its second read-back with the rows kernel enqueued, so the wall clock
      is taken around the call plus a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise; timed alone as well);
  (b) Trace.upload_async + wait of the finished, page-locked 2^20 x 20 section: the transfer the call replaces;
  (c) the device time of each kernel from the library's event profiler (mh_prof_*), in a pass of its own.
  (d) for `mix` at 2^--chain-log-n rows: Miden.hasher_section in place + Miden.poseidon2_trace + fence against uploading the finished
      chiplets trace and the finished third trace (16 rows per request).
(a), (b), (d) and the fence are medians of `--steps` runs after one warm-up run.  The head of the device's section is compared with the
rule (tests/hasher_section_ref.py) first.  Nothing is asserted about speed.

  python tools/bench_hasher_section.py [--steps 7] > profiles/hasher_section.txt"""
import argparse, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

KERNELS = ("hs_plan", "hs_carries", "hs_offsets", "hs_order", "hs_chains", "hs_insert", "hs_ranks", "hs_rows")


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


def perms_of(ops):
    k, c = ops["kind"], ops["count"].astype(np.int64)
    return np.where(k < 2, 1, np.where(k == 4, 2 * c, c))


def operands_of(ops):
    k, c = ops["kind"], ops["count"].astype(np.int64)
    return np.select([k == 0, k == 1, k == 2, k == 3], [12, 8, 8 * c, 4 + 4 * c], 8 + 4 * c)


def lay_out(dtype, kind, count, rng, repeat=0.0):
    """ops of the given kinds and counts with fresh 64-bit operands; a share `repeat` of them takes kind, count, index and operands of
    an earlier op instead"""
    n = len(kind)
    ops = np.zeros(n, dtype=dtype)
    ops["kind"], ops["count"] = kind, count
    depth = np.minimum(ops["count"], 63).astype(np.uint64)
    ops["index"] = np.where(ops["kind"] >= 3, rng.integers(0, 1 << 63, n, dtype=np.uint64) & ((np.uint64(1) << depth) - np.uint64(1)),
                            np.where(ops["kind"] == 1, rng.integers(0, 1 << 63, n, dtype=np.uint64), 0))
    need = operands_of(ops)
    ops["payload"] = np.cumsum(need) - need
    if repeat:
        again = np.nonzero(rng.random(n) < repeat)[0]
        again = again[again > 0]
        src = (rng.random(again.size) * again).astype(np.int64)      # an earlier op (which may itself be a repeat: processed in order)
        for i, s in zip(again.tolist(), src.tolist()):
            ops[i] = ops[s]
    return ops, rng.integers(0, 1 << 64, int(need.sum()), dtype=np.uint64)


def lists(dtype, log_rows, seed=11):
    rng = np.random.default_rng(seed)
    n_perms = 1 << (log_rows - 1)
    z = lambda n: np.zeros(n, dtype=np.uint32)  # noqa: E731
    yield "permutes", lay_out(dtype, z(n_perms), z(n_perms), rng)
    n = n_perms // 32
    yield "merkle32", lay_out(dtype, z(n) + 3, z(n) + 32, rng)
    m = n_perms // 8
    kind = rng.integers(0, 5, m).astype(np.uint32)
    count = np.select([kind < 2, kind == 2, kind == 3], [0, rng.integers(1, 9, m), rng.integers(1, 33, m)], rng.integers(1, 17, m)).astype(np.uint32)
    ops, felts = lay_out(dtype, kind, count, rng, repeat=0.25)
    keep = np.cumsum(perms_of(ops)) <= n_perms
    ops = ops[keep]
    top = n_perms - int(perms_of(ops).sum())
    extra = np.zeros(top, dtype=dtype)
    extra["payload"] = len(felts) + 12 * np.arange(top)
    order = rng.permutation(len(ops) + top)
    mix = np.concatenate([ops, extra])[order]
    felts = np.concatenate([felts, rng.integers(0, 1 << 64, 12 * top, dtype=np.uint64)])
    yield "mix", (mix, felts)
    yield "mix, sorted by length", (mix[np.argsort(perms_of(mix), kind="stable")], felts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--chain-log-n", type=int, default=17)
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    import hasher_section_ref as HR
    log_n = args.log_n
    print(f"mh_hasher_section_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    for name, (ops, felts) in lists(pkg.HASH_OP_DTYPE, log_n):
        t, info, _ = pkg.hasher_section(ctx, ops, felts, log_n)
        sec = t.download()
        t.free()
        head = 300
        hrows = HR.section(ops[:head], felts)[0]
        live = 2 * int(perms_of(ops[:head]).sum())
        assert (sec[:live] == hrows[:live]).all(), "the head of the device's section differs from the rule's"
        kinds = np.bincount(ops["kind"], minlength=5).tolist()
        print(f"\n{name}: {len(ops)} ops (kinds 0..4: {kinds}), {felts.size * 8 / 1e6:.0f} MB of operands + {ops.nbytes / 1e6:.1f} MB of ops -> "
              f"{info.n_rows} rows, {info.n_permutations} permutations, {info.n_requests} distinct pre-states "
              f"({100.0 * (1 - info.n_requests / info.n_permutations):.1f} % repeats), mrupdate_id {info.mrupdate_id}; longest chain "
              f"{int(np.where(ops['kind'] < 2, 1, ops['count']).max())}", flush=True)
        pin, own = pkg.pinned_array(ctx.lib, sec.shape)
        pin[:] = sec

        def build(fence=True):
            t, _, _ = pkg.hasher_section(ctx, ops, felts, log_n)
            if fence:
                ctx.poseidon2_permute(one)
            t.free()

        def upload():
            t = pkg.Trace.upload_async(ctx, pin)
            t.wait()
            t.free()

        line("(a) hasher_section from the host list + fence", median_ms(build, args.steps))
        line("    the call alone (returns with the rows kernel enqueued)", median_ms(lambda: build(False), args.steps))
        line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
        line("(b) Trace.upload_async + wait, page-locked 2^%d x 20" % log_n, median_ms(upload, args.steps))
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(args.steps):
            build()
        prof = ctx.prof()
        ctx.prof_enable(False)
        print("  (c) device time per call, event profiler (hs_carries: both scans; hs_ranks: flags + ranks; hs_insert with its memsets):\n      "
              + ", ".join(f"{k} {prof.get(k, {'ms': float('nan')})['ms'] / args.steps:.3f} ms" for k in KERNELS), flush=True)
        del own, pin, sec

    # (d) the chain
    cl = args.chain_log_n
    ops, felts = dict(lists(pkg.HASH_OP_DTYPE, cl))["mix"]
    m = pkg.Miden(ctx)
    n = 1 << cl
    chip_host = np.zeros((n, 22), dtype=np.uint64)
    chip_host[:, 0:5] = 1
    chip_host[:, 21] = np.arange(1, n + 1, dtype=np.uint64)
    chip = pkg.Trace(ctx, chip_host)
    info, _ = m.hasher_section(chip, ops, felts)
    third, p2info = m.poseidon2_trace(chip)
    assert p2info.n_requests == info.n_requests
    finished = [chip.download(), third.download()]
    third.free()
    pins = [pkg.pinned_array(ctx.lib, f.shape) for f in finished]
    for (p, _), f in zip(pins, finished):
        p[:] = f
    print(f"\n(d) the chain at 2^{cl} controller rows (mix): {info.n_requests} requests -> third trace 2^{p2info.log_n} x 16 "
          f"({finished[1].nbytes / 1e6:.0f} MB), chiplets 2^{cl} x 22 ({finished[0].nbytes / 1e6:.0f} MB)", flush=True)

    def chain():
        m.hasher_section(chip, ops, felts)
        t, _ = m.poseidon2_trace(chip)
        ctx.poseidon2_permute(one)
        t.free()

    def upload_both():
        ts = [pkg.Trace.upload_async(ctx, p) for p, _ in pins]
        for t in ts:
            t.wait()
        for t in ts:
            t.free()

    line("    Miden.hasher_section in place + Miden.poseidon2_trace + fence", median_ms(chain, args.steps))
    line("    Trace.upload_async + wait of both finished traces, page-locked", median_ms(upload_both, args.steps))
    m.free()
    ctx.close()


if __name__ == "__main__":
    main()
