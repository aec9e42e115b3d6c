"""Times the memory chiplet's trace section built on the device (mh_memory_section_build, csrc/memory_section.hip) next to the upload it
replaces and the host generator.

Setup: 2^20 accesses over 2^16 (ctx, word) pairs in 4 contexts, one access per cycle, every kind, in program order (48 MB as
mh_mem_access records); the section is 2^20 x 17 felts (143 MB).
  (a) memory_section from the host list.  The call returns after its second read-back with the rows kernel enqueued, so the wall clock
      is taken around the call plus a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise; timed alone as well);
  (b) Trace.upload_async + wait of the finished, page-locked 2^20 x 17 section: the transfer the call replaces;
  (c) testing/chiplets_trace.Memory.section() on the host for the same list, ONE run (a Python loop with one modular inverse per row:
      the TEST generator, not the reference's Rust);
  the device time of each kernel from the library's event profiler (mh_prof_*), in a pass of its own, with the number of sort passes
  that ran (a digit that is the same in every key is skipped).
The same figures for a list whose contexts, words and clocks spread over all their bits, so that all twelve passes run.
(a), (b) and the fence are medians of `--steps` runs after one warm-up run.  The device's section is compared with (c) first.
Nothing is asserted about speed.

  python tools/bench_memory_section.py [--steps 7] > profiles/memory_section.txt"""
import argparse, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

KERNELS = ("ms_keys", "ms_hist", "ms_table_scan", "ms_scatter", "ms_reduce", "ms_carries", "ms_rows")


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


def access_list(dtype, log_n, spread, seed=7):
    """2^log_n accesses over 2^(log_n - 4) (ctx, word) pairs in 4 contexts, clk = 1 + arrival index; spread: contexts, words and
    clocks take values over all their bits"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    words_per_ctx = max(1, n >> 6)
    a = np.zeros(n, dtype=dtype)
    ctxs = np.array([0x00000000, 0x5A5A5A5A, 0xA5A5A5A5, 0xFFFFFFFF] if spread else [0, 1, 2, 3], dtype=np.uint32)
    a["ctx"] = ctxs[rng.integers(0, 4, n)]
    w = rng.integers(0, words_per_ctx, n, dtype=np.uint64)
    if spread:
        w = (w * np.uint64(65521 * 8191)) % np.uint64(1 << 30)
    kind = rng.integers(0, 4, n).astype(np.uint32)
    a["addr"] = (w * np.uint64(4)).astype(np.uint32) + np.where(kind & 2, 0, rng.integers(0, 4, n)).astype(np.uint32)
    clk = np.arange(1, n + 1, dtype=np.uint64)
    a["clk"] = (clk * np.uint64(((1 << 32) - 1) >> log_n) if spread else clk).astype(np.uint32)
    a["kind"] = kind
    a["value"] = rng.integers(0, 1 << 64, (n, 4), dtype=np.uint64)
    return a


def sort_passes(a):
    hi = (a["ctx"].astype(np.uint64) << np.uint64(30)) | (a["addr"] >> np.uint32(2)).astype(np.uint64)
    vh = int(np.bitwise_or.reduce(hi) ^ np.bitwise_and.reduce(hi))
    vl = int(np.bitwise_or.reduce(a["clk"]) ^ np.bitwise_and.reduce(a["clk"]))
    return sum(1 for d in range(4) if (vl >> (8 * d)) & 255) + sum(1 for d in range(8) if (vh >> (8 * d)) & 255)


def host_section(CT, a):
    """-> (Memory.section() of the list, seconds the section() call took)"""
    m = CT.Memory()
    fns = (lambda c, ad, k, v: m.write(c, ad, k, v[0]), lambda c, ad, k, v: m.read(c, ad, k),
           lambda c, ad, k, v: m.write_word(c, ad, k, v), lambda c, ad, k, v: m.read_word(c, ad, k))
    for c, ad, k, kd, v in zip(a["ctx"].tolist(), a["addr"].tolist(), a["clk"].tolist(), a["kind"].tolist(), a["value"].tolist()):
        fns[kd](c, ad, k, v)
    t0 = time.perf_counter()
    sec = m.section()
    return sec, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    from miden_vm_amd.testing import chiplets_trace as CT
    log_n, n = args.log_n, 1 << args.log_n
    print(f"mh_memory_section_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    for spread in (False, True):
        a = access_list(pkg.MEM_ACCESS_DTYPE, log_n, spread)
        keys = np.unique((a["ctx"].astype(np.uint64) << np.uint64(30)) | (a["addr"] >> np.uint32(2)).astype(np.uint64)).size
        print(f"\n2^{log_n} accesses ({a.nbytes / 1e6:.0f} MB) over {keys} words in {np.unique(a['ctx']).size} contexts, "
              f"{'contexts, words and clocks spread over all their bits' if spread else 'clocks 1 .. 2^%d' % log_n}: "
              f"{sort_passes(a)} of 12 sort passes run; section 2^{log_n} x 17 ({n * 17 * 8 / 1e6:.0f} MB)", flush=True)
        sec, t_host = host_section(CT, a)
        t, info, _ = pkg.memory_section(ctx, a, log_n)
        assert (t.download() == sec).all() and info.n_words == keys, "the device's section differs from the generator's"
        t.free()
        pin, own = pkg.pinned_array(ctx.lib, sec.shape)
        pin[:] = sec

        def build(fence=True):
            t, _, _ = pkg.memory_section(ctx, a, log_n)
            if fence:
                ctx.poseidon2_permute(one)
            t.free()

        def upload():
            t = pkg.Trace.upload_async(ctx, pin)
            t.wait()
            t.free()

        line("(a) memory_section from the host list + fence", median_ms(build, args.steps))
        line("    the call alone (returns with the rows kernel enqueued)", median_ms(lambda: build(False), args.steps))
        line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
        line("(b) Trace.upload_async + wait, page-locked 2^%d x 17" % log_n, median_ms(upload, args.steps))
        print(f"  {'(c) Memory.section() on the host (test generator), one run':<74s}        {t_host * 1e3:9.0f} ms", flush=True)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(args.steps):
            build()
        prof = ctx.prof()
        ctx.prof_enable(False)
        print("    device time per call, event profiler (hist / table_scan / scatter: all passes together):\n      " + ", ".join(
            f"{name} {prof.get(name, {'ms': float('nan')})['ms'] / args.steps:.3f} ms" for name in KERNELS), flush=True)
        del own
    ctx.close()


if __name__ == "__main__":
    main()
