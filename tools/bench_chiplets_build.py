"""Times the whole chiplets trace built on the device from the five lists (mh_miden_chiplets_build, csrc/chiplets_build.hip and the five
section builders) next to the upload it replaces.

Setup: lists that fill 2^--log-n rows (default 2^20): half of the rows hasher controller rows (the `mix` of
tools/bench_hasher_section.py), 2^14 bitwise operations (2^17 rows), the rest less the ACE, kernel and padding rows memory accesses (the
dense list of tools/bench_memory_section.py, cut to size), ONE verifier-shaped ACE evaluation -- the constraint-evaluation circuit of the
three-AIR statement as tests/ace_codegen.py builds it, over random inputs, closed to zero -- and a 16-procedure kernel with 1000 calls.
  (a) Miden.chiplets_build from the host lists + a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise);
  (b) Trace.upload_async + wait of the finished, page-locked 2^log_n x 22 matrix: the transfer the call replaces;
  (c) the five standalone builders called alone, each with a fence, and their sum;
  (d) the device time of each kernel from the library's event profiler (mh_prof_*), in a pass of its own;
  (e) the ACE builder alone on the verifier-shaped circuit: gates, rounds (n_rounds) and the evaluate kernel's time.
(a), (b), (c) are medians of `--steps` runs after one warm-up run, host wall clock.  The device's trace is compared with the rules
(tests/*_section_ref.py, chiplets_frame_ref.py) on the bitwise, ACE and kernel-ROM sections and the frame first.  Nothing is asserted
about speed.

  python tools/bench_chiplets_build.py [--steps 7] > profiles/chiplets_build.txt"""
import argparse, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402

KERNELS = ("hs_plan", "hs_carries", "hs_offsets", "hs_order", "hs_chains", "hs_insert", "hs_ranks", "hs_rows", "bw_rows", "ms_keys", "ms_hist",
           "ms_table_scan", "ms_scatter", "ms_reduce", "ms_carries", "ms_rows", "ace_plan", "ace_gates", "ace_eval", "ace_rows", "kr_sort", "kr_calls",
           "kr_rows", "cb_frame")


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


def verifier_circuit(AR, seed=3):
    """The three-AIR constraint-evaluation circuit (tests/ace_codegen.py) as one evaluation over random inputs, closed to zero."""
    import ace_codegen as AC
    from miden_vm_amd import dag, core_air as CO, chiplets_air as CA, miden_air as MA
    airs = [dag.parse_air_blob(a.blob) for a in (CO.core_air()[0], CA.chiplets_air()[0], MA.poseidon2_permutation_air(num_public=32)[0])]
    built = AC.build_multi_air_circuit(airs, [0, 1, 2])
    rng = np.random.default_rng(seed)
    inputs, wire, const_at = [], {}, {}

    def const(v):
        if v not in const_at:
            const_at[v] = len(inputs)
            inputs.append(v)
        return ("i", const_at[v])

    nodes = built["nodes"]
    for i, n in enumerate(nodes):                      # inputs first: READ wires come before every gate
        if n[0] == "in":
            wire[i] = ("i", len(inputs))
            inputs.append((int(rng.integers(0, AR.P, dtype=np.uint64)), int(rng.integers(0, AR.P, dtype=np.uint64))))
        elif n[0] == "c":
            wire[i] = const(tuple(n[1]) if isinstance(n[1], (tuple, list)) else (int(n[1]), 0))
    zero = const((0, 0)) if any(n[0] == "neg" for n in nodes) else None
    c = AR.Circuit(inputs)
    for i, n in enumerate(nodes):
        if n[0] == "neg":
            wire[i] = c.gate(AR.SUB, zero, wire[n[1]])
        elif n[0] in ("add", "sub", "mul"):
            wire[i] = c.gate({"add": AR.ADD, "sub": AR.SUB, "mul": AR.MUL}[n[0]], wire[n[1]], wire[n[2]])
    assert wire[built["root"]] == ("g", len(c.gates) - 1)
    return c.close(), built


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    args = ap.parse_args()
    assert args.steps >= 5 and args.log_n >= 16
    pkg = load_package()
    import ace_section_ref as AR, bitwise_section_ref as BR, kernel_rom_section_ref as KR, chiplets_frame_ref as FR
    import bench_hasher_section as BH, bench_memory_section as BM
    log_n, n = args.log_n, 1 << args.log_n
    rng = np.random.default_rng(17)
    hash_ops, hash_felts = dict(BH.lists(pkg.HASH_OP_DTYPE, log_n - 1))["mix"]
    h_rows = (2 * int(BH.perms_of(hash_ops).sum()) + 7) & ~7
    n_bw = 1 << (log_n - 6)
    bw = np.zeros(n_bw, dtype=pkg.BITWISE_OP_DTYPE)
    bw["op"], bw["a"], bw["b"] = rng.integers(0, 2, n_bw), rng.integers(0, 1 << 32, n_bw, dtype=np.uint32), rng.integers(0, 1 << 32, n_bw, dtype=np.uint32)
    circuit, built = verifier_circuit(AR)
    ace_evals, ace_felts = AR.make_list([circuit], ptr=1 << 20, clk0=7)
    ace_rows = int(ace_evals["num_vars"][0]) // 2 + int(ace_evals["num_eval"][0])
    procs = rng.integers(0, 1 << 64, (16, 4), dtype=np.uint64)
    calls = procs[rng.integers(0, 16, 1000)]
    n_mem = n - 1 - h_rows - 8 * n_bw - ace_rows - 16
    mem = BM.access_list(pkg.MEM_ACCESS_DTYPE, log_n - 1, spread=False)[:n_mem]
    assert len(mem) == n_mem > 0
    lists = dict(hash_ops=hash_ops, hash_felts=hash_felts, bitwise_ops=bw, mem_accesses=mem, ace_evals=ace_evals, ace_felts=ace_felts,
                 kernel_procs=procs, kernel_calls=calls)
    print(f"mh_miden_chiplets_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    print(f"lists for 2^{log_n} rows: hasher {len(hash_ops)} ops -> {h_rows} rows, bitwise {n_bw} ops -> {8 * n_bw} rows, memory {n_mem} accesses, "
          f"ACE 1 evaluation of {int(ace_evals['num_vars'][0])} inputs and {int(ace_evals['num_eval'][0])} gates -> {ace_rows} rows "
          f"(the circuit: {built['ops']} operations, {built['constants']} constants), kernel 16 procedures, 1000 calls; "
          f"{sum(v.nbytes for v in lists.values()) / 1e6:.0f} MB of lists against {n * 22 * 8 / 1e6:.0f} MB of trace", flush=True)
    ctx = pkg.Ctx(0)
    m = pkg.Miden(ctx)
    one = np.zeros((1, 12), dtype=np.uint64)
    t, info = m.chiplets_build(lists, log_n)
    assert info.trace_len == n, info
    got = t.download()
    t.free()
    st = list(info.start)
    for s, rows in ((1, BR.section(bw)[0]), (3, AR.section(ace_evals, ace_felts)[0]), (4, KR.section(procs, calls)[0])):
        ones, col0, width = FR.LAYOUT[s]
        part = got[st[s]:st[s] + rows.shape[0]]
        assert (part[:, col0:col0 + width] == rows).all() and (part[:, :ones] == 1).all() and not part[:, ones].any(), f"section {s} differs from its rule"
    assert (got[:, 21] == np.arange(1, n + 1, dtype=np.uint64)).all() and (got[n - 1, 0:5] == 1).all() and not got[n - 1, 5:21].any()
    _, ace_ref = AR.section(ace_evals, ace_felts)
    assert info.ace.n_rounds == ace_ref["n_rounds"]
    pin, own = pkg.pinned_array(ctx.lib, got.shape)
    pin[:] = got

    def build():
        t, _ = m.chiplets_build(lists, log_n)
        ctx.poseidon2_permute(one)
        t.free()

    def upload():
        t = pkg.Trace.upload_async(ctx, pin)
        t.wait()
        t.free()

    def alone(fn):
        def run():
            fn()[0].free()
            ctx.poseidon2_permute(one)
        return run

    ta = median_ms(build, args.steps)
    line("(a) Miden.chiplets_build from the host lists + fence", ta)
    line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
    tb = median_ms(upload, args.steps)
    line("(b) Trace.upload_async + wait, page-locked 2^%d x 22" % log_n, tb)
    parts = [("hasher_section", alone(lambda: pkg.hasher_section(ctx, hash_ops, hash_felts))), ("bitwise_section", alone(lambda: pkg.bitwise_section(ctx, bw))),
             ("memory_section", alone(lambda: pkg.memory_section(ctx, mem))), ("ace_section", alone(lambda: pkg.ace_section(ctx, ace_evals, ace_felts))),
             ("kernel_rom_section", alone(lambda: pkg.kernel_rom_section(ctx, procs, calls)))]
    total = 0.0
    for name, fn in parts:
        tm = median_ms(fn, args.steps)
        total += tm[0]
        line(f"(c) {name} alone (its own trace) + fence", tm)
    print(f"  (c) the sum of the five medians: {total:.3f} ms; (a) / (b) = {ta[0] / tb[0]:.2f}", flush=True)
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.steps):
        build()
    prof = ctx.prof()
    ctx.prof_enable(False)
    print("  (d) device time per call, event profiler (kr_sort runs twice a call; memsets inside their scopes):\n      "
          + ", ".join(f"{k} {prof[k]['ms'] / args.steps:.3f} ms" for k in KERNELS if k in prof), flush=True)
    print(f"  (e) the verifier-shaped circuit: {info.ace.n_gates} gates in {info.ace.n_rounds} rounds "
          f"({info.ace.n_gates / max(1, info.ace.n_rounds):.2f} gates a round, {-(-int(info.ace.n_gates) // 64)} windows); "
          f"ace_eval {prof['ace_eval']['ms'] / args.steps:.3f} ms" if "ace_eval" in prof else "", flush=True)
    del own, pin
    m.free()
    ctx.close()


if __name__ == "__main__":
    main()
