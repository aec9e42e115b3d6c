"""Times the Keccak round and sponge traces built on the device (mh_keccak_traces_build, mh_keccak_round_trace_build,
csrc/keccak_traces.hip) next to the upload they replace and the example's device path.

Setup: 160 messages, 80 of 100 bytes (one block) and 80 of 300 bytes (three blocks): 320 permutations, the bench's own Keccak load --
2^19 round rows x 68, 2^14 sponge rows x 67.
  (a) keccak_traces from the messages + a fence (a one-state mh_poseidon2_permute, which ends in a stream synchronise);
  (b) keccak_round_trace from the 320 permutation inputs + fence;
  (c) the example's kt_keccak_round_trace (examples/keccak_trace_device.hip) on the same inputs: the device path there was before
      (it also counts the byte-pair table's multiplicities, allocates with hipMalloc and ends in a device synchronise);
  (d) Trace.upload_async + wait of the two finished, page-locked matrices: the transfer (a) replaces;
  (e) the device time of each kernel from the library's event profiler (mh_prof_*), in a pass of its own;
  (f) one message of --long-bytes bytes (default 10^6): a single wave walks its blocks one after the other, the serial worst case.
(a) .. (d) are medians of `--steps` runs after one warm-up run, host wall clock; (f) of three.  The device's traces are compared with
the generators (testing/precompile_trace.py) first.  Nothing is asserted about speed.

  python tools/bench_keccak_traces.py [--steps 7] > profiles/keccak_traces.txt"""
import argparse, ctypes as C, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

KERNELS = ("kt_offsets", "kt_absorb_permute", "kt_round_rows", "kt_sponge_rows")


def median_ms(fn, steps, after=None):
    """fn() timed; after(result) untimed"""
    ts = []
    for i in range(steps + 1):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if after:
            after(r)
        if i:
            ts.append(dt)
    return statistics.median(ts), min(ts), max(ts)


def line(name, t):
    print(f"  {name:<74s} median {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--long-bytes", type=int, default=1000000)
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    from miden_vm_amd import precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(23)
    msgs = [bytes(rng.integers(0, 256, 100 if i % 2 == 0 else 300, dtype=np.uint8)) for i in range(160)]
    sp = PT.SpongeRequires()
    heads = [sp.require(m)["chunk_head"] for m in msgs]
    states = np.array(sp.perm_inputs, dtype=np.uint64)
    exp_sponge, exp_round = PT.keccak_sponge_trace(sp), PT.keccak_round_trace(sp.perm_inputs)[0]
    print(f"mh_keccak_traces_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    print(f"{len(msgs)} messages, {sum(len(m) for m in msgs)} bytes, {len(states)} permutations: round trace {exp_round.shape[0]} x 68 "
          f"({exp_round.nbytes / 1e6:.0f} MB), sponge trace {exp_sponge.shape[0]} x 67 ({exp_sponge.nbytes / 1e6:.1f} MB)", flush=True)
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    rt, st, info = pkg.keccak_traces(ctx, msgs, heads)
    assert (rt.download() == exp_round).all() and (st.download() == exp_sponge).all() and info.n_perms == len(states)
    t = pkg.keccak_round_trace(ctx, states)
    assert (t.download() == exp_round).all()
    for x in (rt, st, t):
        x.free()

    def from_messages():
        r, s, _ = pkg.keccak_traces(ctx, msgs, heads)
        ctx.poseidon2_permute(one)
        r.free()
        s.free()

    def from_states():
        r = pkg.keccak_round_trace(ctx, states)
        ctx.poseidon2_permute(one)
        r.free()

    ta = median_ms(from_messages, args.steps)
    line("(a) keccak_traces from the messages + fence", ta)
    line("    the fence alone (one-state mh_poseidon2_permute)", median_ms(lambda: ctx.poseidon2_permute(one), args.steps))
    tb = median_ms(from_states, args.steps)
    line("(b) keccak_round_trace from the permutation inputs + fence", tb)

    tc = None
    so = os.path.join(ROOT, "examples", "libkeccak_trace_device.so")
    if os.path.exists(so):
        kt = C.CDLL(so)
        kt.kt_free.argtypes = [C.c_void_p]
        program = np.array(PA.keccak_round_slots(), dtype=np.int32)
        rcs = np.array(PA.KECCAK_RC, dtype=np.uint64)

        def example():
            tr, cnt, mem, lg = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
            rc = kt.kt_keccak_round_trace(states.ctypes.data_as(C.c_void_p), C.c_int(len(states)), rcs.ctypes.data_as(C.c_void_p),
                                          program.ctypes.data_as(C.c_void_p), C.byref(tr), C.byref(lg), C.byref(cnt), C.byref(mem))
            assert rc == 0
            return tr, cnt, mem

        tc = median_ms(example, args.steps, after=lambda r: [kt.kt_free(p) for p in r])
        line("(c) the example's kt_keccak_round_trace on the same inputs (frees untimed)", tc)
    else:
        print("  (c) examples/libkeccak_trace_device.so is not built: skipped", flush=True)

    pin_r, own_r = pkg.pinned_array(ctx.lib, exp_round.shape)
    pin_s, own_s = pkg.pinned_array(ctx.lib, exp_sponge.shape)
    pin_r[:], pin_s[:] = exp_round, exp_sponge

    def upload():
        a, b = pkg.Trace.upload_async(ctx, pin_r), pkg.Trace.upload_async(ctx, pin_s)
        a.wait()
        b.wait()
        a.free()
        b.free()

    td = median_ms(upload, args.steps)
    line("(d) Trace.upload_async + wait of both matrices, page-locked", td)
    print(f"  (a) / (d) = {ta[0] / td[0]:.2f}; (b) / (d) = {tb[0] / td[0]:.2f}" + (f"; (b) / (c) = {tb[0] / tc[0]:.2f}" if tc else ""), flush=True)

    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.steps):
        from_messages()
    prof = ctx.prof()
    ctx.prof_enable(False)
    print("  (e) device time per call of (a), event profiler:\n      "
          + ", ".join(f"{k} {prof[k]['ms'] / args.steps:.3f} ms" for k in KERNELS if k in prof), flush=True)

    long_msg = bytes(rng.integers(0, 256, args.long_bytes, dtype=np.uint8))
    blocks = len(long_msg) // 136 + 1

    def long_one():
        r, s, _ = pkg.keccak_traces(ctx, [long_msg], [0])
        ctx.poseidon2_permute(one)
        r.free()
        s.free()

    tf = median_ms(long_one, 3)
    line(f"(f) one message of {len(long_msg)} bytes, {blocks} blocks walked by one wave + fence", tf)
    ctx.prof_enable(True)
    ctx.prof_reset()
    long_one()
    prof = ctx.prof()
    ctx.prof_enable(False)
    print("      " + ", ".join(f"{k} {prof[k]['ms']:.3f} ms" for k in KERNELS if k in prof)
          + f"; kt_absorb_permute {1e3 * prof['kt_absorb_permute']['ms'] / blocks:.2f} us a block", flush=True)
    del own_r, own_s, pin_r, pin_s
    ctx.close()


if __name__ == "__main__":
    main()
