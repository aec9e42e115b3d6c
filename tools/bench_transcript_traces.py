"""Times the precompile prover's ChunkNode and TranscriptEval traces built on the device (mh_chunk_node_trace_build,
mh_transcript_eval_trace_build, csrc/transcript_traces.hip) next to the upload they replace and the generators that lay them today.

The workload is the edge ledger of tests/transcript_traces_cases.py scaled up: --claims Keccak claims of lengths i mod 300 (the empty
input repeats), a --chain-step uint_add chain closed by an `is`, 70 created points, P + pai is P, a 70-term MSM claimed in reversed
order, a pin, all folded under a zero leaf.  The Poseidon2 trace both builds read is built on the device from the ledger with digest
references before the clock starts (mh_poseidon2_chiplet_trace_build has its own table, profiles/poseidon2_chiplet.txt).

  (a) chunk_node_trace + transcript_eval_trace from the lists + a fence (a one-state mh_poseidon2_permute, which ends in a stream
      synchronise); the fence alone;
  (b) the device time of (a) per kernel, from the context's event profiler, in a pass of its own;
  (c) ctx.upload_trace of the two finished matrices (pageable numpy arrays: what a caller without these entries does);
  (d) Trace.upload_async + wait of the two matrices from page-locked memory: the fastest upload the library has;
  (e) the generators chunk_node_trace + transcript_eval_trace on the same ledgers; the Poseidon2 permutations the recording ran on the
      host for the digests these rows hold are counted and timed apart (one batched numpy call over as many states: a lower bound, the
      ledger runs them one by one).
All medians of --steps runs after a warm-up, host wall clock.  The device's traces are compared with the generators' cell for cell.

  python tools/bench_transcript_traces.py [--steps 7] [--claims 4000] [--chain 2000] > profiles/transcript_traces.txt"""
import argparse, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PHASES = ("cn_chunk_check", "cn_record_check", "cn_rows", "te_row_check", "te_read_check", "te_rows")


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


def ledger(PT, PA, n_claims, chain):
    fp, group, m = PA.K1_BASE_BOUND_PTR, PA.K1_GROUP_PTR, PA.K1_BOUND + 1
    s = PT.Session()
    claims = [s.keccak(bytes((7 * i + j) & 0xff for j in range(i % 300)))[1] for i in range(n_claims)]
    x = s.uint_leaf(PA.K1_G[0], fp)
    acc = x
    for _ in range(chain):
        acc = s.uint_add(acc, x)
    claims.append(s.uint_is(acc, s.uint_leaf((chain + 1) * PA.K1_G[0] % m, fp)))
    mult = PT.k1_multiples(70)
    pts = [s.ec_create(group, s.uint_leaf(px, fp), s.uint_leaf(py, fp)) for px, py in mult]
    claims.append(s.ec_is(s.ec_add(pts[4], s.ec_pai(group)), pts[4]))
    e = None
    for p in pts:
        intro = s.msm_intro(p)
        e = intro if e is None else s.msm_combine(e, intro)
    by_base = dict(s.msm.terms(e))
    node = s.ec_msm(e, [(p, s.eval.uint_leaf(by_base[p["point"]])) for p in reversed(pts)])
    vx, vy = s.msm_value_coords(e)
    claims.append(s.ec_is(node, s.ec_create(group, s.uint_leaf(vx, fp), s.uint_leaf(vy, fp))))
    claims.append(s.pin_uint(100, (PA.K1_G[0] * 3 + 1) % m, fp))
    return s, s.assert_and_fold(claims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--claims", type=int, default=4000)
    ap.add_argument("--chain", type=int, default=2000)
    args = ap.parse_args()
    assert args.steps >= 5
    pkg = load_package()
    from miden_vm_amd import miden_air as MA, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    ctx = pkg.Ctx(0)
    one = np.zeros((1, 12), dtype=np.uint64)
    t0 = time.perf_counter()
    s, root = ledger(PT, PA, args.claims, args.chain)
    t_ledger = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cn_lists, te_lists = PT.chunk_node_lists(s.chunk, s.node), PT.transcript_lists(s.eval, root)
    t_lists = (time.perf_counter() - t0) * 1e3
    absorptions, blocks, refs = s.p2.lists(refs=True)
    p2, p2info = pkg.poseidon2_chiplet_trace(ctx, np.array(absorptions, dtype=pkg.P2C_ABSORPTION_DTYPE).reshape(-1), blocks, refs)
    print(f"mh_chunk_node_trace_build + mh_transcript_eval_trace_build, measured: median of {args.steps} runs after a warm-up, host wall clock")
    cn, cinfo = ctx.chunk_node_trace(p2, *cn_lists)
    te, tinfo, public_root = ctx.transcript_eval_trace(p2, *te_lists)
    got = [cn.download(), te.download()]
    cn.free()
    te.free()
    list_bytes = sum(x.nbytes for x in cn_lists) + sum(x.nbytes for x in te_lists[:3])
    matrix_bytes = sum(g.nbytes for g in got)
    print(f"the edge ledger with {args.claims} Keccak claims and a chain of {args.chain}: {cinfo.n_records} records on {cinfo.n_chunks} chunk rows, "
          f"{tinfo.n_nodes} nodes on {tinfo.active_rows} active rows, {p2info.n_cycles} Poseidon2 cycles "
          f"({int((refs >= 0).sum())} halves are references); traces {got[0].shape[0]} x 42 and {got[1].shape[0]} x 39; lists {list_bytes / 1e6:.2f} MB "
          f"(bytes {cn_lists[0].nbytes} + digests {cn_lists[1].nbytes} + records {cn_lists[2].nbytes} + nodes {te_lists[0].nbytes} + terms {te_lists[1].nbytes} "
          f"+ literals {te_lists[2].nbytes} B) against matrices {matrix_bytes / 1e6:.2f} MB; recording the ledgers (host: Keccak and Poseidon2 in Python; "
          f"not part of the build) {t_ledger:.0f} ms, the lists {t_lists:.0f} ms", flush=True)

    def build():
        a, _ = ctx.chunk_node_trace(p2, *cn_lists)
        b, _, _ = ctx.transcript_eval_trace(p2, *te_lists)
        ctx.poseidon2_permute(one)
        a.free()
        b.free()

    ta = median_ms(build, args.steps)
    line("(a) chunk_node_trace + transcript_eval_trace from the lists + fence", ta)
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
    for _ in range(3):
        t0 = time.perf_counter()
        exp_te, exp_root = PT.transcript_eval_trace(s.eval, root)
        exp_cn = PT.chunk_node_trace(s.chunk, s.node)
        gen.append((time.perf_counter() - t0) * 1e3)
    exp = (exp_cn, exp_te)
    for name, g, e in zip(("chunk/node", "eval"), got, exp):
        assert g.shape == e.shape and (g == e).all(), f"the device's {name} trace differs from the generator's"
    assert public_root == exp_root
    print("  both traces and the public root equal the generators', cell for cell", flush=True)

    def upload():
        trs = [ctx.upload_trace(e) for e in exp]
        ctx.poseidon2_permute(one)
        for t in trs:
            t.free()

    tc = median_ms(upload, args.steps)
    line("(c) ctx.upload_trace of the two finished matrices + fence", tc)
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
    line("(d) Trace.upload_async + wait of the two matrices, page-locked", td)
    te_ = (statistics.median(gen), min(gen), max(gen))
    line("(e) the generators chunk_node_trace + transcript_eval_trace (3 runs)", te_)
    states = np.zeros((int(p2info.n_cycles), 12), dtype=np.uint64)
    line(f"    the {p2info.n_cycles} host permutations behind their digests, as ONE numpy batch", median_ms(lambda: MA.permute_batch(states), 3))
    print(f"  (a) / (c) = {ta[0] / tc[0]:.3f}, (a) / (d) = {ta[0] / td[0]:.3f}: the build is {'BELOW' if ta[0] < td[0] else 'NOT below'} the page-locked upload; "
          f"(a) / (e) = {ta[0] / te_[0]:.5f}", flush=True)
    del pins
    p2.free()
    ctx.close()


if __name__ == "__main__":
    main()
