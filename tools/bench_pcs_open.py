"""The standalone PCS (mh_pcs_*) at the bench size: the three trees of miden:LOG_N:51:8 at the production parameters
(main 51, aux 16, quotient 16 base columns, blowup 8) opened at N = 1, 2, 4 points, next to the STARK session's own two-point stages on
the SAME trees.
    python tools/bench_pcs_open.py [--log-n 20] [--reps 5]
Per N one JSON line: min / median / max milliseconds of evals() + deep() (wall clock around the blocking calls, after one warm-up),
of the whole mh_pcs_open, and the profiler's spans and kernel classes from a separate profiled pass.  The yardstick line is the session's
`span:evaluate at OOD points` + `span:DEEP quotient` measured the same way.  N = 2 uses the session's own points (z, z * w_N)."""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from __graft_entry__ import load_package

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
pkg = load_package()
from miden_vm_amd import dag, protocol

P = pkg.P
ctx = pkg.Ctx(0)
params, state = dict(protocol.PROD_PARAMS), protocol.challenger_state()
rng = np.random.default_rng(7)
host = rng.integers(0, P, (1 << args.log_n, 51), dtype=np.uint64)
host[:, 0] = 0
ef = lambda: (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))  # noqa: E731


def stats(ms):
    return dict(min=round(min(ms), 3), median=round(statistics.median(ms), 3), max=round(max(ms), 3))


def spans(names):
    prof = ctx.prof()
    return {k: round(prof[k]["ms"], 3) for k in names if k in prof}


def session_to_quotient():
    s = pkg.Session(ctx, [pkg.DeviceAir(ctx, dag.dummy_miden_air(51, 8))], [ctx.upload_trace(host)], [], params)
    s.commit_main()
    s.commit_aux([ef() for _ in range(s.shape.num_randomness)])
    s.commit_quotient(ef(), ef())
    return s


z = ef()
w = pow(1753635133440165772, 1 << (32 - args.log_n), P)
alpha, beta = ef(), ef()
# ---- the yardstick: the session's two-point stages (a session runs them once, so one session per repetition) ----
t_sess, sess_spans = [], None
for rep in range(args.reps + 2):
    profiled = rep == args.reps + 1
    s = session_to_quotient()
    assert s.ood_point_ok(z)
    if profiled:
        ctx.prof_enable(True)
        ctx.prof_reset()
    t0 = time.perf_counter()
    s.ood(z)
    s.deep(alpha, beta)
    dt = (time.perf_counter() - t0) * 1e3
    if profiled:
        sess_spans = spans(["span:evaluate at OOD points", "span:DEEP quotient", "deep_ood_eval", "deep_assemble", "deep_extend"])
        ctx.prof_enable(False)
    elif rep:
        t_sess.append(dt)
    if rep < args.reps + 1:
        s.free()
print(json.dumps(dict(what="session ood + deep (two points)", log_n=args.log_n, ms=stats(t_sess), profiled=sess_spans)), flush=True)

# ---- the standalone stages on the last session's trees ----
trees = s.trees()
extra = []
while len(extra) < 2:
    c = ef()
    if pkg.pcs_point_ok(args.log_n, params["log_blowup"], c):
        extra.append(c)
zw = (z[0] * w % P, z[1] * w % P)
for n, pts in ((1, [z]), (2, [z, zw]), (4, [z, zw] + extra)):
    t_stage, t_open, prof = [], [], None
    for rep in range(args.reps + 2):
        profiled = rep == args.reps + 1
        op = pkg.PcsOpening(ctx, trees, pts, params)
        if profiled:
            ctx.prof_enable(True)
            ctx.prof_reset()
        t0 = time.perf_counter()
        op.evals()
        op.deep(alpha, beta)
        dt = (time.perf_counter() - t0) * 1e3
        if profiled:
            prof = spans(["span:pcs evaluate at the points", "span:pcs DEEP quotient", "pcs_ood_eval", "pcs_deep_assemble", "pcs_deep_extend"])
            ctx.prof_enable(False)
        elif rep:
            t_stage.append(dt)
        op.free()
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        pkg.pcs_open(ctx, trees, pts, params, state, [])
        if rep:
            t_open.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what=f"pcs evals + deep, N = {n}", log_n=args.log_n, ms=stats(t_stage), whole_pcs_open_ms=stats(t_open), profiled=prof)),
          flush=True)
s.free()
ctx.close()
