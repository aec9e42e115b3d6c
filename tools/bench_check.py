"""The constraint checker (Miden.check, mh_check_miden_traces) on the real Miden statement of tools/bench_miden_real.py -- 2^20 core /
2^20 chiplets / 2^18 Poseidon2 rows at the default 9250 iterations -- in screen and exact mode, next to mh_prove_miden on the same inputs.
    python tools/bench_check.py [iterations=9250] [steps=3]
Prints one JSON line: median milliseconds of each, device-resident traces (the uploads are not timed)."""
import os, sys, json, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
pkg = load_package()
from miden_vm_amd.testing import core_trace

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 9250
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx = pkg.Ctx(0)
r = core_trace.prove_inputs(core_trace.CoreVM(stack_inputs=list(range(16))), core_trace.bench_program(iters))
m = pkg.Miden(ctx)
traces = [ctx.upload_trace(r[k]) for k in ("core", "chiplets", "poseidon2")]
pv, aux = r["public_values"], r["aux_inputs"]


def timed(fn):
    fn()  # warm-up: kernels loaded, pools filled
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


screen_ms, e1 = timed(lambda: m.check(*traces, pv, aux))
exact_ms, e2 = timed(lambda: m.check(*traces, pv, aux, exact=True))
prove_ms, _ = timed(lambda: m.prove(*traces, pv, aux))
assert e1 == [] and e2 == [], (e1, e2)
print(json.dumps({"log_heights": [t.log_n for t in traces], "check_screen_ms": round(screen_ms, 2), "check_exact_ms": round(exact_ms, 2),
                  "prove_ms": round(prove_ms, 2), "screen_over_prove": round(screen_ms / prove_ms, 3), "steps": steps}), flush=True)
