"""The bus-balance checker (Miden.check_balance, mh_check_balance_miden_traces) on the real Miden statement of tools/bench_check.py --
2^20 core / 2^20 chiplets / 2^18 Poseidon2 rows at the default 9250 iterations: balanced (screen, exact), one damaged message cell, a whole
damaged column -- next to the constraint screen and mh_prove_miden on the same inputs, in the same run.
    python tools/bench_balance.py [iterations=9250] [steps=3] [--exact-only]
Prints one JSON line: median milliseconds of each, device-resident traces (the uploads are not timed).  --exact-only runs the balanced
exact mode alone (for a kernel trace of that stage)."""
import os, sys, json, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
pkg = load_package()
from miden_vm_amd import core_air as CO
from miden_vm_amd.testing import core_trace

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if len(args) > 0 else 9250
steps = int(args[1]) if len(args) > 1 else 3
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


exact_ms, e2 = timed(lambda: m.check_balance(*traces, pv, aux, exact=True))
assert e2 == [], e2[:3]
out = {"log_heights": [t.log_n for t in traces], "balance_exact_ms": round(exact_ms, 2), "steps": steps}
if "--exact-only" not in sys.argv:
    screen_ms, e1 = timed(lambda: m.check_balance(*traces, pv, aux))
    assert e1 == []
    core = r["core"].copy()
    col = CO.STACK_TOP[1]
    core[1000, col] = (int(core[1000, col]) + 1) % pkg.P
    one = [ctx.upload_trace(core), traces[1], traces[2]]
    one_ms, e3 = timed(lambda: m.check_balance(*one, pv, aux))
    core[:, col] = (core[:, col] + 1) % pkg.P
    whole = [ctx.upload_trace(core), traces[1], traces[2]]
    col_ms, e4 = timed(lambda: m.check_balance(*whole, pv, aux))
    check_ms, e5 = timed(lambda: m.check(*traces, pv, aux))
    prove_ms, _ = timed(lambda: m.prove(*traces, pv, aux))
    assert e5 == []
    out.update({"balance_screen_ms": round(screen_ms, 2), "one_cell_ms": round(one_ms, 2), "one_cell_entries": len(e3),
                "one_cell_pushes": sum(e.pushes for e in e3), "whole_column_ms": round(col_ms, 2), "whole_column_entries": len(e4),
                "whole_column_pushes": sum(e.pushes for e in e4), "check_screen_ms": round(check_ms, 2), "prove_ms": round(prove_ms, 2)})
print(json.dumps(out), flush=True)
