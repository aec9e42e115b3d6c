#!/usr/bin/env python3
"""bench.py -- trace rows/s of the MI355X proving hot path (BASELINE.json metric).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 the driver launches one rank per GPU with
torch.distributed.run.  One JSON line on rank 0.

A "step" = one complete proof (`prove`, crates/lifted-stark/src/prover/mod.rs:230-578) of the miden-bench synthetic instance
`miden:LOG_N:51:8` (benches/miden-bench: DummyMidenAir, 51 main columns + 8 EF aux columns) with the production PCS
parameters (air/src/config.rs:54-67) and the Poseidon2 LMCS + challenger, the trace already resident in HBM.

  N = 1   LOG_N = 20 (BASELINE.json configs[1], the configuration the metric is quoted on), one GPU.
  N > 1   ONE proof of LOG_N = 24 (configs[3]) sharded by cosets over the N GPUs: `mh_prove_sharded` with the communicator
          inside the library (csrc/comm_rccl.cpp: RCCL collectives on the prover's own stream), "scaling": "strong" -- the
          north-star scenario.  value = 2^24 rows / seconds per proof.  If the in-library RCCL communicator cannot be set
          up on the node, the torch.distributed communicator is used; if no sharded proof can be made at all, the line
          falls back to N independent proofs and says so ("scaling": "weak", config.fallback).

value = rows of the proved trace / seconds per step, whole job.  A plain run sets up, warms up, times the K steps and prints
the line (`metric`, `value`, `unit`, `ms_per_step`, `config`, ...); `--dump-outputs DIR` also writes the proof of the last
timed step as .npy files (see dump_outputs).  Everything else below is measured with `--full` only.

With `--full`: the CPU oracle is used ONLY for the `cpu_baseline` leg (a
bounded sample), never inside the timed GPU region.  Extra keys on the N = 1 line: `h2d_inclusive` (SURVEY.md section 8(d):
the same proof with the host->device upload of the trace inside the timed region) and `miden_shape` (the full Miden VM
shape: three AIRs of widths 51/22/16 with 4/3/1 EF aux columns, the published reference figure's neighbour) and `in_flight`
(three proofs in flight on the one GPU, one context per proving thread: service throughput, not the headline) and
`hash_configs` (the same proof under the reference's other hash functions: Blake3_256 = its default, Keccak, RPO, RPX).
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts (RCCL, cross-process buffers)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec


GEN_NOTE = ("Python TEST generator (miden-vm_amd/testing/precompile_trace.py: the reference builds these matrices in precompiles-prover/src/**/trace.rs), "
            "not product; excluded from every rate")


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def synth_trace(rng, log_n, width):
    """DummyMidenAir trace shape (crates/lifted-stark/src/testing/airs/miden.rs:105-124): column 0 all-zero, the rest uniform
    in [0, p).  Seeded numpy PCG64 (SmallRng is not reproducible here)."""
    import numpy as np
    P = 0xFFFFFFFF00000001
    t = rng.integers(0, P, (1 << log_n, width), dtype=np.uint64)
    t[:, 0] = 0
    return t


class ProveRunner:
    """One GPU, one proof of miden:LOG_N:51:8 per step."""

    def __init__(self, pkg, ctx, log_n, seed):
        import numpy as np
        from miden_vm_amd import dag, protocol
        self.pkg, self.ctx, self.log_n = pkg, ctx, log_n
        self.air = dag.dummy_miden_air(51, 8)
        self.dair = pkg.DeviceAir(ctx, self.air)
        self.host_trace = synth_trace(np.random.default_rng(seed), log_n, 51)
        self.trace = ctx.upload_trace(self.host_trace)
        self.params = dict(protocol.PROD_PARAMS)
        self.state = protocol.challenger_state()
        self.pre = protocol.protocol_pre_observe(self.params, [])
        self.proof = None

    def step(self):
        self.proof = self.pkg.prove(self.ctx, [self.dair], [self.trace], [], self.params, self.state, self.pre, None)

    def step_with_upload(self, pinned):
        # mh_trace_upload_async: DMA + transpose on the copy stream, the proof's first kernel waits for them on the GPU
        t = self.pkg.Trace.upload_async(self.ctx, pinned)
        self.proof = self.pkg.prove(self.ctx, [self.dair], [t], [], self.params, self.state, self.pre, None)
        t.free()

    def step_with_cols_upload(self, pinned_cols):
        # mh_trace_upload_cols_async: a COLUMN-major host matrix, eight columns per copy, the LDE of a group waits for that group only
        t = self.pkg.Trace.upload_cols_async(self.ctx, pinned_cols)
        self.proof = self.pkg.prove(self.ctx, [self.dair], [t], [], self.params, self.state, self.pre, None)
        t.free()

    def leaf_permutations_per_step(self):
        return (8 << self.log_n) * (7 + 2 + 2)  # main 51, aux 16, quotient 16 columns, 8 felts per permutation


class ShardedRunner:
    """N GPUs, ONE proof of miden:LOG_N:51:8 per step, sharded by cosets (every rank holds the trace: same seed)."""

    def __init__(self, pkg, ctx, log_n, comm):
        import numpy as np
        from miden_vm_amd import dag, protocol, sharding
        self.pkg, self.ctx, self.log_n, self.comm, self.sharding = pkg, ctx, log_n, comm, sharding
        self.air = dag.dummy_miden_air(51, 8)
        self.dair = pkg.DeviceAir(ctx, self.air)
        # every rank holds the (same, seeded) host matrix; each moves 1/N of its rows over its own PCIe link, the rest arrives over xGMI
        self.trace = sharding.upload_trace_sharded(pkg, ctx, comm, synth_trace(np.random.default_rng(7), log_n, 51))
        self.params = dict(protocol.PROD_PARAMS)
        self.state = protocol.challenger_state()
        self.pre = protocol.protocol_pre_observe(self.params, [])
        self.proof = None

    def step(self):
        self.proof = self.sharding.prove_sharded(self.pkg, self.ctx, self.comm, [self.dair], [self.trace], [], self.params, self.state,
                                                 self.pre, None)


def roofline(prof, pmc_file):
    """Dominant kernel of the timed region: algorithmic bytes per launch (attributed inside the library next to the launch)
    over the average launch duration (HIP events on the library's stream)."""
    if not prof:
        return None
    name = max((k for k in prof if not k.startswith(("comm_", "span:")) and k != "lde_intt"), key=lambda k: prof[k]["ms"])  # lde_intt is nested in lde
    e = prof[name]
    ach = (e["bytes"] / 1e9) / (e["ms"] / 1e3)
    traffic = None
    try:  # HBM bytes per launch from the committed rocprofv3 PMC passes of this build (profiles/), if they describe this kernel
        t = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
        if t.get("kernel") == name and abs(t["hbm_bytes_per_launch"] / (e["bytes"] / max(1, e["count"])) - 1) < 0.5:
            traffic = t["hbm_bytes_per_launch"]
    except Exception:
        pass
    return {"kernel": name, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "traffic": traffic, "avg_launch_ms": e["ms"] / max(1, e["count"]), "alg_bytes_per_launch": e["bytes"] / max(1, e["count"]),
            "note": "Poseidon2 hashing is integer-VALU bound (no 64-bit multiplier on CDNA4): see roofline_valu and DESIGN.md section 3"}


def valu_roofline(ctx, prof, perms, steps, pmc_json=None):
    """The bound the hash kernels actually live on: VALU issue.  On gfx950 every VALU instruction of this integer code
    (v_mad_u64_u32, the carry-chain VOP3 forms, v_lshl_add_u64, shifts) issues in 4 cycles per wave per SIMD (tools/permbench,
    tools/instbench).  peak = SIMDs x max shader clock x 64 lanes / (issue cycles of the instruction sequence of one permutation):
    506 field multiplications (472 S-box + 22 round-scale + 12 de-scale) of 13 VALU instructions + the linear layers as they
    stand in the ISA of p2f_permute (counted per basic block x trip count: DESIGN.md section 3).  It is the ceiling of THIS
    instruction sequence -- a shorter sequence raises it (round 3 went 10 953 -> 9 967) -- so the register-only rate of the code
    and the instruction count are reported next to it."""
    out = {"kernel": "lmcs_leaf_absorb", "bound": "valu", "unit": "Gperm/s"}
    ach = perms / (prof["lmcs_leaf_absorb"]["ms"] / steps * 1e-3)
    out["achieved"] = ach / 1e9
    try:
        out["register_rate"] = ctx.poseidon2_register_rate() / 1e9
    except Exception as e:  # pragma: no cover
        out["register_rate_error"] = repr(e)[:120]
    # Issue cost per instruction class (tools/instbench, profiles/r01_microbench.txt, relative to each other): v_mad_u64_u32, the VOP3
    # carry-chain forms (v_add_co / v_addc_co / v_subb_co with SGPR carries), v_lshl_add_u64 and 64-bit shifts all cost the same slot
    # (1.86-2.00 ns in the microbenchmark = the 4 cycles the permutation measures); only carry-less 32-bit VOP1/VOP2 (v_mov,
    # v_cndmask, v_and, v_add_u32) are cheaper (1.26 ns = 0.65 of a slot): 2.4 % of the dynamic mix (cndmask of the folds and of the final canonicalisation).
    N_MUL, MUL_VALU, LIN_VALU, SIMDS, MAX_CLOCK_GHZ = 506, 13, 3389, 1024, 2.4
    CYC_WIDE, CYC_PLAIN, PLAIN_SHARE = 4.0, 2.6, 0.024
    isa_valu = N_MUL * MUL_VALU + LIN_VALU
    cycles = isa_valu * ((1 - PLAIN_SHARE) * CYC_WIDE + PLAIN_SHARE * CYC_PLAIN)
    out["peak"] = SIMDS * MAX_CLOCK_GHZ * 64 / cycles
    out["frac"] = out["achieved"] / out["peak"]
    measured = None
    try:
        measured = json.load(open(os.path.join(ROOT, "profiles", pmc_json))).get("valu_per_permutation_SQ_INSTS_VALU") if pmc_json else None
    except (OSError, ValueError):
        pass
    out["valu_per_permutation"] = {"isa_count_p2f_permute": isa_valu, "round2_isa_count": 10953, "measured_SQ_INSTS_VALU_leaf_kernel": measured,
                                   "issue_cycles_by_class": {"mad_u64_u32 / carry-chain VOP3 / 64-bit add, shift": CYC_WIDE, "plain 32-bit VOP1/VOP2": CYC_PLAIN},
                                   "plain_share_of_dynamic_mix": PLAIN_SHARE}
    out["peak_basis"] = (f"{SIMDS} SIMDs x {MAX_CLOCK_GHZ} GHz (max clock) x 64 lanes / ({isa_valu} VALU: {100 * (1 - PLAIN_SHARE):.1f} % at {CYC_WIDE:.0f} issue "
                         f"cycles, {100 * PLAIN_SHARE:.1f} % at {CYC_PLAIN}); measured clock under this load 2.24-2.35 GHz (s_memtime)")
    return out


def in_flight_probe(pkg, log_n, device, k=3, steps=4):
    """Service throughput: k proofs in flight on the one GPU, each proving thread with its own context (its own HIP stream).
    The latency-bound stretches of one proof (tree tops of a few waves, FRI tail, Fiat-Shamir round trips) are filled by the
    kernels of the others.  NOT the headline: `value` stays the rate of one proof at a time."""
    import threading
    ctxs = [pkg.Ctx(device) for _ in range(k)]
    runners = [ProveRunner(pkg, c, log_n, 11 + i) for i, c in enumerate(ctxs)]
    for r in runners:
        r.step()
    bar = threading.Barrier(k + 1)

    def work(r):
        bar.wait()
        for _ in range(steps):
            r.step()
        bar.wait()

    th = [threading.Thread(target=work, args=(r,)) for r in runners]
    for t in th:
        t.start()
    bar.wait()
    t0 = time.perf_counter()
    bar.wait()
    dt = time.perf_counter() - t0
    for t in th:
        t.join()
    for r in runners:
        r.trace.free()
        r.dair.free()
    for c in ctxs:
        c.close()
    return {"proofs_in_flight": k, "proofs": k * steps, "value": k * steps * (1 << log_n) / dt, "unit": "trace rows/s",
            "ms_per_proof_amortised": dt / (k * steps) * 1e3,
            "note": "k proving threads, one context (HIP stream) each, same GPU; every proof is a complete independent proof"}


def in_flight_h2d_probe(pkg, log_n, device, k=3, steps=6):
    """The service loop with EVERY proof's host->device upload inside the timed region: k proving threads, each with its own
    context and its own page-locked host trace (the reference's hand-over: a host RowMajorMatrix, prover/src/lib.rs:317-355).  A
    thread keeps TWO traces in flight: the upload of proof j+1 (mh_trace_upload_async: DMA + transpose on the context's copy stream)
    is issued before mh_prove of proof j, so the 7.5 ms DMA rides under proof j's kernels (the SDMA engine does not slow a VALU-bound
    kernel, profiles/r03_h2dbench.txt); `steps` uploads and `steps` proofs per thread lie inside the timed region, the first upload
    of every thread exposed."""
    import threading
    ctxs = [pkg.Ctx(device) for _ in range(k)]
    runners = [ProveRunner(pkg, c, log_n, 31 + i) for i, c in enumerate(ctxs)]
    pins = []
    for r in runners:
        r.trace.free()
        pin, owner = pkg.pinned_array(r.ctx.lib, r.host_trace.shape)
        pin[:] = r.host_trace
        pins.append((pin, owner))
        r.step_with_upload(pin)
    bar = threading.Barrier(k + 1)

    def work(r, pin):
        bar.wait()
        nxt = pkg.Trace.upload_async(r.ctx, pin)
        for i in range(steps):
            cur, nxt = nxt, (pkg.Trace.upload_async(r.ctx, pin) if i + 1 < steps else None)
            r.proof = pkg.prove(r.ctx, [r.dair], [cur], [], r.params, r.state, r.pre, None)
            cur.free()
        bar.wait()

    th = [threading.Thread(target=work, args=(r, p[0])) for r, p in zip(runners, pins)]
    for t in th:
        t.start()
    bar.wait()
    t0 = time.perf_counter()
    bar.wait()
    dt = time.perf_counter() - t0
    for t in th:
        t.join()
    for r in runners:
        r.dair.free()
    for c in ctxs:
        c.close()
    return {"proofs_in_flight": k, "proofs": k * steps, "value": k * steps * (1 << log_n) / dt, "unit": "trace rows/s",
            "ms_per_proof_amortised": dt / (k * steps) * 1e3, "upload_bytes_per_proof": int(runners[0].host_trace.nbytes),
            "note": "every proof = upload of its 2^%d x 51 row-major host trace (page-locked) + transpose + complete proof, all inside the "
                    "timed region; k proving threads, one context each, same GPU; per thread the upload of proof j+1 is in flight under "
                    "proof j" % log_n}


def jit_load_probe(pkg, ctx):
    """mh_air_load of the three real Miden AIRs: cold (empty cache directory: hiprtc compiles every chunk) and cached (code objects
    from disk).  A prover service runs tools/jit_precompile.py at build time (mh_jit_precompile needs no GPU), so its request path
    only ever sees the cached figure."""
    import shutil, tempfile
    from miden_vm_amd import miden_air, chiplets_air, core_air
    out = {}
    old = os.environ.get("MH_JIT_CACHE_DIR")
    for name, air in (("poseidon2_permutation", miden_air.poseidon2_permutation_air(num_public=32)[0]), ("chiplets", chiplets_air.chiplets_air()[0]),
                      ("core", core_air.core_air()[0])):
        tmp = tempfile.mkdtemp(prefix="mh_jit_cold_")
        try:
            os.environ["MH_JIT_CACHE_DIR"] = tmp
            ro, os.environ["MH_JIT_CACHE_RO_DIR"] = os.environ.get("MH_JIT_CACHE_RO_DIR", ""), ""   # cold = not even the shipped kernels
            t0 = time.perf_counter()
            d = pkg.DeviceAir(ctx, air)
            cold = time.perf_counter() - t0
            d.free()
            t0 = time.perf_counter()
            d = pkg.DeviceAir(ctx, air)
            cached = time.perf_counter() - t0
            out[name] = {"dag_nodes": int(air.blob[8]), "constraints": int(air.blob[9]), "chunks": d.compiled_chunks, "max_vgprs": d.compiled_max_vgprs,
                         "jit_cold_s": round(cold, 2), "jit_cached_ms": round(cached * 1e3, 2)}
            d.free()
        finally:
            os.environ["MH_JIT_CACHE_RO_DIR"] = ro
            if old is None:
                os.environ.pop("MH_JIT_CACHE_DIR", None)
            else:
                os.environ["MH_JIT_CACHE_DIR"] = old
            shutil.rmtree(tmp, ignore_errors=True)
    return out


def chiplets_air_probe(pkg, ctx, log_n=20, steps=3):
    """The real ChipletsAir alone at 2^log_n rows (production parameters, aux columns on the device): what a real multi-chiplet
    constraint system costs on the compiled constraint path -- quotient_eval_ms, chunks, VGPRs, logup_aux_ms -- and what loading it
    costs (hiprtc cold = empty cache directory, cached = code objects from disk)."""
    import shutil, tempfile
    from miden_vm_amd import dag, protocol, chiplets_air
    from miden_vm_amd.testing import chiplets_trace
    air, _ = chiplets_air.chiplets_air(num_public=0)
    lookup = dag.lookup_from_constraints(air.blob)
    tmp = tempfile.mkdtemp(prefix="mh_jit_cold_")
    old = os.environ.get("MH_JIT_CACHE_DIR")
    ro = os.environ.get("MH_JIT_CACHE_RO_DIR", "")
    try:
        os.environ["MH_JIT_CACHE_DIR"] = tmp
        os.environ["MH_JIT_CACHE_RO_DIR"] = ""
        t0 = time.perf_counter()
        d0, l0 = pkg.DeviceAir(ctx, air), pkg.DeviceLookup(ctx, lookup)
        cold = time.perf_counter() - t0
        d0.free()
        t0 = time.perf_counter()
        dair, dlk = pkg.DeviceAir(ctx, air), pkg.DeviceLookup(ctx, lookup)
        cached = time.perf_counter() - t0
    finally:
        os.environ["MH_JIT_CACHE_RO_DIR"] = ro
        if old is None:
            os.environ.pop("MH_JIT_CACHE_DIR", None)
        else:
            os.environ["MH_JIT_CACHE_DIR"] = old
        shutil.rmtree(tmp, ignore_errors=True)
    dair.attach_lookup(dlk)
    trace, _ = chiplets_trace.bulk_chiplets(log_n, log_n, seed=2)
    dtr = ctx.upload_trace(trace)
    prm, st = dict(protocol.PROD_PARAMS), protocol.challenger_state()
    pre = protocol.protocol_pre_observe(prm, [])
    proof = pkg.prove(ctx, [dair], [dtr], [], prm, st, pre, None)
    ok, _ = pkg.verify([air], [log_n], [], prm, st, pre, proof.fields, proof.commitments)
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, [dair], [dtr], [], prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_reset()
    pkg.prove(ctx, [dair], [dtr], [], prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    out = {"workload": f"ChipletsAir alone, 2^{log_n} x 22 + 3 EF aux, production parameters, bulk workload (hasher / bitwise / memory / kernel ROM)",
           "constraints": int(air.blob[9]), "dag_nodes": int(air.blob[8]), "ms_per_proof": dt * 1e3, "rows_per_s": (1 << log_n) / dt, "verifies": bool(ok),
           "quotient_eval_ms": prof.get("quotient_eval", {}).get("ms", 0), "logup_aux_ms": prof.get("logup_aux", {}).get("ms", 0),
           "compiled_chunks": dair.compiled_chunks, "chunk_max_vgprs": dair.compiled_max_vgprs,
           "jit_cold_s": cold, "jit_cached_ms": cached * 1e3}
    dtr.free()
    try:  # the hand-over of a trace builder that writes columns: the generator fills page-locked column-major memory
        cols, _owner = pkg.pinned_array(ctx.lib, (22, 1 << log_n))
        chiplets_trace.bulk_chiplets(log_n, log_n, seed=2, out_cols=cols)
        rows, _owner2 = pkg.pinned_array(ctx.lib, (1 << log_n, 22))
        rows[:] = cols.T

        def run(upload, src):
            t = upload(ctx, src)
            pkg.prove(ctx, [dair], [t], [], prm, st, pre, None)
            t.free()

        for name, upload, src in (("h2d_inclusive_colmajor_producer_ms", pkg.Trace.upload_cols_async, cols),
                                  ("h2d_inclusive_rowmajor_ms", pkg.Trace.upload_async, rows)):
            run(upload, src)
            t0 = time.perf_counter()
            for _ in range(steps):
                run(upload, src)
            out[name] = (time.perf_counter() - t0) / steps * 1e3
    except Exception as e:
        out["h2d_error"] = repr(e)[:200]
    dair.free()
    return out


def precompile_session_probe(pkg, ctx, n_perms=80, steps=3):
    """The second client (precompiles-prover/src/session/prove.rs): n_perms Keccak-f[1600] permutations through the real KeccakRoundAir
    (two lanes, 68 columns + 20 EF LogUp columns + 10 periodic), the real BytePairLutAir (2^16 rows, four PREPROCESSED columns committed at
    setup), the group table and the sponge side of the memory bus (miden-vm_amd/precompile_airs.py); production parameters
    (`precompile_pcs_params`), every aux column built on the device, verified through `ChipletMultiAir::eval_external`."""
    import numpy as np
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(3)
    states = [[int(x) for x in rng.integers(0, 1 << 63, 25)] for _ in range(n_perms)]
    t0 = time.perf_counter()
    ledger = PT.BytePairLutRequires()
    trace, mem = PT.keccak_round_trace(states, ledger)
    pairs = [PA.keccak_round_air(), PA.byte_pair_lut_air(), PA.ec_groups_air(), PA.requirer_air()]
    host = [trace, PT.byte_pair_lut_trace(ledger), PT.ec_groups_trace(), PT.requirer_trace(PT.sponge_side_requests(states, mem))]
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [71, 72, 73, 74]
    t0 = time.perf_counter()
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[1].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])   # setup: Preprocessed::build, once per configuration
    dairs[1].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    setup_s = time.perf_counter() - t0
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(),
                       external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_reset()
    pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    for t in traces:
        t.free()
    # the same with the two big main traces BUILT ON THE DEVICE (examples/keccak_trace_device.hip: a client-side GPU trace generator) and
    # handed over with mh_trace_from_device: 200 bytes per permutation cross PCIe; generation inside the timed region
    dev = None
    try:
        import ctypes as C
        kt = C.CDLL(os.path.join(ROOT, "examples", "libkeccak_trace_device.so"))
        st_np = np.array(states, dtype=np.uint64)
        program = np.array([list(x) for x in PA.keccak_round_slots()], dtype=np.int32)
        rcs = np.array(PA.KECCAK_RC, dtype=np.uint64)
        small = [ctx.upload_trace(host[2]), ctx.upload_trace(host[3])]

        def gen_and_prove():
            tr_dev, cnt_dev, mem_dev, lg = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
            t0 = time.perf_counter()
            rc = kt.kt_keccak_round_trace(st_np.ctypes.data_as(C.c_void_p), C.c_int(n_perms), rcs.ctypes.data_as(C.c_void_p),
                                          program.ctypes.data_as(C.c_void_p), C.byref(tr_dev), C.byref(lg), C.byref(cnt_dev), C.byref(mem_dev))
            if rc != 0:
                raise RuntimeError(f"kt_keccak_round_trace: {rc}")
            g = time.perf_counter() - t0
            t_kr = pkg.Trace.from_device(ctx, tr_dev.value, lg.value, PA.KR_MAIN_COLS)
            t_bpl = pkg.Trace.from_device(ctx, cnt_dev.value, 16, 3)
            for p_ in (tr_dev, cnt_dev, mem_dev):
                kt.kt_free(p_)
            pr = pkg.prove(ctx, dairs, [t_kr, t_bpl] + small, root_pub, prm, st, pre, None)
            t_kr.free(); t_bpl.free()
            return g, pr
        g, pr = gen_and_prove()
        same = bool((pr.digest == proof.digest).all())
        t0 = time.perf_counter()
        gs = []
        for _ in range(steps):
            g, pr = gen_and_prove()
            gs.append(g)
        dev = {"trace_generation_ms": sum(gs) / len(gs) * 1e3, "ms_per_proof_with_generation": (time.perf_counter() - t0) / steps * 1e3,
               "same_proof_as_from_host_traces": same,
               "note": "KeccakRound (2^k x 68) and BytePairLut (2^16 x 3) main traces generated in HBM by a client-side kernel, one wave per permutation (hipMalloc and zero-fill of the buffers included)"}
    except Exception as e:
        dev = {"error": repr(e)[:200]}
    return {"workload": f"precompile session: {n_perms} Keccak-f permutations (KeccakRoundAir 68 + 20 EF aux, BytePairLutAir 3 + 2 EF aux + 4 preprocessed, "
                        "EcGroupsAir, sponge side of the memory bus), production parameters, aux columns on the device",
            "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3, "keccak_permutations_per_s": n_perms / dt,
            "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok),
            "compiled_chunks": [a.compiled_chunks for a in dairs], "chunk_max_vgprs": [a.compiled_max_vgprs for a in dairs],
            "kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items() if not k.startswith("span:") and v["ms"] > 0.05},
            "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}, "setup_s": setup_s, "device_built_traces": dev}


def keccak_hash_session_probe(pkg, ctx, steps=3):
    """Keccak-256 of 54 inputs (up to 1.4 KiB each, 40 KiB, 323 Keccak-f permutations: the round chiplet at 2^19 rows) proven over SEVEN
    real chiplets of the second client, in the shape and order the reference's session runs them: ChunkNodeAir (the input tape and one
    transcript-DAG node per distinct input -- `Binding(H_keccak, True, 0, 0)` -- on one row range), Poseidon2Air (the tape's content hash and
    the node hashes), KeccakRoundAir (the permutations), BytePairLutAir (2^16-row PREPROCESSED table), KeccakSpongeAir (pad10*1, absorb,
    squeeze: 67 columns, 24 flattened LogUp columns), EcGroupsAir; outside them only the transcript's readers of the bindings.  Production
    parameters, every aux column on the device."""
    import numpy as np
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(6)
    inputs = [b"", b"abc"] + [bytes(rng.integers(0, 256, int(rng.integers(0, 1401)), dtype=np.uint8)) for _ in range(52)]
    t0 = time.perf_counter()
    ledger, p2 = PT.BytePairLutRequires(), PT.Poseidon2Requires()
    chunks = PT.ChunkRequires(p2)
    sp = PT.SpongeRequires(chunks, ledger)
    nd = PT.KeccakNodeRequires(sp)
    outs = [nd.require(data) for data in inputs]
    kr_trace, mem = PT.keccak_round_trace(sp.perm_inputs, ledger)
    p2_main, _ = PT.poseidon2_chiplet_trace(p2, permute_batch=ctx.poseidon2_permute)
    # `ChipletAir::all()` order (session/prove.rs:111-126): ChunkNode (chunk + Keccak node on one row range), Poseidon2, KeccakRound,
    # BytePairLut, KeccakSponge, [TranscriptEval: its Binding readers], EcGroups
    pairs = [PA.chunk_node_air(), PA.poseidon2_chiplet_air(), PA.keccak_round_air(), PA.byte_pair_lut_air(), PA.keccak_sponge_air(),
             PA.requirer_air(payload=7), PA.ec_groups_air()]
    host = [PT.chunk_node_trace(chunks, nd), p2_main, kr_trace, PT.byte_pair_lut_trace(ledger), PT.keccak_sponge_trace(sp),
            PT.requirer_trace(PT.binding_requests(nd), payload=7), PT.ec_groups_trace()]
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [71, 72, 73, 74]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[3].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])
    dairs[3].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(),
                       external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    n_bytes = sum(len(x) for x in inputs)
    return {"workload": "Keccak-256 hashing session in ChipletAir::all() order: ChunkNodeAir 42 + 14 EF aux, Poseidon2Air, KeccakRoundAir, BytePairLutAir (preprocessed), KeccakSpongeAir 67 + 24 EF aux, the transcript's Binding readers, EcGroupsAir; production parameters, aux columns on the device",
            "inputs": len(inputs), "distinct_inputs": len(nd.records), "input_bytes": n_bytes, "keccak_permutations": len(sp.perm_inputs),
            "poseidon2_permutations": p2.next_seq, "log_trace_heights": proof.log_trace_heights,
            "ms_per_proof": dt * 1e3, "hashes_per_s": len(inputs) / dt, "keccak_permutations_per_s": len(sp.perm_inputs) / dt,
            "input_KiB_per_s": n_bytes / dt / 1024, "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok),
            "keccak256_of_empty": outs[0]["keccak_digest"].hex(), "compiled_chunks": [a.compiled_chunks for a in dairs], "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def chunk_poseidon2_session_probe(pkg, ctx, steps=3):
    """Two chiplets of the second client closing each other's bus: `ChunkAir` and `Poseidon2Air` (precompiles-prover/src/transcript/poseidon2:
    32 columns = state, three witnessed S-boxes, thirteen cube registers; sixteen periodic columns; absorption chains).  1.07 MiB of
    hasher input in 64 invocations = 34 332 Poseidon2 permutations proven in-circuit (2^20 rows), the digests' readers and the Memory64 /
    ChunkChain sides from the stand-in; production parameters, aux columns on the device, verified through `eval_external`.  The trace
    generator steps through the absorption chains with the device permutation (`mh_poseidon2_permute`)."""
    import numpy as np
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(4)
    t0 = time.perf_counter()
    ledger = PT.Poseidon2Requires()
    req = PT.ChunkRequires(ledger)
    inputs = [bytes(rng.integers(0, 256, int(rng.integers(0, 32769)), dtype=np.uint8)) for _ in range(63)]
    inputs.append(inputs[0])
    for data in inputs:
        req.require(data)
        ledger.require_digest(req.last)
    p2_main, outs = PT.poseidon2_chiplet_trace(ledger, permute_batch=ctx.poseidon2_permute)
    others = PT.chunk_side_requests(req, poseidon2_chiplet=True) + PT.poseidon2_out_requests(ledger, outs)
    pairs = [PA.chunk_air(), PA.poseidon2_chiplet_air(), PA.requirer_air(payload=6), PA.ec_groups_air()]
    host = [PT.chunk_trace(req), p2_main, PT.requirer_trace(others, payload=6), PT.ec_groups_trace()]
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [71, 72, 73, 74]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub)
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_reset()
    pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    for t in traces:
        t.free()
    n_bytes = sum(len(x) for x in inputs)
    return {"workload": "chunk + Poseidon2 session: ChunkAir 12 + 5 EF aux, Poseidon2Air 32 + 3 EF aux + 16 periodic, the remaining bus sides (8 + 1 EF aux), EcGroupsAir; production parameters, aux columns on the device",
            "input_bytes": n_bytes, "poseidon2_permutations": ledger.next_seq, "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3,
            "permutations_per_s": ledger.next_seq / dt, "input_MiB_per_s": n_bytes / dt / (1 << 20), "proof_bytes": len(proof.bytes),
            "verifies_with_eval_external": bool(ok), "compiled_chunks": [a.compiled_chunks for a in dairs],
            "kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items() if not k.startswith("span:") and v["ms"] > 0.05},
            "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def uint_add_session_probe(pkg, ctx, steps=3):
    """The second client's modular-addition chiplet (precompiles-prover/src/uint/add: `UintAddAir`, a + b = c mod p over stored 256-bit
    values by a vertical Schwartz-Zippel identity at the LogUp challenge -- a main-trace constraint over the extension field that reads a
    verifier challenge): 2^16 relations (2^17 rows x 30 + 3 EF), the store's and the readers' sides of its two buses from the stand-in,
    the group table; production parameters, aux columns on the device, verified through `eval_external`."""
    import random
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = random.Random(9)
    t0 = time.perf_counter()
    bound = rng.getrandbits(255) | (1 << 254) | 1
    store = PT.UintStore()
    fp = store.pin_modulus(1, bound)
    add = PT.UintAddRequires()
    n_ops = 1 << 16
    vals = [rng.randrange(1, bound + 1) for _ in range(n_ops + 1)]
    ptrs = [store.intern(v, fp) for v in vals]
    for i in range(n_ops):
        add.record(ptrs[i], ptrs[i + 1], store.intern((vals[i] + vals[i + 1]) % (bound + 1), fp), fp, 1)
    main = PT.uint_add_trace(add, store)
    others = store.uint_val_requests() + PT.uint_add_consumer_requests(add)
    pairs = [PA.uint_add_air(), PA.requirer_air(payload=10), PA.ec_groups_air()]
    host = [main, PT.requirer_trace(others, payload=10), PT.ec_groups_trace()]
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [71, 72, 73, 74]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub)
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    return {"workload": "uint-add session: UintAddAir 30 + 3 EF aux (one periodic selector), the store's and the readers' bus sides (12 + 1 EF aux), EcGroupsAir; production parameters, aux columns on the device",
            "relations": n_ops, "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3, "modular_additions_per_s": n_ops / dt,
            "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok), "compiled_chunks": [a.compiled_chunks for a in dairs],
            "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def precompile_full_session_probe(pkg, ctx, steps=3):
    """The second client's WHOLE session: all twelve AIRs of `ChipletAir::all()` in the reference's order (precompiles-prover/src/session/
    prove.rs:111-126) -- [ChunkNode, Poseidon2, KeccakRound, BytePairLut, KeccakSponge, TranscriptEval, UintStoreMul, UintAdd, EcGroups,
    EcPointStore, EcGroupAdd, EcMsm] -- over the fixed environment, no stand-in, the transcript root as the public input: 24 Keccak-256
    claims, a 256-bit arithmetic claim, a pin claim, an EC addition claim and an MSM claim folded into one root; production parameters,
    every aux column on the device, verified through the full `eval_external`."""
    import numpy as np
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(12)
    t0 = time.perf_counter()
    inputs = [b"", b"abc"] + [bytes(rng.integers(0, 256, int(rng.integers(0, 1201)), dtype=np.uint8)) for _ in range(22)]
    pairs, host, info = PT.precompile_session(inputs, permute_batch=ctx.poseidon2_permute)
    gen_s = time.perf_counter() - t0
    airs_h, root_pub = [p_[0] for p_ in pairs], info["public_root"]
    prm = dict(protocol.PROD_PARAMS)
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[3].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])
    dairs[3].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    ext = PA.external_assertions(pkg, fixed_uints=True)
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(), external=ext)
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_reset()
    pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    for t in traces:
        t.free()
    led = info["ledgers"]
    return {"kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items() if not k.startswith("span:") and v["ms"] > 0.05},
            "workload": "the whole deferred-precompile session: ChipletAir::all() = ChunkNodeAir, Poseidon2Air, KeccakRoundAir, BytePairLutAir (preprocessed), KeccakSpongeAir, TranscriptEvalAir, UintStoreMulAir, UintAddAir, EcGroupsAir, EcPointStoreAir, EcGroupAddAir, EcMsmAir; the fixed environment; the transcript root as the public input; production parameters, aux columns on the device",
            "keccak_claims": len(inputs), "input_bytes": sum(len(x) for x in inputs), "transcript_nodes": len(led["eval"].nodes),
            "poseidon2_permutations": led["p2"].next_seq, "keccak_permutations": len(led["node"].sponge.perm_inputs), "point_additions": len(led["ec_add"].ops),
            "modular_macs": len(led["muls"].ops), "modular_additions": len(led["adds"].ops), "public_root": [int(x) for x in root_pub],
            "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3, "proof_bytes": len(proof.bytes),
            "verifies_with_eval_external": bool(ok), "keccak256_of_empty": bytes(info["keccak_digests"][0]).hex(),
            "compiled_chunks": [a.compiled_chunks for a in dairs], "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def ec_msm_session_probe(pkg, ctx, steps=3):
    """The second client's MSM chiplet (precompiles-prover/src/ec/msm: `EcMsmAir`, symbolic multi-scalar-multiplication expressions built
    by intro / neg / combine steps the AIR checks one by one: variable-length blocks, merge walks over sorted term lists, a strict pointer
    ordering) on top of the arithmetic + EC stack, SEVEN real chiplets over the fixed environment: sum of eight terms k_i P_i with 256-bit
    scalars by Straus' interleaved double-and-add over expressions (~1 280 proven merge steps, each with a proven point addition and its
    proven field arithmetic); production parameters, aux columns on the device, verified through the full `eval_external`."""
    import random
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = random.Random(8)
    t0 = time.perf_counter()
    terms = [(rng.getrandbits(256) % PA.K1_BOUND, m) for m in (1, 2, 3, 5, 7, 11, 13, 17)]
    pairs, host, (val, expr, (store, adds, muls, ec, ec_add, msm)) = PT.ec_msm_session(terms)
    gen_s = time.perf_counter() - t0
    x_ptr, _ = ec.point_params(val)[1]
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [111, 112, 113, 114]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[0].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])
    dairs[0].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    ext = PA.external_assertions(pkg, fixed_uints=True)
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(), external=ext)
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    return {"workload": "MSM session in SessionTraces::mains order: BytePairLutAir (preprocessed), UintStoreMulAir 44 + 29 EF aux, UintAddAir 30 + 3, EcGroupsAir, EcPointStoreAir 14 + 5, EcGroupAddAir 21 + 12, EcMsmAir 38 + 11 EF aux, the resolve's readers; the fixed environment; production parameters, aux columns on the device",
            "msm_terms": len(terms), "scalar_bits": 256, "expressions": len(msm.exprs), "term_rows": sum(len(e["rows"]) for e in msm.exprs),
            "point_additions": len(ec_add.ops), "modular_additions": len(adds.ops), "modular_macs": len(muls.ops), "stored_uints": len(store.rows),
            "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3, "msm_per_s": 1.0 / dt, "proof_bytes": len(proof.bytes),
            "verifies_with_eval_external": bool(ok), "value_x": hex(store.value(x_ptr)), "compiled_chunks": [a.compiled_chunks for a in dairs],
            "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def uint_arith_session_probe(pkg, ctx, steps=3):
    """The second client's 256-bit arithmetic with every chiplet real (precompiles-prover/src/uint: `UintStoreMulAir` -- the range-checked
    store and kappa_a a b +- kappa_c c = r (mod p) by vertical Schwartz-Zippel identities carried in three aux REGISTER columns -- and
    `UintAddAir`): a Horner evaluation over the secp256k1 base field, 2^14 proven multiply-accumulates + 2^14 proven modular additions over
    49 159 stored values (2^18 rows x 44 + 29 EF, 2^15 x 30 + 3), the 2^16-row preprocessed table, the fixed environment; production parameters, aux columns
    (26 LogUp + 3 registers) on the device, verified through the full `eval_external`."""
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    t0 = time.perf_counter()
    n_steps = 1 << 14
    pairs, host, (final, (store, adds, muls)) = PT.uint_arith_session(n_steps)
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [101, 102, 103, 104]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[0].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])
    dairs[0].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(),
                       external=PA.external_assertions(pkg, fixed_uints=True))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    return {"workload": "uint arithmetic session: BytePairLutAir (preprocessed), UintStoreMulAir 44 + 29 EF aux (26 LogUp columns, 3 registers), UintAddAir 30 + 3, EcGroupsAir, the relations' readers; the fixed environment; production parameters, aux columns on the device",
            "modular_macs": len(muls.ops), "modular_additions": len(adds.ops), "stored_uints": len(store.rows), "log_trace_heights": proof.log_trace_heights,
            "ms_per_proof": dt * 1e3, "modular_macs_per_s": len(muls.ops) / dt, "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok),
            "horner_value": hex(final), "compiled_chunks": [a.compiled_chunks for a in dairs], "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def ec_add_session_probe(pkg, ctx, steps=3):
    """The second client's group-law chiplet (precompiles-prover/src/ec/add: `EcGroupAddAir`, 21 columns, twelve flattened LogUp columns on
    seven buses, four-row blocks; every piece of field arithmetic a pointer-level certificate consumed from the uint chiplets) inside the
    reference's "arithmetic + EC stack" in its order: 16 scalar multiples k G over secp256k1 by double-and-add with 256-bit scalars =
    ~6 000 proven point additions (doubles, chords, pass-throughs; results minted with closure certificates) over SIX real chiplets --
    BytePairLutAir (preprocessed), UintStoreMulAir (the uint store and the multiply-accumulate relation: 44 columns, 26 LogUp columns and
    three extension-field registers built by a scan over affine maps), UintAddAir, EcGroupsAir, EcPointStoreAir, EcGroupAddAir -- every
    bus between them closed by themselves, over the session's fixed environment (the full `fixed_boundary_correction`); production parameters, aux columns on the device, verified through `eval_external`."""
    import random
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = random.Random(5)
    t0 = time.perf_counter()
    scalars = [rng.getrandbits(256) % PA.K1_BOUND for _ in range(16)]
    pairs, host, (results, (store, adds, muls, ec, ec_add)) = PT.ec_add_session(scalars)
    gen_s = time.perf_counter() - t0
    x_ptr, y_ptr = ec.point_params(results[0])[1]
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [91, 92, 93, 94]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    raw = ctx.upload_trace(airs_h[0].preprocessed)
    com = pkg.commit_traces(ctx, [raw], prm["log_blowup"])
    dairs[0].attach_preprocessed(com.tree(), 0, raw=raw)
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub, preprocessed_root=com.root())
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, preprocessed_root=com.root(),
                       external=PA.external_assertions(pkg, fixed_uints=True))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    n_adds = len(ec_add.ops)
    return {"workload": "EC addition session in SessionTraces::mains order: BytePairLutAir (preprocessed), UintStoreMulAir 44 + 29 EF aux (26 LogUp columns, 3 registers), UintAddAir 30 + 3, EcGroupsAir, EcPointStoreAir 14 + 5, EcGroupAddAir 21 + 12 EF aux, the additions' readers; production parameters, aux columns on the device",
            "stored_uints": len(store.rows),
            "scalar_multiplications": len(scalars), "point_additions": n_adds, "modular_additions": len(adds.ops), "modular_macs": len(muls.ops),
            "stored_points": len(ec.points), "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3,
            "point_additions_per_s": n_adds / dt, "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok),
            "first_multiple_x": hex(store.value(x_ptr)), "compiled_chunks": [a.compiled_chunks for a in dairs], "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def ec_store_session_probe(pkg, ctx, steps=3):
    """The second client's point store (precompiles-prover/src/ec: `EcPointStoreAir`, 14 columns, five flattened LogUp columns -- the
    EcPoint provide, the EcGroup and closure-certificate consumes, the curve-membership trio u = x^2 + a, w = x u + b, y^2 = w as three
    degree-3 UintMul consumes) next to the group table it reads: 2^15 - 1 points of secp256k1 bound by value (98 301 membership relations),
    the foreign sides of the UintMul / EcPoint buses from the stand-in; production parameters, aux columns on the device."""
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    t0 = time.perf_counter()
    n_points = (1 << 15) - 1
    pairs, host, _ = PT.ec_store_session(n_points)
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [81, 82, 83, 84]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub)
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    return {"workload": "ec-store session: EcPointStoreAir 14 + 5 EF aux, EcGroupsAir 6 + 1, the foreign bus sides (12 + 1 EF aux); production parameters, aux columns on the device",
            "points": n_points + 1, "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3, "bound_points_per_s": n_points / dt,
            "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok), "compiled_chunks": [a.compiled_chunks for a in dairs],
            "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def chunk_session_probe(pkg, ctx, steps=3):
    """The second client's chunk chiplet (precompiles-prover/src/hash/chunk: `ChunkAir`, twelve columns, five flattened LogUp columns on
    the Memory64 / Poseidon2In / ChunkChain buses): 1.07 MiB of hasher input in 64 invocations (35 076 chunks, 2^16 rows), the other sides
    of its buses from the one-interaction-per-row stand-in (2^18 rows), the group table; production parameters, aux columns on the device,
    verified through `ChipletMultiAir::eval_external`."""
    import numpy as np
    from miden_vm_amd import protocol, precompile_airs as PA
    from miden_vm_amd.testing import precompile_trace as PT
    rng = np.random.default_rng(4)
    t0 = time.perf_counter()
    req = PT.ChunkRequires()
    inputs = [bytes(rng.integers(0, 256, int(rng.integers(0, 32769)), dtype=np.uint8)) for _ in range(63)]
    inputs.append(inputs[0])
    for data in inputs:
        req.require(data)
    pairs = [PA.chunk_air(), PA.requirer_air(payload=6), PA.ec_groups_air()]
    host = [PT.chunk_trace(req), PT.requirer_trace(PT.chunk_side_requests(req), payload=6), PT.ec_groups_trace()]
    gen_s = time.perf_counter() - t0
    airs_h = [p_[0] for p_ in pairs]
    prm = dict(protocol.PROD_PARAMS)
    root_pub = [71, 72, 73, 74]
    dairs = [pkg.DeviceAir(ctx, a) for a in airs_h]
    for d, (_, lk) in zip(dairs, pairs):
        d.attach_lookup(pkg.DeviceLookup(ctx, lk))
    st = protocol.challenger_state(PA.PLACEHOLDER_RELATION_DIGEST)
    pre = protocol.protocol_pre_observe(prm, root_pub)
    traces = [ctx.upload_trace(t) for t in host]
    proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    ok, _ = pkg.verify(airs_h, proof.log_trace_heights, root_pub, prm, st, pre, proof.fields, proof.commitments, external=PA.external_assertions(pkg))
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, dairs, traces, root_pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    for t in traces:
        t.free()
    n_bytes = sum(len(x) for x in inputs)
    return {"workload": "chunk session: ChunkAir 12 + 5 EF aux, the other sides of its three buses (8 + 1 EF aux), EcGroupsAir; production parameters, aux columns on the device",
            "input_bytes": n_bytes, "chunks": req.next_chunk_seq, "log_trace_heights": proof.log_trace_heights, "ms_per_proof": dt * 1e3,
            "input_MiB_per_s": n_bytes / dt / (1 << 20), "proof_bytes": len(proof.bytes), "verifies_with_eval_external": bool(ok),
            "compiled_chunks": [a.compiled_chunks for a in dairs], "test_trace_generator_s": {"seconds": gen_s, "note": GEN_NOTE}}


def miden_real_probe(pkg, ctx, iters=9250, steps=3, lmcs="poseidon2", inputs=None):
    """THE Miden statement, no stand-ins: CoreAir + ChipletsAir + Poseidon2PermutationAir (miden-vm_amd/{core,chiplets,miden}_air.py) over
    the traces of ONE executed program -- a loop over a hash / u32 / memory mix run by the small VM of miden-vm_amd/core_trace.py --
    with the reference's statement framing (RELATION_DIGEST, observe_protocol_params, `MidenMultiAir::observe`), production parameters,
    all eight LogUp aux columns built on the device, verified with `MidenMultiAir::eval_external` (boundary corrections).  This is the
    neighbour of the reference's published prover figure (README.md:148-153: ~100-150 k rows/s on 16-64 CPU threads)."""
    import json as _json
    from miden_vm_amd import dag, protocol, miden_air, chiplets_air, core_air, miden_statement
    from miden_vm_amd.testing import core_trace
    gen_s = None
    if isinstance(inputs, tuple):      # (inputs, seconds the test generator took)
        inputs, gen_s = inputs
    if inputs is None:
        t0 = time.perf_counter()
        inputs = core_trace.prove_inputs(core_trace.CoreVM(stack_inputs=list(range(16))), core_trace.bench_program(iters))
        gen_s = time.perf_counter() - t0
    r = inputs
    if lmcs != "poseidon2":
        ctx.set_lmcs(lmcs)
    host_airs = [core_air.core_air()[0], chiplets_air.chiplets_air()[0], miden_air.poseidon2_permutation_air(num_public=32)[0]]
    host = [r["core"], r["chiplets"], r["poseidon2"]]
    lhs = [int(t.shape[0]).bit_length() - 1 for t in host]
    t0 = time.perf_counter()
    airs = [pkg.DeviceAir(ctx, a) for a in host_airs]
    for d, a in zip(airs, host_airs):
        d.attach_lookup(pkg.DeviceLookup(ctx, dag.lookup_from_constraints(a.blob)))
    air_load_s = time.perf_counter() - t0
    traces = [ctx.upload_trace(t) for t in host]
    prm = dict(protocol.PROD_PARAMS)
    kat = _json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))
    st = protocol.challenger_state(kat["relation_digest"])
    pub, aux_inputs = r["public_values"], r["aux_inputs"]
    pre = miden_statement.statement_pre_observe(prm, pub, aux_inputs)
    proof = pkg.prove(ctx, airs, traces, pub, prm, st, pre, None)
    ok, _ = pkg.verify(host_airs, lhs, pub, prm, st, pre, proof.fields, proof.commitments,
                       external=miden_statement.external_assertions(pkg, pub, aux_inputs), lmcs=lmcs)
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, airs, traces, pub, prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_reset()
    pkg.prove(ctx, airs, traces, pub, prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    for t in traces:
        t.free()
    # the same proof with the three host matrices (row-major, page-locked: what `prove_stark` receives) uploaded inside
    # the timed region -- mh_prove_host starts the uploads in proof order, matrix k + 1 lands under matrix k's LDE and leaf hashing
    h2d_ms, up_bytes = None, sum(int(t.nbytes) for t in host)
    try:
        pins = []
        for t in host:
            pin, owner = pkg.pinned_array(ctx.lib, t.shape)
            pin[:] = t
            pins.append((pin, owner))
        pkg.prove_host(ctx, airs, [p_[0] for p_ in pins], pub, prm, st, pre, None)
        t0 = time.perf_counter()
        for _ in range(steps):
            pkg.prove_host(ctx, airs, [p_[0] for p_ in pins], pub, prm, st, pre, None)
        h2d_ms = (time.perf_counter() - t0) / steps * 1e3
        del pins
    except Exception as e:
        h2d_ms = repr(e)[:200]
    rows = 1 << max(lhs)
    return {"workload": f"the real Miden statement (CoreAir 51 + 4 EF, ChipletsAir 22 + 3 EF, Poseidon2PermutationAir 16 + 1 EF) of a loop of {iters} "
                        "iterations (u32 / bitwise / memory / HPERM mix), production parameters",
            "lmcs": lmcs, "log_trace_heights": lhs, "ms_per_proof": dt * 1e3, "rows_per_s": rows / dt, "proof_bytes": len(proof.bytes),
            "verifies_with_eval_external": bool(ok), "h2d_inclusive_ms": h2d_ms, "upload_bytes": up_bytes,
            "constraints": [int(a.blob[9]) for a in host_airs],
            "compiled_chunks": [a.compiled_chunks for a in airs], "chunk_max_vgprs": [a.compiled_max_vgprs for a in airs],
            "kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items() if not k.startswith("span:") and v["ms"] > 0.05},
            "air_load_s": air_load_s,
            **({"test_trace_generator_s": {"seconds": gen_s, "note": "Python TEST generator (miden-vm_amd/testing/core_trace.py), not product: the reference's "
                                                                     "processor builds these matrices; excluded from every rate"}} if gen_s is not None else {}),
            # speed-ups are quoted from the H2D-inclusive time only (the metric includes the upload) and only against the
            # reference's one published figure, which is another machine, another program and the Blake3 configuration
            "vs_published_cpu_reference": {"reference_rows_per_s": 152000, "note": "README.md:151 of the reference: blake3 example, 64-thread EPYC 9R45, other "
                                           "hardware and another program: an order-of-magnitude anchor, not a like-for-like baseline; ratio = "
                                           "rows / h2d_inclusive time / 152 k",
                                           "ratio_h2d_inclusive": (rows / (h2d_ms / 1e3) / 152000) if isinstance(h2d_ms, float) else None}}


def miden_real_sharded_probe(pkg, ctx, comm, sharding, barrier, max_over_ranks, rank, iters=9250, steps=2):
    """The real three-AIR Miden statement (as `miden_real`) proved ONCE PER STEP by all ranks together: `mh_prove_sharded` over
    CoreAir (compiled chunks, 4 EF aux) + ChipletsAir + Poseidon2PermutationAir, heights 2^20 / 2^20 / 2^18, device LogUp on every
    rank, `MidenMultiAir` framing; rank 0 verifies through eval_external.  Every rank builds the same traces (the test generator
    is deterministic) and uploads them before the clock starts."""
    import json as _json
    from miden_vm_amd import dag, protocol, miden_air, chiplets_air, core_air, miden_statement
    from miden_vm_amd.testing import core_trace
    r = core_trace.prove_inputs(core_trace.CoreVM(stack_inputs=list(range(16))), core_trace.bench_program(iters))
    host_airs = [core_air.core_air()[0], chiplets_air.chiplets_air()[0], miden_air.poseidon2_permutation_air(num_public=32)[0]]
    host = [r["core"], r["chiplets"], r["poseidon2"]]
    lhs = [int(t.shape[0]).bit_length() - 1 for t in host]
    airs = [pkg.DeviceAir(ctx, a) for a in host_airs]
    for d, a in zip(airs, host_airs):
        d.attach_lookup(pkg.DeviceLookup(ctx, dag.lookup_from_constraints(a.blob)))
    traces = [ctx.upload_trace(t) for t in host]
    prm = dict(protocol.PROD_PARAMS)
    kat = _json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))
    st = protocol.challenger_state(kat["relation_digest"])
    pub, aux_inputs = r["public_values"], r["aux_inputs"]
    pre = miden_statement.statement_pre_observe(prm, pub, aux_inputs)
    proof = sharding.prove_sharded(pkg, ctx, comm, airs, traces, pub, prm, st, pre, None)
    ok = None
    if rank == 0:
        ok, _ = pkg.verify(host_airs, lhs, pub, prm, st, pre, proof.fields, proof.commitments, external=miden_statement.external_assertions(pkg, pub, aux_inputs))
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = sharding.prove_sharded(pkg, ctx, comm, airs, traces, pub, prm, st, pre, None)
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0) / steps
    ctx.prof_enable(True)
    ctx.prof_filter(None)
    ctx.prof_reset()
    sharding.prove_sharded(pkg, ctx, comm, airs, traces, pub, prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    for t in traces:
        t.free()
    rows = 1 << max(lhs)
    return {"workload": f"the real Miden statement (CoreAir + ChipletsAir + Poseidon2PermutationAir of a loop of {iters} iterations), ONE proof "
                        "sharded by cosets over the ranks, production parameters, traces resident on every rank",
            "log_trace_heights": lhs, "ms_per_proof": dt * 1e3, "rows_per_s": rows / dt, "proof_bytes": len(proof.bytes),
            "verifies_with_eval_external": bool(ok) if ok is not None else None, "digest": [hex(int(x)) for x in proof.digest],
            "sharded_breakdown": {"comm_ms": {k: round(v["ms"], 3) for k, v in prof.items() if k.startswith("comm_")},
                                  "kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items() if not k.startswith(("span:", "comm_")) and v["ms"] > 0.05}}}


def hash_config_probe(pkg, device, log_n, lmcs, steps=5):
    """A complete proof (mh_prove: transcript, PoW search and openings included) of the bench instance under another of the
    reference's five StarkConfigs (air/src/config.rs:212-353; HashFunction::Blake3_256 is ProvingOptions::default())."""
    ctx = pkg.Ctx(device)
    try:
        ctx.set_lmcs(lmcs)
        r = ProveRunner(pkg, ctx, log_n, 21)
        r.step()
        t0 = time.perf_counter()
        for _ in range(steps):
            r.step()
        dt = (time.perf_counter() - t0) / steps
        nbytes = len(r.proof.bytes)
        r.trace.free()
        r.dair.free()
    finally:
        ctx.close()
    return {"ms_per_proof": dt * 1e3, "rows_per_s": (1 << log_n) / dt, "proof_bytes": nbytes}


def dump_outputs(proof, out_dir):
    """What a caller of the timed path receives from one step -- the Proof of `prove` -- as DIR/<name>.npy in float64.  A Goldilocks
    element (u64) does not fit a float64 mantissa, so every u64 becomes its two 32-bit halves on a last axis of 2: [low, high] (exact).
    fields (F, 2), commitments (C, 4, 2), digest (4, 2), proof_bytes (B,) the serialised StarkProofData, log_trace_heights (T,).
    A proof is a few hundred kB at most (logarithmic in the trace), far below the 64 MB bound."""
    import numpy as np

    def halves(a):
        a = np.asarray(a, dtype=np.uint64)
        return np.stack([a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)], axis=-1).astype(np.float64)

    os.makedirs(out_dir, exist_ok=True)
    arrays = {"fields": halves(proof.fields), "commitments": halves(proof.commitments), "digest": halves(proof.digest),
              "proof_bytes": np.frombuffer(proof.bytes, dtype=np.uint8).astype(np.float64),
              "log_trace_heights": np.asarray(proof.log_trace_heights, dtype=np.float64)}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_baseline(runner, cpu_log_n):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_binding as ob
    t = synth_trace(np.random.default_rng(1), cpu_log_n, 51)
    ob.use_fast_library(True)  # ORACLE_FAST build: same results, no 128-bit division per multiplication
    ob.lib()
    t0 = time.perf_counter()
    ob.prove([runner.air], [t], [], runner.params)
    dt = time.perf_counter() - t0
    cores = ob.omp_threads()
    return {"value": (1 << cpu_log_n) / dt, "unit": "trace rows/s", "cores": cores, "kind": "port",
            "sample": f"CPU restatement (oracle/, OpenMP {cores} threads) proving miden:{cpu_log_n}:51:8 with the same parameters in {dt:.2f} s",
            "cpu_model": cpu_model(),
            "note": "a plain C++ restatement, not the reference's Rayon/AVX prover (unbuildable here: no Rust).  The reference's only "
                    "published figure (README.md:151, 64-thread EPYC 9R45, ~152 k rows/s) is for a different instance: the blake3 "
                    "example with all three Miden AIRs (89 main + 16 aux columns, real constraints), whose neighbour here is the "
                    "`miden_shape` key, not this DummyMidenAir workload"}


def miden_shape_probe(pkg, ctx, steps=3):
    """The full Miden VM statement shape at 2^20 rows for every AIR (SURVEY.md section 8 sizes): main widths 51/22/16, aux 4/3/1
    EF, one LogUp final per AIR.  Core is a degree-9 stand-in (the core AIR is not ported yet); the SECOND instance is the real
    ChipletsAir (miden-vm_amd/chiplets_air.py: 113 + 7 constraints of degree <= 9, 2 periodic columns, three LogUp columns) on a
    bulk workload (chiplets_trace.bulk_chiplets), the THIRD the real Poseidon2PermutationAir (miden-vm_amd/miden_air.py: 61
    constraints of degree 8, 16 periodic columns) holding exactly the permutations the chiplets trace requests; both AIRs' aux
    columns are built on the device from the lookup programs derived from their constraint DAGs.  Timed twice: traces resident,
    and with the three host matrices uploaded inside the timed region (mh_trace_upload_async in proof order: matrices 2 and 3
    land under the LDE + leaf sponges of matrix 1)."""
    import numpy as np
    from miden_vm_amd import dag, protocol, miden_air, chiplets_air
    from miden_vm_amd.testing import chiplets_trace
    p2, _ = miden_air.poseidon2_permutation_air()
    ch, _ = chiplets_air.chiplets_air(num_public=0)
    host_airs = [dag.dummy_miden_air(51, 4, num_aux_values=1), ch, p2]
    t0 = time.perf_counter()
    airs = [pkg.DeviceAir(ctx, a) for a in host_airs]
    for i in (1, 2):
        airs[i].attach_lookup(pkg.DeviceLookup(ctx, dag.lookup_from_constraints(host_airs[i].blob)))
    air_load_s = time.perf_counter() - t0
    tr_ch, tr_p2 = chiplets_trace.bulk_chiplets(20, 20, seed=5)
    host = [synth_trace(np.random.default_rng(11), 20, 51), tr_ch, tr_p2]
    traces = [ctx.upload_trace(t) for t in host]
    prm, st = dict(protocol.PROD_PARAMS), protocol.challenger_state()
    pre = protocol.protocol_pre_observe(prm, [])
    proof = pkg.prove(ctx, airs, traces, [], prm, st, pre, None)
    ok, _ = pkg.verify(host_airs, [20, 20, 20], [], prm, st, pre, proof.fields, proof.commitments)
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = pkg.prove(ctx, airs, traces, [], prm, st, pre, None)
    dt = (time.perf_counter() - t0) / steps
    ctx.prof_enable(True)  # the two kernel classes reported below: one more proof, outside the timing (event records cost ~0.7 ms per proof here)
    ctx.prof_reset()
    proof = pkg.prove(ctx, airs, traces, [], prm, st, pre, None)
    prof = ctx.prof()
    ctx.prof_enable(False)
    prof = {k: dict(v, ms=v["ms"] * steps) for k, v in prof.items()}  # the expressions below divide by `steps`
    for t in traces:
        t.free()
    out = {"workload": "three AIRs at 2^20 rows: main 51/22/16, aux 4/3/1 EF (89 + 16 base columns), production parameters; second AIR = the real "
                       "ChipletsAir, third = the real Poseidon2PermutationAir (aux columns from the lookup programs derived from their "
                       "constraint DAGs, on the device); core = a degree-9 stand-in",
           "ms_per_proof": dt * 1e3, "rows_per_s": (1 << 20) / dt, "proof_bytes": len(proof.bytes), "verifies": bool(ok),
           "quotient_eval_ms": prof.get("quotient_eval", {}).get("ms", 0) / steps, "logup_aux_ms": prof.get("logup_aux", {}).get("ms", 0) / steps,
           "p2_air_compiled_chunks": airs[2].compiled_chunks, "p2_air_chunk_max_vgprs": airs[2].compiled_max_vgprs,
           "chiplets_air_compiled_chunks": airs[1].compiled_chunks, "chiplets_air_chunk_max_vgprs": airs[1].compiled_max_vgprs,
           "air_load_s": air_load_s}
    try:
        pins = []
        for t in host:
            a, owner = pkg.pinned_array(ctx.lib, t.shape)
            a[:] = t
            pins.append((a, owner))

        def with_upload(asynchronous):
            up = [pkg.Trace.upload_async(ctx, a) if asynchronous else ctx.upload_trace(a) for a, _ in pins]
            pkg.prove(ctx, airs, up, [], prm, st, pre, None)
            for t in up:
                t.free()

        for mode in (True, False):
            with_upload(mode)
            t0 = time.perf_counter()
            for _ in range(steps):
                with_upload(mode)
            d = (time.perf_counter() - t0) / steps
            out["h2d_inclusive_ms" if mode else "h2d_inclusive_serial_ms"] = d * 1e3
        out["upload_bytes"] = int(sum(t.nbytes for t in host))
        del pins
    except Exception as e:  # pragma: no cover
        out["h2d_error"] = repr(e)[:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=20, help="rows of the single-GPU instance (N = 1)")
    ap.add_argument("--shard-log-n", type=int, default=int(os.environ.get("MIDEN_BENCH_SHARD_LOG_N", "24")),
                    help="rows of the ONE proof sharded over the GPUs (N > 1)")
    ap.add_argument("--comm", default=os.environ.get("MIDEN_BENCH_COMM", "rccl"), choices=["rccl", "torch"])
    ap.add_argument("--full", action="store_true",
                    help="also the per-kernel breakdown, the rooflines, the H2D-inclusive figure, the real statement, the precompile session "
                         "and the CPU baseline (the options below refine what --full measures); without it only the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the proof of the last one as DIR/<name>.npy (float64; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="headline, roofline and CPU baseline only (no h2d_inclusive / real-statement probes)")
    ap.add_argument("--extras", action="store_true",
                    help="also the twenty side probes (miden_shape, jit_load, chiplets_air, the second client's per-chiplet sessions, in-flight "
                         "proofs, the other hash configurations); the --full line carries the headline, the H2D-inclusive figure, the real "
                         "statement under Poseidon2 and Blake3 and the whole precompile session")
    ap.add_argument("--cpu-log-n", type=int, default=18)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist
    from __graft_entry__ import load_package
    pkg = load_package()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # Control plane (rendezvous, barriers, the max over ranks, handing the RCCL id around): torch.distributed over gloo.  The
    # DATA path of a sharded proof is RCCL inside libmidenhip (or, with --comm torch, torch.distributed callbacks).
    # MIDEN_BENCH_BACKEND=nccl makes torch use its own RCCL for the control plane as well.
    backend = os.environ.get("MIDEN_BENCH_BACKEND", "gloo")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def all_ok(flag):
        if world == 1:
            return bool(flag)
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    ctx = pkg.Ctx(dev_index)
    mode, comm, comm_name, fallback = "single", None, None, None
    comm_log = []  # one entry per communicator tried: its bring-up steps with their wall times -- a failure on the 8-GPU box is read from the line
    if world > 1:
        import threading
        from miden_vm_amd import sharding
        own_gpu = torch.cuda.device_count() >= world  # one GPU per rank (the driver's node) or ranks sharing a device (test box)
        choices = [args.comm] + (["torch"] if args.comm == "rccl" else [])
        if "torch" in choices and own_gpu and backend != "nccl":
            choices.insert(choices.index("torch"), "torch-nccl")  # torch's own RCCL before the host-staged gloo path
        for choice in choices:
            box = {}

            def attempt():
                steps_ = box.setdefault("steps", [])
                t_ = time.perf_counter()

                def mark(name):
                    nonlocal t_
                    now = time.perf_counter()
                    steps_.append([name, round(now - t_, 3)])
                    t_ = now
                try:
                    torch.cuda.set_device(dev_index)  # the current device is per thread
                    box["at"] = "create (unique id broadcast + communicator init)"
                    if choice == "rccl":
                        c_ = sharding.RcclComm(ctx, rank, world)
                    elif choice == "torch-nccl":
                        c_ = sharding.TorchComm(rank, world, group=box["group"])
                    else:
                        c_ = sharding.TorchComm(rank, world)
                    box["comm"] = c_
                    mark("create")
                    box["at"] = "selftest (all_to_all / all_gather / gather_to / broadcast on small buffers)"
                    sharding.comm_selftest(ctx, c_)
                    mark("selftest")
                    box["at"] = "trial proof (2^12 rows, sharded)"
                    trial = ShardedRunner(pkg, ctx, 12, c_)  # a small sharded proof before the big trace is built
                    trial.step()
                    box["ok"] = trial.proof is not None
                    trial.trace.free()
                    mark("trial_proof_2p12")
                    box["at"] = "done"
                except Exception as e:
                    box["err"] = f"{box.get('at', '?')}: {repr(e)[:160]}"

            try:
                if choice == "torch-nccl":
                    box["group"] = dist.new_group(backend="nccl")  # collective call: made by every rank, outside the watchdog
                # watchdog: a communicator that hangs while coming up (not one that fails) must not hang the bench -- the attempt
                # runs on its own thread, the ranks agree on the outcome over the control plane, a stuck thread is abandoned
                th = threading.Thread(target=attempt, daemon=True)
                th.start()
                th.join(timeout=float(os.environ.get("MIDEN_BENCH_COMM_TIMEOUT", "240")))
                if th.is_alive():
                    box["err"] = f"timed out after {os.environ.get('MIDEN_BENCH_COMM_TIMEOUT', '240')} s in: {box.get('at', 'thread start')}"
            except Exception as e:
                box["err"] = repr(e)[:160]
            ok = bool(box.get("ok")) and "err" not in box
            comm_log.append({"choice": choice, "ok_on_rank0": ok, "steps_s": list(box.get("steps", [])), **({"error": box["err"]} if "err" in box else {})})
            if not ok:
                fallback = (fallback or "") + f"{choice}: {box.get('err', 'no proof')}; "
            if all_ok(ok):
                mode, comm_name, comm = "sharded", choice, box["comm"]
                break
        if mode != "sharded":
            mode = "replicas"

    if mode == "sharded":
        runner = ShardedRunner(pkg, ctx, args.shard_log_n, comm)
        log_n, rows_per_step, scaling = args.shard_log_n, 1 << args.shard_log_n, "strong"
    else:
        runner = ProveRunner(pkg, ctx, args.log_n, 1 + rank)
        log_n, rows_per_step = args.log_n, (1 << args.log_n) * world
        # N = 1 is the first point of the strong-scaling series the N > 1 lines continue (one proof sharded over the GPUs; a single
        # MI355X proves 2^24 rows at the same rows/s as 2^20); independent replicas after a fallback are weak scaling
        scaling = "strong" if world == 1 else "weak"

    for _ in range(args.warmup):
        runner.step()
    # Timed region.  With --full: HIP events around the DOMINANT kernel class only (for the rooflines).  An event record is a
    # barrier packet on the stream; with every class and span recorded (~130 scopes per proof) a 2^20-row proof is 0.5 ms slower
    # (47.7 vs 47.2 ms).  The full per-class breakdown (`kernels`, `spans`, `sharded_breakdown`) comes from a second, untimed pass
    # right after.  A plain run records nothing.
    DOMINANT = "lmcs_leaf_absorb"
    if args.full:
        ctx.prof_filter(DOMINANT)
        ctx.prof_enable(True)
        ctx.prof_reset()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(runner.proof, args.dump_outputs)

    if mode == "sharded":
        how = {"rccl": "in-library RCCL collectives", "torch-nccl": "torch.distributed communicator, torch's RCCL",
               "torch": "torch.distributed communicator, host-staged"}[comm_name]
        par = f"one proof sharded by cosets over {world} GPUs ({how})"
    elif world > 1:
        par = f"{world} independent proofs (one trace per GPU): sharded proving could not be set up"
    else:
        par = "1 GPU"
    out = {
        "metric": "trace rows/sec proved (2^20-row trace, 96-bit sec)",
        "value": rows_per_step / (dt / args.steps),
        "unit": "trace rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": "u64 (Goldilocks field, p = 2^64 - 2^32 + 1)",
        "data": "synthetic (DummyMidenAir-shaped trace, numpy PCG64)",
        "config": {"workload": f"full proof of miden:{log_n}:51:8 (DummyMidenAir 2^{log_n} x 51 + 8 EF aux), 96-bit production PCS "
                               "params (blowup 8, FRI arity 4, 27 queries, PoW 4/12/16), Poseidon2 LMCS; trace resident in HBM, "
                               "transcript on host",
                   "log_trace_rows": log_n, "main_width": 51, "aux_width_ef": 8, "log_blowup": 3,
                   "proof_bytes": len(runner.proof.bytes) if runner.proof else None, "parallelism": par},
    }
    if fallback:
        out["config"]["fallback"] = fallback
    if comm_log:
        out["config"]["comm"] = {"chosen": comm_name, "mode": mode, "attempts": comm_log, "collective_timeout_s": float(os.environ.get("MH_COMM_TIMEOUT_S", "120")),
                                 "note": "rank 0's view; every attempt runs on a watchdog thread (MIDEN_BENCH_COMM_TIMEOUT) and the ranks agree on its outcome "
                                         "over the gloo control plane; inside the library every collective is bounded by MH_COMM_TIMEOUT_S (error code, no hang)"}

    def shutdown():
        if comm is not None and hasattr(comm, "close"):
            comm.close()
        if world > 1:
            dist.destroy_process_group()

    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        shutdown()
        return

    prof_timed = ctx.prof()
    ctx.prof_filter(None)
    ctx.prof_reset()
    bd_steps = max(1, min(args.steps, 2 if mode == "sharded" else 5))
    t_bd = time.perf_counter()
    for _ in range(bd_steps):
        runner.step()
    barrier()
    bd_ms = (time.perf_counter() - t_bd) / bd_steps * 1e3
    prof = ctx.prof()
    ctx.prof_enable(False)
    if mode == "sharded":
        # the measured split of this rank's time next to the model of DESIGN.md section 5 (miden-vm_amd/sharding.py), so that the
        # line can be read against a prediction: sharded kernels, the replicated inverse transforms, collectives
        from miden_vm_amd import sharding as _sh
        per = lambda k: prof.get(k, {}).get("ms", 0.0) / bd_steps
        comm_ms = {k: round(per(k), 3) for k in prof if k.startswith("comm_")}
        out["sharded_breakdown"] = {
            "comm_ms": comm_ms, "comm_calls_per_proof": {k: prof[k]["count"] / bd_steps for k in prof if k.startswith("comm_")},
            "replicated_intt_ms": round(per("lde_intt"), 3), "ood_ms": round(per("deep_ood_eval"), 3),
            "kernel_ms": round(sum(per(k) for k in prof if not k.startswith(("comm_", "span:")) and k != "lde_intt"), 3),
            # the model scales the 2^24 single-GPU spans linearly: meaningful for large proofs only (fixed latencies dominate small ones)
            "model": ({k: (round(v, 2) if isinstance(v, float) else v) for k, v in _sh.predict_sharded_ms(world, log_n).items()}
                      if log_n >= 22 else None),
            "model_note": "per-rank ms predicted from the single-GPU spans of profiles/r03_config_shapes.txt (2^24: 739 ms) with "
                          "60 GB/s per xGMI link and direction; replicated = inverse NTTs + host-serial tree tops / transcript"}
    pmc_json = next(f for f in ("r06_pmc_leaf_absorb.json", "r05_pmc_leaf_absorb.json", "r04_pmc_leaf_absorb.json", "r03_pmc_leaf_absorb.json", "r02_pmc_leaf_absorb.json")
                    if os.path.exists(os.path.join(ROOT, "profiles", f)))
    # the dominant class of the full pass must be the one the timed region recorded; if a configuration moves it, say so and fall back
    full_dom = max((k for k in prof if not k.startswith(("comm_", "span:")) and k != "lde_intt"), key=lambda k: prof[k]["ms"]) if prof else None
    live = prof_timed if (DOMINANT in prof_timed and full_dom == DOMINANT) else prof
    live_steps = args.steps if live is prof_timed else bd_steps
    out["roofline"] = roofline(live, pmc_json)
    if out["roofline"] is not None:
        out["roofline"]["measured_over"] = ("the timed region" if live is prof_timed else
                                            f"the untimed breakdown pass (dominant class here is {full_dom}, not {DOMINANT})")
    try:
        perms = (8 << log_n) * (7 + 2 + 2) // (world if mode == "sharded" else 1)  # per rank
        out["roofline_valu"] = valu_roofline(ctx, live, perms, live_steps, pmc_json)
    except Exception as e:
        out["roofline_valu"] = {"error": repr(e)[:200]}
    out["breakdown_pass"] = {"steps": bd_steps, "ms_per_step_with_every_class_recorded": bd_ms,
                             "note": "kernels / spans / sharded_breakdown: a second, untimed pass with every kernel class and span recorded "
                                     "(event records are barrier packets: ~0.5 ms per 2^20-row proof); the timed region records the dominant class only"}
    out["kernels"] = {k: {"ms_per_step": v["ms"] / bd_steps, "launches_per_step": v["count"] / bd_steps,
                          "alg_GBps": (v["bytes"] / 1e9) / (v["ms"] / 1e3) if v["ms"] > 0 else None}
                      for k, v in prof.items() if not k.startswith("span:")}
    # the same timings under the reference's tracing span names, stage spans included
    out["spans"] = {k[5:]: round(v["ms"] / bd_steps, 4) for k, v in prof.items() if k.startswith("span:")}
    if mode == "sharded" and not args.no_extras:
        # the workload that matters, next to the DummyMidenAir headline: the real statement, one proof over all ranks
        try:
            def _max_over_ranks(x):
                tt = torch.tensor([x], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                return float(tt.item())
            from miden_vm_amd import sharding as _shd
            res = miden_real_sharded_probe(pkg, ctx, comm, _shd, barrier, _max_over_ranks, rank,
                                           iters=int(os.environ.get("MIDEN_BENCH_REAL_ITERS", "9250")))
            out["miden_real_sharded"] = res
        except Exception as e:
            out["miden_real_sharded"] = {"error": repr(e)[:300]}
    if world == 1 and not args.no_extras:
        try:  # the same proof with the trace upload inside the timed region (page-locked source buffer)
            pin, owner = pkg.pinned_array(ctx.lib, runner.host_trace.shape)
            pin[:] = runner.host_trace
            runner.step_with_upload(pin)
            barrier()
            t1 = time.perf_counter()
            n_h2d = max(3, min(args.steps, 10))
            for _ in range(n_h2d):
                runner.step_with_upload(pin)
            barrier()
            d = (time.perf_counter() - t1) / n_h2d
            # the same from a COLUMN-major host matrix (what a trace builder that writes columns would hand over): it pipelines
            pin_t, owner_t = pkg.pinned_array(ctx.lib, runner.host_trace.shape[::-1])
            pin_t[:] = runner.host_trace.T
            runner.step_with_cols_upload(pin_t)
            barrier()
            t2 = time.perf_counter()
            for _ in range(n_h2d):
                runner.step_with_cols_upload(pin_t)
            barrier()
            d_cols = (time.perf_counter() - t2) / n_h2d
            out["h2d_inclusive_colmajor_host"] = {"ms_per_step": d_cols * 1e3, "value": (1 << log_n) / d_cols, "unit": "trace rows/s",
                                                  "note": "mh_trace_upload_cols_async: columns in groups of eight, LDE of a group when it has landed; "
                                                          "NOT the reference's RowMajorMatrix hand-over (that is h2d_inclusive)"}
            out["h2d_inclusive"] = {"value": (1 << log_n) / d, "unit": "trace rows/s", "ms_per_step": d * 1e3, "steps": n_h2d,
                                    "upload_bytes": int(runner.host_trace.nbytes),
                                    "note": "mh_trace_upload_async (DMA from mh_host_alloc memory + transpose on the copy stream) inside the timed "
                                            "region.  ONE row-major matrix: every column NTT needs all rows and column windows of a row-major host "
                                            "buffer move at 16-36 GB/s (PCIe read tags, profiles/r03_h2dbench.txt), so the 428 MB / 57 GB/s copy is "
                                            "exposed; with several matrices (miden_shape) all but the first are hidden"}
            del pin, owner
        except Exception as e:
            out["h2d_inclusive"] = {"error": repr(e)[:200]}
        if args.extras:
            try:
                out["miden_shape"] = miden_shape_probe(pkg, ctx)
            except Exception as e:
                out["miden_shape"] = {"error": repr(e)[:200]}
        try:
            from miden_vm_amd.testing import core_trace as _ct
            t_gen = time.perf_counter()
            real_inputs = _ct.prove_inputs(_ct.CoreVM(stack_inputs=list(range(16))), _ct.bench_program(9250))
            t_gen = time.perf_counter() - t_gen
            out["miden_real"] = miden_real_probe(pkg, ctx, inputs=(real_inputs, t_gen))
            c3 = pkg.Ctx(dev_index)
            try:  # ProvingOptions::default() = Blake3_256: the configuration the reference's published figure is quoted on
                out["miden_real_blake3"] = miden_real_probe(pkg, c3, inputs=real_inputs, lmcs="blake3")
            finally:
                c3.close()
            # BASELINE.json configs[0]: a ~2^16-row program, the reference's own CPU-runnable case, as a latency
            # point of the real statement: 575 iterations of the same loop body = 2^16 core rows
            if args.extras:
                small = _ct.prove_inputs(_ct.CoreVM(stack_inputs=list(range(16))), _ct.bench_program(575))
                r16 = miden_real_probe(pkg, ctx, inputs=small, steps=5)
                out["miden_real_2p16"] = {k: r16[k] for k in ("log_trace_heights", "ms_per_proof", "rows_per_s", "h2d_inclusive_ms", "proof_bytes",
                                                               "verifies_with_eval_external", "kernels_ms")}
        except Exception as e:
            out["miden_real"] = {"error": repr(e)[:300]}
        try:
            out["precompile_full_session"] = precompile_full_session_probe(pkg, ctx)
        except Exception as e:
            out["precompile_full_session"] = {"error": repr(e)[:300]}
    if world == 1 and args.extras and not args.no_extras:
        try:
            out["jit_load"] = jit_load_probe(pkg, ctx)
        except Exception as e:
            out["jit_load"] = {"error": repr(e)[:200]}
        try:
            out["chiplets_air"] = chiplets_air_probe(pkg, ctx)
        except Exception as e:
            out["chiplets_air"] = {"error": repr(e)[:200]}
        try:
            out["precompile_session"] = precompile_session_probe(pkg, ctx)
        except Exception as e:
            out["precompile_session"] = {"error": repr(e)[:300]}
        try:
            out["chunk_session"] = chunk_session_probe(pkg, ctx)
        except Exception as e:
            out["chunk_session"] = {"error": repr(e)[:300]}
        try:
            out["chunk_poseidon2_session"] = chunk_poseidon2_session_probe(pkg, ctx)
        except Exception as e:
            out["chunk_poseidon2_session"] = {"error": repr(e)[:300]}
        try:
            out["keccak_hash_session"] = keccak_hash_session_probe(pkg, ctx)
        except Exception as e:
            out["keccak_hash_session"] = {"error": repr(e)[:300]}
        try:
            out["uint_add_session"] = uint_add_session_probe(pkg, ctx)
        except Exception as e:
            out["uint_add_session"] = {"error": repr(e)[:300]}
        try:
            out["ec_store_session"] = ec_store_session_probe(pkg, ctx)
        except Exception as e:
            out["ec_store_session"] = {"error": repr(e)[:300]}
        try:
            out["ec_add_session"] = ec_add_session_probe(pkg, ctx)
        except Exception as e:
            out["ec_add_session"] = {"error": repr(e)[:300]}
        try:
            out["uint_arith_session"] = uint_arith_session_probe(pkg, ctx)
        except Exception as e:
            out["uint_arith_session"] = {"error": repr(e)[:300]}
        try:
            out["ec_msm_session"] = ec_msm_session_probe(pkg, ctx)
        except Exception as e:
            out["ec_msm_session"] = {"error": repr(e)[:300]}
        try:
            # the service-level probes run in a process of their own (tools/bench_inflight_h2d.py, no torch in it): measured in THIS
            # process, which also hosts PyTorch's HIP runtime, the same loops lose the copy / kernel overlap (k = 1 with its uploads
            # pipelined: 56.0 ms here against 47.8 ms stand-alone on the same box)
            import subprocess
            res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_inflight_h2d.py"), "3", "6", str(log_n)], capture_output=True, text=True,
                                 timeout=600, env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", str(dev_index))))
            lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
            out["in_flight_h2d"], out["pipelined_h2d"], out["in_flight"] = lines[0], lines[1], lines[2]
        except Exception as e:
            out["in_flight"] = {"error": repr(e)[:200]}
        try:  # the same proof under the reference's other StarkConfigs (Blake3_256 = its DEFAULT ProvingOptions)
            out["hash_configs"] = {"note": "mh_prove of the same instance on a context set to another LMCS hasher / challenger "
                                           "(mh_ctx_set_lmcs); rpo / rpx at 2^16 rows (Rescue Prime is supported, not tuned)",
                                   "blake3": hash_config_probe(pkg, dev_index, log_n, "blake3"),
                                   "keccak": hash_config_probe(pkg, dev_index, log_n, "keccak"),
                                   "rpo_2p16": hash_config_probe(pkg, dev_index, min(log_n, 16), "rpo", steps=2),
                                   "rpx_2p16": hash_config_probe(pkg, dev_index, min(log_n, 16), "rpx", steps=2)}
        except Exception as e:
            out["hash_configs"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(runner, args.cpu_log_n)
    elif rank == 0:
        out["cpu_baseline"] = None
    if world > 1:
        out["scale_note"] = (f"N = 1 proves 2^{args.log_n} rows per step, N > 1 ONE proof of 2^{args.shard_log_n} rows sharded over the GPUs: a speed-up "
                             "against the N = 1 line is a ratio of rows/s on two instances.  One MI355X proves 2^24 x 51 + 8 EF at 22.7 M rows/s "
                             "(739 ms, profiles/r03_config_shapes.txt; 2^20: 22.8 M rows/s) -- within 1 % of the 2^20 rate, so the ratio of the "
                             "lines is the strong-scaling speed-up of the 2^24 instance to that accuracy")
    if rank == 0:
        # The driver keeps the parsed contract keys and the last 4 kB of the line: what matters goes LAST, compact.
        def top_kernels(d, k=4):
            km = (d or {}).get("kernels_ms") or {}
            return dict(sorted(km.items(), key=lambda kv: -kv[1])[:k])
        def brief(d, keys):
            return {k: d.get(k) for k in keys if isinstance(d, dict) and k in d} if isinstance(d, dict) else d
        summary = {"headline_ms": round(out["ms_per_step"], 3), "headline_rows_per_s": round(out["value"]),
                   "roofline_frac_hbm": (out.get("roofline") or {}).get("frac"), "roofline_frac_valu": (out.get("roofline_valu") or {}).get("frac"),
                   "h2d_inclusive_ms": (out.get("h2d_inclusive") or {}).get("ms_per_step")}
        for key in ("miden_real", "miden_real_blake3", "precompile_full_session"):
            d = out.get(key)
            if isinstance(d, dict) and "error" not in d:
                summary[key] = {**brief(d, ("log_trace_heights", "ms_per_proof", "h2d_inclusive_ms", "proof_bytes", "verifies_with_eval_external")),
                                "top_kernels_ms": top_kernels(d)}
            elif d is not None:
                summary[key] = d
        if comm_log:  # the bring-up ladder in the part of the line the driver's tail keeps
            summary["comm"] = {"chosen": comm_name, "mode": mode, "fallback": fallback,
                               "attempts": [{"choice": a["choice"], "ok": a["ok_on_rank0"], "s": round(sum(t for _, t in a["steps_s"]), 2),
                                             **({"error": a["error"][:120]} if "error" in a else {})} for a in comm_log]}
        if isinstance(out.get("miden_real_sharded"), dict):
            summary["miden_real_sharded"] = brief(out["miden_real_sharded"], ("ms_per_proof", "rows_per_s", "log_trace_heights", "error"))
        if isinstance(out.get("cpu_baseline"), dict):
            summary["cpu_baseline"] = brief(out["cpu_baseline"], ("value", "unit", "cores", "kind"))
        first = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]
        last = ["roofline", "roofline_valu", "cpu_baseline", "h2d_inclusive", "scale_note"]
        bulky = [k for k in out if k not in first and k not in last]
        out = {**{k: out[k] for k in first if k in out}, **{k: out[k] for k in bulky}, **{k: out[k] for k in last if k in out}, "summary": summary}
        print(json.dumps(out), flush=True)
    shutdown()


if __name__ == "__main__":
    main()
