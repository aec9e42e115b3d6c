"""GPU: the DEEP quotient assembled on ONE coset and extended by a coset LDE (csrc/deep.hip, the default whenever the rank stores
at least two cosets and the max trace height is >= DEEP_ONE_COSET_MIN_LOG_N = 2) against the assemble kernel on EVERY coset
(MH_DEEP_ALL_COSETS=1, read at each call).  Field arithmetic is exact and every stored felt canonical, so the FRI layer -- and with
it the proof -- must be identical byte for byte; every case proves the same statement both ways in one process and hands the
default proof to the oracle verifier.  Which path ran is read off the profile: `deep_extend` is recorded by the one-coset path only.

log_N = 0 cannot be reached through the prover (a trace needs at least two rows); the case below pins that down for both settings,
the height-below-the-minimum fallback is exercised at log_N = 1."""
import numpy as np
import pytest
import oracle_binding as ob
import airs as A
from __graft_entry__ import load_package
from miden_vm_amd import dag

pytestmark = pytest.mark.gpu
FAST = dict(log_blowup=3, log_folding_arity=2, log_final_degree=2, folding_pow_bits=1, deep_pow_bits=2, num_queries=5,
            query_pow_bits=3)
MIN_LOG_N = 2  # kernels.hpp DEEP_ONE_COSET_MIN_LOG_N


@pytest.fixture(scope="module")
def ctx():
    pkg = load_package()
    c = pkg.Ctx(0)
    yield c
    c.close()


def prove_both(ctx, monkeypatch, airs_, traces, pub, params, lmcs="poseidon2"):
    """The statement proved with the assemble kernel on every coset, then by the default path.  Returns (default proof, whether the
    default path extended from one coset)."""
    pkg = load_package()
    ob.set_lmcs(lmcs)
    ctx.set_lmcs(lmcs)
    try:
        dairs = [pkg.DeviceAir(ctx, a) for a in airs_]
        dtr = [ctx.upload_trace(t) for t in traces]
        st, pre = ob.challenger_state(), ob.protocol_pre_observe(params, pub)

        def aux_builder(idx, rnd):
            a = airs_[idx]
            if a.build_aux is None:
                return np.zeros((traces[idx].shape[0], 2 * a.aux_width), dtype=np.uint64), [0] * (2 * a.num_aux_values)
            return a.build_aux(traces[idx], rnd[:a.num_randomness])

        cb = aux_builder if any(a.build_aux is not None for a in airs_) else None
        profs = {}
        proofs = {}
        for mode in ("all", "default"):
            if mode == "all":
                monkeypatch.setenv("MH_DEEP_ALL_COSETS", "1")
            else:
                monkeypatch.delenv("MH_DEEP_ALL_COSETS")
            ctx.prof_enable(True)
            ctx.prof_reset()
            proofs[mode] = pkg.prove(ctx, dairs, dtr, pub, params, st, pre, cb)
            profs[mode] = ctx.prof()
            ctx.prof_enable(False)
        old, new = proofs["all"], proofs["default"]
        assert "deep_extend" not in profs["all"] and profs["all"]["deep_assemble"]["count"] == 1
        assert new.bytes == old.bytes
        assert new.fields.size == old.fields.size and (new.fields == old.fields).all()
        assert new.commitments.shape == old.commitments.shape and (new.commitments == old.commitments).all()
        assert (new.digest == old.digest).all()
        ok, msg = ob.verify(airs_, new.log_trace_heights, pub, {"fields": new.fields, "commitments": new.commitments}, params)
        assert ok, msg
        assert profs["default"]["deep_assemble"]["count"] == 1
        extended = "deep_extend" in profs["default"]
        if extended:
            # one coset instead of 2^log_blowup: the assemble kernel's algorithmic bytes shrink by exactly that factor
            assert profs["default"]["deep_extend"]["count"] == 1
            assert profs["default"]["deep_assemble"]["bytes"] * (1 << params["log_blowup"]) == profs["all"]["deep_assemble"]["bytes"]
        else:
            assert profs["default"]["deep_assemble"]["bytes"] == profs["all"]["deep_assemble"]["bytes"]
        return new, extended
    finally:
        ob.set_lmcs("poseidon2")
        ctx.set_lmcs("poseidon2")
        ctx.prof_enable(False)


@pytest.mark.parametrize("log_n", [MIN_LOG_N, 8, 12, 13])
def test_heights_around_the_ntt_tile(ctx, monkeypatch, log_n):
    # 2^12 is the NTT tile: 12 is the last single-pass plan, 13 the first with a strided pass -- for the 2-column call of the extension
    _, extended = prove_both(ctx, monkeypatch, [dag.dummy_miden_air(11, 2)], [A.dummy_trace(log_n, 11)], [], FAST)
    assert extended


def test_dummy_miden_shape(ctx, monkeypatch):
    _, extended = prove_both(ctx, monkeypatch, [dag.dummy_miden_air(51, 8)], [A.dummy_trace(10, 51)], [], ob.PROD_PARAMS)
    assert extended


def test_mixed_heights_odd_width(ctx, monkeypatch):
    # heights 2^9 and 2^7: the shorter matrices are read through nm_mask as lifted columns f(x^4); 11 + 12 = 23 main columns, and
    # each odd-width matrix leaves the two-column unrolled loop with a remainder
    airs_ = [dag.dummy_miden_air(11, 2), dag.dummy_miden_air(12, 1)]
    _, extended = prove_both(ctx, monkeypatch, airs_, [A.dummy_trace(9, 11, seed=2), A.dummy_trace(7, 12, seed=3)], [], FAST)
    assert extended
    _, extended = prove_both(ctx, monkeypatch, airs_[::-1], [A.dummy_trace(9, 12, seed=3), A.dummy_trace(7, 11, seed=2)], [], FAST)
    assert extended


def test_more_columns_than_one_flush(ctx, monkeypatch):
    # 141 main columns in one matrix: the delayed-reduction accumulators are flushed inside the column loop (DEEP_FLUSH = 128)
    _, extended = prove_both(ctx, monkeypatch, [dag.dummy_miden_air(141, 2)], [A.dummy_trace(8, 141, seed=4)], [], FAST)
    assert extended


def test_two_cosets(ctx, monkeypatch):
    # log_blowup = 1: the smallest extension (the Fibonacci AIR has quotient degree 2)
    t, pub = A.fib_trace(8)
    prm = dict(FAST, log_blowup=1, log_folding_arity=1, log_final_degree=1)
    _, extended = prove_both(ctx, monkeypatch, [A.fib_air()], [t], pub, prm)
    assert extended


def test_fallback_below_the_minimum_height(ctx, monkeypatch):
    t, pub = A.fib_trace(MIN_LOG_N - 1)
    _, extended = prove_both(ctx, monkeypatch, [A.fib_air()], [t], pub, FAST)
    assert not extended


@pytest.mark.parametrize("all_cosets", [True, False])
def test_one_row_traces_are_refused_either_way(ctx, monkeypatch, all_cosets):
    # log_N = 0 never reaches the DEEP quotient: the prover refuses the statement, with the switch and without it
    pkg = load_package()
    if all_cosets:
        monkeypatch.setenv("MH_DEEP_ALL_COSETS", "1")
    t, pub = A.fib_trace(0)
    with pytest.raises(pkg.MidenHipError, match="at least 2 rows"):
        pkg.prove(ctx, [pkg.DeviceAir(ctx, A.fib_air())], [ctx.upload_trace(t)], pub, FAST, ob.challenger_state(),
                  ob.protocol_pre_observe(FAST, pub))


def test_blake3_leaves(ctx, monkeypatch):
    # the layer feeds the byte-hash FRI leaf kernel
    _, extended = prove_both(ctx, monkeypatch, [dag.dummy_miden_air(11, 2)], [A.dummy_trace(8, 11)], [], FAST, lmcs="blake3")
    assert extended


def test_sharded_two_ranks(monkeypatch):
    """Two thread ranks, blowup 8: each stores four cosets (lbl = 2), rank 1 from coset0 = 4, and extends from its own first coset --
    no collective is added.  Both ranks' proofs, either way, are the single-GPU proof."""
    from test_gpu_sharded import _thread_ranks
    airs_, traces = [dag.dummy_miden_air(11, 2)], [A.dummy_trace(9, 11, seed=6)]
    st, pre = ob.challenger_state(), ob.protocol_pre_observe(FAST, [])

    def body(pkg, sharding, rank, ctx, comm):
        dairs = [pkg.DeviceAir(ctx, a) for a in airs_]
        dtr = [ctx.upload_trace(t) for t in traces]
        ctx.prof_enable(True)
        ctx.prof_reset()
        got = sharding.prove_sharded(pkg, ctx, comm, dairs, dtr, [], FAST, st, pre, None)
        prof = ctx.prof()
        ctx.prof_enable(False)
        ref = pkg.prove(ctx, dairs, dtr, [], FAST, st, pre, None) if rank == 0 else None
        return got, prof, ref

    out = {}
    for mode in ("all", "default"):
        if mode == "all":
            monkeypatch.setenv("MH_DEEP_ALL_COSETS", "1")  # set before the rank threads start: they only read it
        else:
            monkeypatch.delenv("MH_DEEP_ALL_COSETS")
        out[mode] = _thread_ranks(2, body)
    ref = out["all"][0][2]
    assert out["default"][0][2].bytes == ref.bytes
    for mode in ("all", "default"):
        for got, prof, _ in out[mode]:
            assert got.bytes == ref.bytes
            assert (got.commitments == ref.commitments).all() and (got.digest == ref.digest).all()
            assert ("deep_extend" in prof) == (mode == "default")
    ok, msg = ob.verify(airs_, ref.log_trace_heights, [], {"fields": ref.fields, "commitments": ref.commitments}, FAST)
    assert ok, msg
