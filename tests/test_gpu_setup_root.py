"""The device and the host agree on the verifying key (run with -m gpu).

  * mh_precompile_preprocessed_root (the byte-pair table committed on the device) == mh_precompile_setup_root (derived on the host),
    for the five hashers;
  * mh_commit_traces == mh_commit_host on mixed heights (lifting, two height groups) under Poseidon2 and Blake3;
  * a device session proof (the statement of tests/test_gpu_precompile_c_abi.py) is accepted by mh_verify_precompile with no root
    given, refused for another public root, and refused for an explicit wrong setup root because of the setup root;
  * mh_prove_precompile_traces refuses a byte-pair trace of 2^15 rows with the code and message of mh_prove_precompile."""
import numpy as np
import pytest
import oracle_binding as ob
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu
HASHERS = ["poseidon2", "blake3", "keccak", "rpo", "rpx"]
INPUTS = [b"", b"abc", b"abc", bytes(range(200))]  # the session of tests/test_gpu_precompile_c_abi.py


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pc(ctx):
    return pkg.Precompile(ctx)


@pytest.mark.parametrize("hasher", HASHERS)
def test_device_and_host_agree_on_the_setup_root(pc, hasher):
    assert [int(x) for x in pc.preprocessed_root(hasher)] == [int(x) for x in pkg.precompile_setup_root(hasher)]


@pytest.mark.parametrize("log_blowup", [1, 3])
@pytest.mark.parametrize("hasher", ["poseidon2", "blake3"])
def test_commit_traces_equals_commit_host_on_mixed_heights(ctx, hasher, log_blowup):
    mats = [np.random.default_rng(10 + i).integers(0, pkg.P, (1 << lh, w), dtype=np.uint64) for i, (lh, w) in enumerate([(3, 3), (5, 10), (5, 1)])]
    ctx.set_lmcs(hasher)
    try:
        com = pkg.commit_traces(ctx, [ctx.upload_trace(m) for m in mats], log_blowup)
        assert [int(x) for x in com.root()] == [int(x) for x in pkg.commit_host(mats, log_blowup, lmcs=hasher)]
    finally:
        ctx.set_lmcs("poseidon2")


@pytest.fixture(scope="module")
def session():
    _, traces, info = PT.precompile_session(INPUTS, lambda *a: ob.lookup_build_aux(*a))
    return traces, [int(x) for x in info["public_root"]]


def test_device_proof_verifies_against_the_derived_root(pc, session):
    traces, root = session
    proof = pc.prove(traces, root)
    ok, dig = pkg.verify_precompile(None, root, proof.bytes)
    assert ok and (dig == proof.digest).all(), dig
    ok, dig = pkg.verify_precompile(pc.preprocessed_root(), root, proof.bytes)
    assert ok and (dig == proof.digest).all(), dig
    ok, msg = pkg.verify_precompile(None, [(root[0] + 1) % PA.P] + root[1:], proof.bytes)
    assert not ok and "setup" not in msg, msg
    wrong = [int(x) for x in pc.preprocessed_root()]
    wrong[0] = (wrong[0] + 1) % PA.P
    ok, msg = pkg.verify_precompile(wrong, root, proof.bytes)
    assert not ok and "preprocessed_root is not the byte-pair table's setup commitment" in msg, msg


def test_traces_entry_checks_the_byte_pair_height(ctx, pc, session):
    traces, root = session
    short = list(traces)
    short[3] = traces[3][: 1 << 15]
    with pytest.raises(pkg.MidenHipError) as host:
        pc.prove(short, root)
    with pytest.raises(pkg.MidenHipError) as dev:
        pc.prove([ctx.upload_trace(t) for t in short], root)
    assert str(dev.value) == str(host.value) and "libmidenhip error 1:" in str(host.value) and "2^16 rows" in str(host.value)
