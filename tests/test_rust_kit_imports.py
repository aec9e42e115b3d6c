"""The Rust kits (tools/ref_fixtures/src/main.rs, src/bin/export_dag.rs: never compiled here, no cargo in the image) checked
against the reference checkout WITHOUT a compiler: every `use` path resolves through the workspace's modules and re-exports,
every associated function / public field they touch exists, every Cargo dependency is a workspace dependency, and the calls
into crates outside the workspace (p3-air's symbolic builder, wincode) have a precedent in the reference's own sources.  A moved
import fails here instead of on the maintainer's first `cargo build`.  The reference's answers (verdicts only) are replayed from
tests/golden/rust_kit_facts.json, recorded from a checkout by tests/golden/make_rust_kit_facts.py; the resolver itself runs on a
miniature workspace the test writes."""
import json, os, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_fixtures"))
import check_imports as ci  # noqa: E402

FACTS = json.load(open(os.path.join(ROOT, "tests", "golden", "rust_kit_facts.json")))

# A made-up workspace with the shapes the resolver must follow: an inline module re-exporting another crate's item and module, a
# file module, names imported from a crate outside the workspace (one glob), impl blocks and public fields.
MINI = {
    "Cargo.toml": '[workspace]\nmembers = ["front", "back"]\n',
    "front/Cargo.toml": '[package]\nname = "mini-front"\n',
    "front/src/lib.rs": "pub mod stark {\n    pub use mini_back::prover::ProverInstance;\n    pub use mini_back::proof;\n"
                        "    pub mod air {\n        pub use p3_air::{Air, AirBuilder};\n        pub mod symbolic { pub use p3_air::symbolic::*; }\n    }\n}\n"
                        "pub mod config;\n",
    "front/src/config.rs": "// pub fn commented_out()\npub fn poseidon2_config(params: u32, digest: u64) -> u32 { params }\n",
    "back/Cargo.toml": '[package]\nname = "mini-back"\n',
    "back/src/lib.rs": "pub mod prover;\npub mod proof {\n    pub struct StarkProofData { pub quotient_commit: u64, private: u8 }\n}\n",
    "back/src/prover/mod.rs": "pub struct ProverInstance;\nimpl ProverInstance {\n    pub fn prove(&self, challenger: u64) -> u8 { 0 }\n}\n",
}


def test_use_tree_parser():
    got = ci.parse_use_tree("a::b::{self, c, d::{e as f, g::*}}")
    assert got == [(["a", "b"], "b"), (["a", "b", "c"], "c"), (["a", "b", "d", "e"], "f"), (["a", "b", "d", "g"], "*")]
    items = ci.split_items("pub use x::{a, b}; const K: T = T { a: 1 }; pub fn f() { g(); } mod m { pub struct S; }")
    assert len(items) == 4 and items[0].startswith("pub use") and items[3].startswith("mod m")


def test_resolver_follows_modules_reexports_and_catches_a_wrong_path(tmp_path):
    for rel, text in MINI.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(text)
    ws = ci.Workspace(str(tmp_path))
    assert ws.resolve(["mini_front", "stark", "ProverInstance"]) == "ok"               # inline mod + pub use of another crate
    assert ws.resolve(["mini_front", "stark", "proof", "StarkProofData"]) == "ok"      # re-exported sub-module
    assert ws.resolve(["mini_front", "config", "poseidon2_config"]) == "ok"            # file module
    assert ws.resolve(["mini_front", "stark", "air", "Air"]) == "external"             # named import from outside the workspace
    assert ws.resolve(["mini_front", "stark", "air", "symbolic", "SymbolicAirBuilder"]) == "external"  # glob of p3-air: unverifiable
    assert ws.resolve(["mini_front", "stark", "air", "BasedVectorSpace"]) is None       # a name nobody imports there
    assert ws.resolve(["mini_front", "stark", "NoSuchThing"]) is None
    assert ws.has_method("ProverInstance", "prove") and not ws.has_method("ProverInstance", "no_such_method")
    assert ws.signature("ProverInstance", "prove", ["u64"]) == {"params": 1, "mentions": [True]}
    assert ws.signature("ProverInstance", "prove", ["u32"]) == {"params": 1, "mentions": [False]}
    assert ws.has_field("StarkProofData", "quotient_commit") and not ws.has_field("StarkProofData", "private")
    assert ws.workspace_dependency("members") and not ws.workspace_dependency("mini-back")
    # the same queries against the reference, as recorded from it
    ref = ci.RecordedWorkspace(FACTS)
    for kind, args, want in ci.RESOLVER_PROBES:
        assert getattr(ref, kind)(*args) == want, (kind, args)
    with pytest.raises(KeyError):
        ref.resolve(["miden_crypto", "never", "asked"])


def test_every_identifier_the_kits_use_exists_in_the_reference():
    problems, report = ci.check(ci.RecordedWorkspace(FACTS), os.path.join(ROOT, "tools", "ref_fixtures"))
    assert not problems, "\n".join(problems)
    assert sum(1 for r in report if r[2] == "ok") >= 15 and len(report) > 80
