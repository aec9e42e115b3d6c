"""Regenerate tests/golden/rust_kit_facts.json: the answers a miden-vm checkout gives to every query of
tools/ref_fixtures/check_imports.py for the Rust kits as they stand (does a path resolve, does a method or field exist, how many
parameters, does a Cargo feature exist, does an API pattern occur), plus the resolver probes of tests/test_rust_kit_imports.py.
Verdicts only (booleans, counts, "ok" / "external" / null), no text of the checkout.

    python tests/golden/make_rust_kit_facts.py <miden-vm checkout>

Re-run after a kit under tools/ref_fixtures/ changes what it imports or calls; tests/test_rust_kit_imports.py replays the file."""
import json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
KIT = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools", "ref_fixtures")
sys.path.insert(0, KIT)
import check_imports as ci  # noqa: E402


def main():
    ref = sys.argv[1]
    rec = ci.RecordingWorkspace(ci.Workspace(ref))
    problems, _ = ci.check(rec, KIT)
    for kind, args, want in ci.RESOLVER_PROBES:
        got = getattr(rec, kind)(*args)
        assert got == want, (kind, args, got)
    out = os.path.join(HERE, "rust_kit_facts.json")
    json.dump(dict(sorted(rec.facts.items())), open(out, "w"), indent=0)
    print(f"{len(rec.facts)} answers -> {out}; {len(problems)} problem(s) of the kits against this checkout")


if __name__ == "__main__":
    main()
