"""CPU-only: the constraint checker's ABI (include/midenhip.h mh_check_*) agrees across the header, the Rust declarations and the
Python layer, and the Python entry points fail loudly without a GPU (no CPU fallback)."""
import ctypes as C
import os, re, shutil, subprocess
import pytest
from __graft_entry__ import load_package, ROOT

CHECK_FUNCS = ["mh_check_constraints", "mh_constraint_fold", "mh_check_miden", "mh_check_miden_traces", "mh_check_precompile", "mh_check_precompile_traces"]


def header():
    return open(os.path.join(ROOT, "include", "midenhip.h")).read()


def define(src, name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
    return int(m.group(1)) if m else None


def test_header_declares_the_checker():
    h = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for f in CHECK_FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
    assert define(h, "MH_ERR_UNSATISFIED") == 6
    assert define(h, "MH_CHECK_EXACT") == 1
    assert "mh_check_entry" in h


def test_values_agree_across_header_rust_and_python():
    pkg = load_package()
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    for name in ("MH_ERR_UNSATISFIED", "MH_CHECK_EXACT"):
        m = re.search(r"pub const " + name + r": c_int = (\d+);", rs)
        assert m and int(m.group(1)) == define(header(), name) == getattr(pkg, name), name
    for f in CHECK_FUNCS:
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
    # the Rust struct lists the C struct's fields in order
    body = re.search(r"pub struct mh_check_entry \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [n for n, _ in pkg.CheckEntry._fields_]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_ctypes_entry_matches_the_c_struct(tmp_path):
    pkg = load_package()
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "midenhip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mh_check_entry), offsetof(mh_check_entry, rows), '
                   'offsetof(mh_check_entry, first_row), offsetof(mh_check_entry, value), offsetof(mh_check_entry, constraint)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, rows, first, value, cons = map(int, subprocess.check_output([str(exe)], text=True).split())
    E = pkg.CheckEntry
    assert C.sizeof(E) == size == 40
    assert (E.rows.offset, E.first_row.offset, E.value.offset, E.constraint.offset) == (rows, first, value, cons)


def test_library_exports_the_checker():
    pkg = load_package()
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = pkg.load_library()
    for f in CHECK_FUNCS:
        assert hasattr(lib, f), f


def test_check_without_gpu_raises():
    pkg = load_package()
    if os.path.exists(pkg.LIB_PATH) and pkg.load_library().mh_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(pkg.MidenHipError):
        pkg.Miden(pkg.Ctx(0)).check([[0] * 51] * 2, [[0] * 22] * 2, [[0] * 16] * 2, [0] * 32, [0] * 8)
