"""The C-ABI library loads (no GPU needed) and exports exactly what include/pdmp_mi355.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header="pdmp_mi355.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pdmp_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree(pkg):
    assert declared_functions() == sorted(pkg._lib.EXPORTED_SYMBOLS)
    assert declared_functions("pdmp_debug.h") == sorted(pkg._lib.DEBUG_SYMBOLS)  # diagnostics live in their own header
    assert not [f for f in declared_functions() if f.startswith("pdmp_debug")]


def test_library_reads_no_environment(pkg):
    """The ABI promises "no globals": no getenv in the library sources (diagnostics are per-ensemble calls, include/pdmp_debug.h)."""
    csrc = os.path.join(ROOT, "zigzagboomerang.jl_amd", "csrc")
    for f in os.listdir(csrc):
        assert "getenv" not in open(os.path.join(csrc, f), errors="replace").read(), f


def test_library_loads_and_exports_every_symbol(pkg):
    pkg.build.build()
    L = ctypes.CDLL(pkg._lib.lib_path())
    for name in declared_functions() + declared_functions("pdmp_debug.h"):
        assert hasattr(L, name), name
    assert pkg._lib.load().pdmp_abi_version() == pkg._lib.ABI_VERSION == 3


def test_struct_sizes(pkg):
    assert ctypes.sizeof(pkg._lib.PdmpConfig) == 48
    assert pkg._lib.EVENT_DTYPE.itemsize == 32 and pkg._lib.COUNTERS_DTYPE.itemsize == 72
    assert ctypes.sizeof(pkg._lib.Config1d) == 88 and pkg._lib.EVENT1D_DTYPE.itemsize == 24 and pkg._lib.STATE1D_DTYPE.itemsize == 96  # pdmp_1d_*


def test_no_cpu_fallback_without_device(pkg):
    """On a box without a GPU, creating an ensemble must fail loudly (PDMP_ERR_NO_DEVICE), never emulate."""
    if pkg._lib.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(pkg._lib.PdmpError) as ei:
        pkg.Ensemble(1, 4)
    assert ei.value.code == 2


def test_product_never_imports_the_oracle():
    pkg_dir = os.path.join(ROOT, "zigzagboomerang.jl_amd")
    for dp, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "oracle_lib" not in txt and "liboracle" not in txt, (dp, f)
                assert not re.search(r'#include\s*[<"][^>"]*oracle', txt), (dp, f)
                assert not re.search(r'^\s*(from|import)\s+\S*oracle', txt, flags=re.M), (dp, f)


def test_headers_are_plain_c99(tmp_path):
    """include/pdmp_mi355.h and include/pdmp_detmath.h must compile as C99 (the boundary is a C ABI: cgo / ccall / ctypes bind it),
    with the struct sizes the bindings assume."""
    import subprocess
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "pdmp_mi355.h"\n#include "pdmp_debug.h"\n#include "pdmp_detmath.h"\n'
                   "int main(void){ return (int)(sizeof(pdmp_event) != 32) + (int)(sizeof(pdmp_chain_counters) != 72) + "
                   "(int)(sizeof(pdmp_config) != 48) + (int)(pdmp_log(1.0) != 0.0); }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-ffp-contract=off", "-I", inc, str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


SHARED_SCALARS = ("pos_part", "sigmoid", "poisson_time", "poisson_time_L", "poisson_time_L_ref")


def test_shared_scalars_are_defined_once_and_probed_in_every_unit_that_calls_them():
    """poisson_time, sigmoid and pos exist ONCE on the device, in csrc/pdmp_device.hpp: no translation unit defines a copy of its own.  Every
    unit that calls one of them (outside its probe) has a pdmp_debug_math_eval id for that call (include/pdmp_debug.h names the unit and the
    function of each), and the unit's probe returns that call under that id: a new user without a probe, or a private copy, fails here
    (tests/test_gpu_detmath.py holds every probed call, as compiled inside its unit, to the oracle bit for bit)."""
    csrc = os.path.join(ROOT, "zigzagboomerang.jl_amd", "csrc")

    def scalar_definitions(f):
        names = re.findall(r"__device__[^;{(]*?\b(\w+)\s*\(\s*double\b", open(os.path.join(csrc, f)).read())
        return sorted(n for n in names if "poisson_time" in n or "sigmoid" in n or n.endswith("_pos") or n == "pos_part")

    units = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".inc")))
    assert [(f, scalar_definitions(f)) for f in sorted(os.listdir(csrc)) if f != "pdmp_device.hpp" and scalar_definitions(f)] == []
    assert scalar_definitions("pdmp_device.hpp") == sorted(SHARED_SCALARS)

    called = set()  # (unit, scalar): calls in the unit's code before its probe functor (an .inc file belongs to the unit that includes it)
    for f in units:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, f)).read(), flags=re.S)
        text = re.split(r"struct \w+MathEval\b", text)[0]
        owner = f if f.endswith(".hip") else next(u for u in units if '#include "%s"' % f in open(os.path.join(csrc, u)).read())
        called |= {(owner, name) for name in re.findall(r"(?<![\w.])(%s)\s*\(" % "|".join(SHARED_SCALARS), text)}
    src = open(os.path.join(ROOT, "include", "pdmp_debug.h")).read()
    ids = re.findall(r"#define (PDMP_MATH_\w+) \d+\s*/\* (pdmp_\w+\.hip) (\w+) \*/", src)
    probed = {(f, name) for _, f, name in ids}
    assert called <= probed, called - probed
    assert probed - called == {("pdmp_general.hip", "poisson_time")}  # (an id kept for a unit whose event loop takes the _L form only)
    assert len(ids) == len(probed) == 26  # 13 poisson_time (5 plain, 7 _L, 1 _L_ref), 3 sigmoid, 10 pos
    for macro, f, name in ids:  # the probe of the unit returns that call under that id
        probe = re.split(r"struct \w+MathEval\b", open(os.path.join(csrc, f)).read())[1]
        assert re.search(r"(case %s: return %s\(|default: return %s\([^;]*;\s*//\s*%s\b)" % (macro, name, name, macro), probe), (macro, f, name)


def test_scalar_probe_is_parity_library_only(pkg):
    """the default library exports pdmp_debug_math_eval (every pdmp_debug.h symbol) but has no probe kernels: it answers UNSUPPORTED"""
    pkg.build.build()
    a = (ctypes.c_double * 1)(0.5)
    out = (ctypes.c_double * 2)()
    st = pkg._lib.load().pdmp_debug_math_eval(0, 2, 1, a, a, a, out)
    assert st == pkg._lib.PDMP_ERR_UNSUPPORTED
    # ... and so do the probes one layer up: the wave primitives, the queues' first-level codes, the LDS-state helpers
    L = pkg._lib.load()
    assert L.pdmp_debug_queue_eval(0, 0, 1, a, a, a, out) == pkg._lib.PDMP_ERR_UNSUPPORTED
    w = (ctypes.c_uint64 * 64)()
    assert L.pdmp_debug_wave_eval(0, 0, 1, w, w, w) == pkg._lib.PDMP_ERR_UNSUPPORTED
    idx = (ctypes.c_uint32 * 1)(0)
    img = (ctypes.c_double * 8192)()
    assert L.pdmp_debug_state_eval(0, 0, 0, None, 0, 0, 1, idx, a, img) == pkg._lib.PDMP_ERR_UNSUPPORTED
    assert b"parity build" in L.pdmp_last_error()
