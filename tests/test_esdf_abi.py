"""The boundary of the distance field (include/tsdf_hip_esdf.h): a fifth header beside the
tsdf_hip.h contract and the sampling, raycast and prune headers, all of which stay as they are.
No compute calls here — CPU suite."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
SAMPLE_HEADER = os.path.join(REPO, "include", "tsdf_hip_sample.h")
RAYCAST_HEADER = os.path.join(REPO, "include", "tsdf_hip_raycast.h")
PRUNE_HEADER = os.path.join(REPO, "include", "tsdf_hip_prune.h")
ESDF_HEADER = os.path.join(REPO, "include", "tsdf_hip_esdf.h")
ESDF_FUNCTIONS = ["tsdf_esdf_dense", "tsdf_esdf_dense_device"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_esdf_header_declares_the_esdf_table():
    from tsdf_map import _abi
    fns = functions_of(ESDF_HEADER)
    assert fns == sorted(_abi.ESDF_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == ESDF_FUNCTIONS
    txt = open(ESDF_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_ESDF_API 1\b", txt)
    for name, value in (("OBSERVED", 1), ("SITE", 2), ("CAPPED", 4), ("MAX_RADIUS", 128)):
        assert re.search(r"#define TSDF_ESDF_%s\s+%du\b" % (name, value), txt)
        assert getattr(_abi, "ESDF_" + name) == value
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "The box is the world" in flat
    assert "never modifies the map" in flat


def test_esdf_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_esdf.h"\n'
                   "#if TSDF_ESDF_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "#if (TSDF_ESDF_OBSERVED | TSDF_ESDF_SITE | TSDF_ESDF_CAPPED) != 7u\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*h)(tsdf_ctx*, const int64_t*, const int64_t*, uint32_t, float, float,\n"
                   "             float*, uint8_t*) = tsdf_esdf_dense;\n"
                   "    int (*d)(tsdf_ctx*, const int64_t*, const int64_t*, uint32_t, float, float,\n"
                   "             float*, uint8_t*) = tsdf_esdf_dense_device;\n"
                   "    return h == 0 || d == 0 || TSDF_ESDF_MAX_RADIUS != 128u;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_esdf_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.ESDF_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.ESDF_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_five_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES, _abi.ESDF_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert functions_of(SAMPLE_HEADER) == sorted(_abi.SAMPLE_SIGNATURES)
    assert functions_of(RAYCAST_HEADER) == sorted(_abi.RAYCAST_SIGNATURES)
    assert functions_of(PRUNE_HEADER) == sorted(_abi.PRUNE_SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_oracle_has_no_distance_field():
    import oracle
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in ESDF_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in ESDF_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.esdf([0, 0, 0], [1, 1, 1], 1.0)
    from tsdf_map import esdf_around
    with pytest.raises(NotImplementedError):
        esdf_around(v, [0.0, 0.0, 0.0], 0.5, 1.0)
    v.close()


def test_the_radius_rule_of_the_python_layer():
    """radius_vox = ceil(max_dist / voxel_size) in double, refused outside 1..128 before any call
    reaches a library."""
    import oracle
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    assert v.esdf_radius(0.1) == 1 and v.esdf_radius(0.11) == 2 and v.esdf_radius(1e-9) == 1
    assert v.esdf_radius(12.8) == 128 and v.esdf_radius(4.0) == 40
    for bad in (0.0, -1.0, 12.81, 1e9, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            v.esdf_radius(bad)
        with pytest.raises(ValueError):
            v.esdf([0, 0, 0], [1, 1, 1], bad)
    with pytest.raises(ValueError):
        v.esdf([0, 0, 0], [1, -1, 1], 1.0)
    v.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    box = (ctypes.c_int64 * 3)(0, 0, 0)
    d = (ctypes.c_float * 1)(7.0)
    f = (ctypes.c_uint8 * 1)(9)
    assert lib.tsdf_esdf_dense(None, box, box, 1, 0.1, 0.0, d, f) == _abi.TSDF_EINVAL
    assert lib.tsdf_esdf_dense_device(None, box, box, 1, 0.1, 0.0, None, None) == _abi.TSDF_EINVAL
    assert d[0] == 7.0 and f[0] == 9
