"""The raycast's boundary (include/tsdf_hip_raycast.h): a third header beside the tsdf_hip.h
contract and the sampling header, both of which stay as they are.  No compute calls here — CPU
suite."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
SAMPLE_HEADER = os.path.join(REPO, "include", "tsdf_hip_sample.h")
RAYCAST_HEADER = os.path.join(REPO, "include", "tsdf_hip_raycast.h")


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_raycast_header_declares_the_raycast_table():
    from tsdf_map import _abi
    fns = functions_of(RAYCAST_HEADER)
    assert fns == sorted(_abi.RAYCAST_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == ["tsdf_raycast", "tsdf_raycast_device"]
    txt = open(RAYCAST_HEADER).read()
    assert re.search(r'#include "tsdf_hip_sample\.h"', txt)
    assert re.search(r"#define TSDF_RAYCAST_API 1\b", txt)


def test_raycast_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_raycast.h"\n'
                   "#if TSDF_RAYCAST_API != 1 || TSDF_SAMPLE_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*f)(tsdf_ctx*, const float*, const float*, uint64_t, const double*,\n"
                   "             float, float, float, int32_t, float, float*, float*, uint8_t*)\n"
                   "        = tsdf_raycast_device;\n"
                   "    return f == 0 || TSDF_SAMPLE_NEAREST != 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_raycast_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.RAYCAST_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.RAYCAST_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_three_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert functions_of(SAMPLE_HEADER) == sorted(_abi.SAMPLE_SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_oracle_does_not_raycast():
    import oracle
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in ("tsdf_raycast", "tsdf_raycast_device"))
    assert not any(hasattr(lib, f) for f in ("tsdf_raycast", "tsdf_raycast_device"))
    # the feature is detected by the symbol: a library without it refuses, loudly
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.raycast([0.0, 0.0, 0.0], [[1.0, 0.0, 0.0]])


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    pose = (ctypes.c_double * 12)()
    assert lib.tsdf_raycast_device(None, None, None, 0, pose, 0.0, 1.0, 0.05, 0, 0.0, None, None,
                                   None) == _abi.TSDF_EINVAL
    assert lib.tsdf_raycast(None, None, None, 0, None, 0.0, 1.0, 0.05, 0, 0.0, None, None,
                            None) == _abi.TSDF_EINVAL
