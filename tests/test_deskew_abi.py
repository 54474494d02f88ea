"""The deskew boundary (include/tsdf_hip_deskew.h): one more feature header beside the tsdf_hip.h
contract, which stays as it is.  No compute calls here — CPU suite."""
import ctypes
import itertools
import os
import re
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
DESKEW_HEADER = os.path.join(REPO, "include", "tsdf_hip_deskew.h")
NAMES = ["tsdf_os_deskew_device", "tsdf_os_headers"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_deskew_header_declares_the_deskew_table():
    from tsdf_map import _abi
    fns = functions_of(DESKEW_HEADER)
    assert fns == sorted(_abi.DESKEW_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == NAMES
    txt = open(DESKEW_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_DESKEW_API 1\b", txt)


def test_deskew_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_deskew.h"\n'
                   "#if TSDF_DESKEW_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*f)(tsdf_ctx*, const tsdf_os_format*, const uint8_t*, uint32_t,\n"
                   "             const float*, const float*, const float*, float*, uint32_t*)\n"
                   "        = tsdf_os_deskew_device;\n"
                   "    int (*g)(const tsdf_os_format*, const uint8_t*, uint32_t, uint64_t*,\n"
                   "             uint32_t*, uint16_t*) = tsdf_os_headers;\n"
                   "    return f == 0 || g == 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_deskew_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.DESKEW_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.DESKEW_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_all_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = {n: t for n, t in vars(_abi).items() if n.endswith("SIGNATURES")}
    assert len(tables) >= 8 and "DESKEW_SIGNATURES" in tables
    for (a, ta), (b, tb) in itertools.combinations(tables.items(), 2):
        assert not set(ta) & set(tb), (a, b)
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_oracle_does_not_deskew():
    import oracle
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in NAMES)
    assert not any(hasattr(lib, f) for f in NAMES)


def test_bad_arguments_are_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    fmt = _abi.OsFormat(1, 8, 16, 64)
    ts, st, mid = (ctypes.c_uint64 * 64)(), (ctypes.c_uint32 * 64)(), (ctypes.c_uint16 * 64)()
    assert lib.tsdf_os_headers(ctypes.byref(fmt), None, 0, ts, st, mid) == _abi.TSDF_OK
    assert lib.tsdf_os_headers(ctypes.byref(fmt), None, 1, ts, st, mid) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_headers(None, None, 0, ts, st, mid) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_headers(ctypes.byref(fmt), None, 0, None, st, mid) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_headers(ctypes.byref(fmt), None, 0, ts, None, mid) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_headers(ctypes.byref(fmt), None, 0, ts, st, None) == _abi.TSDF_EINVAL
    bad = _abi.OsFormat(7, 8, 16, 64)
    assert lib.tsdf_os_headers(ctypes.byref(bad), None, 0, ts, st, mid) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_deskew_device(None, ctypes.byref(fmt), None, 0, None, None, None, None,
                                     None) == _abi.TSDF_EINVAL
