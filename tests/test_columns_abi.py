"""The boundary of the column maps (include/tsdf_hip_columns.h): one more feature header beside the
tsdf_hip.h contract, which stays as it is.  No compute calls here — CPU suite."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
COLUMNS_HEADER = os.path.join(REPO, "include", "tsdf_hip_columns.h")
COLUMNS_FUNCTIONS = ["tsdf_column_map", "tsdf_column_map_device"]
FLAGS = (("OBSERVED", 1), ("OCCUPIED", 2), ("FREE", 4), ("HAS_ELEV", 8), ("HAS_CEIL", 16))


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_columns_header_declares_the_columns_table():
    from tsdf_map import _abi
    fns = functions_of(COLUMNS_HEADER)
    assert fns == sorted(_abi.COLUMNS_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == COLUMNS_FUNCTIONS
    txt = open(COLUMNS_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_COLUMNS_API 1\b", txt)
    for name, value in FLAGS:
        assert re.search(r"#define TSDF_COLUMN_%s\s+%du\b" % (name, value), txt)
        assert getattr(_abi, "COLUMN_" + name) == value
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "never modifies the map" in flat
    assert "0x7FC00000" in flat and "index = (x - lo[0]) + nx (y - lo[1])" in flat


def test_columns_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_columns.h"\n'
                   "#if TSDF_COLUMNS_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "#if (TSDF_COLUMN_OBSERVED | TSDF_COLUMN_OCCUPIED | TSDF_COLUMN_FREE | \\\n"
                   "     TSDF_COLUMN_HAS_ELEV | TSDF_COLUMN_HAS_CEIL) != 31u\n"
                   "#error\n#endif\n"
                   "typedef int (*fn)(tsdf_ctx*, const int64_t*, const int64_t*, float, float,\n"
                   "                  uint32_t, uint32_t, float*, float*, uint16_t*, uint16_t*,\n"
                   "                  uint8_t*);\n"
                   "int main(void) {\n"
                   "    fn h = tsdf_column_map;\n"
                   "    fn d = tsdf_column_map_device;\n"
                   "    return h == 0 || d == 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_columns_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in COLUMNS_FUNCTIONS if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.COLUMNS_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES, _abi.ESDF_SIGNATURES, _abi.MERGE_SIGNATURES,
              _abi.MESH_SIGNATURES, _abi.DESKEW_SIGNATURES, _abi.COLUMNS_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_the_python_names_exist():
    import tsdf_map
    from tsdf_map import ColumnMap, HipTSDFVolume, TSDFVolume, columns_around, gridmap
    assert callable(TSDFVolume.column_map) and callable(HipTSDFVolume.column_map_device)
    assert gridmap.ColumnMap is ColumnMap and gridmap.columns_around is columns_around
    assert tsdf_map.ColumnMap is ColumnMap
    for name in ("occupancy_grid", "headroom", "step_height"):
        assert callable(getattr(ColumnMap, name))


def test_oracle_has_no_column_maps():
    import oracle
    from tsdf_map import columns_around
    lib = oracle.load()
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in COLUMNS_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in COLUMNS_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.column_map([0, 0, 0], [1, 1, 1])
    with pytest.raises(NotImplementedError):
        columns_around(v, [0.0, 0.0, 0.0], 0.5, -0.2, 0.4)
    # the Python layer's own rules come before any call reaches a library
    with pytest.raises(ValueError):
        v.column_map([0, 0, 0], [1, -1, 1])
    for kw in (dict(min_occ=0), dict(min_free=65536)):
        with pytest.raises(ValueError):
            v.column_map([0, 0, 0], [1, 1, 1], **kw)
    v.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    box = (ctypes.c_int64 * 3)(0, 0, 0)
    e = (ctypes.c_float * 1)(7.0)
    f = (ctypes.c_uint8 * 1)(9)
    assert lib.tsdf_column_map(None, box, box, 0.0, 0.0, 1, 1, e, None, None, None,
                               f) == _abi.TSDF_EINVAL
    assert lib.tsdf_column_map_device(None, box, box, 0.0, 0.0, 1, 1, None, None, None, None,
                                      None) == _abi.TSDF_EINVAL
    assert e[0] == 7.0 and f[0] == 9


def test_the_gridmap_helpers_on_a_hand_made_map():
    """occupancy_grid, headroom and step_height on a 2 x 3 map (no library involved)."""
    from tsdf_map import ColumnMap, _abi
    F = np.float32
    nan = F(np.nan)
    elev = np.array([[0.1, 0.3, nan], [0.2, nan, 1.0]], F)
    ceil = np.array([[2.0, nan, nan], [0.1, 2.0, 2.5]], F)
    flags = np.array([[27, 13, 0], [27, 21, 29]], np.uint8)  # OBS|OCC|E|C, OBS|FREE|E, 0, ..
    z = np.zeros((2, 3), np.uint16)
    m = ColumnMap(elev, ceil, z, z, flags, [-4, 6, 0], [-1, 8, 5], 0.1)
    data, origin, res = m.occupancy_grid()
    assert data.dtype == np.int8 and data.tolist() == [[100, 0, -1], [100, 0, 0]]
    assert origin.tolist() == [-4 * 0.1, 6 * 0.1] and res == 0.1
    assert m.occupancy_grid(unknown=7, free=1, occupied=2)[0].tolist() == [[2, 1, 7], [2, 1, 1]]
    h = m.headroom()
    assert h.dtype == F and h[0, 0] == F(2.0) - F(0.1) and h[1, 0] == F(0.1) - F(0.2)
    assert np.isnan(h[0, 1]) and np.isnan(h[0, 2]) and np.isnan(h[1, 1]) and h[1, 2] == F(1.5)
    s = m.step_height()
    assert s[0, 0] == F(0.3) - F(0.1)           # max(|0.3 - 0.1|, |0.2 - 0.1|)
    assert s[0, 1] == F(0.3) - F(0.1) and s[1, 0] == F(0.2) - F(0.1)
    assert np.isnan(s[0, 2]) and np.isnan(s[1, 1]) and np.isnan(s[1, 2])
    with pytest.raises(ValueError):
        ColumnMap(elev, ceil, z, z, flags, [0, 0, 0], [2, 3, 1], 0.1)
    assert _abi.COLUMN_FREE == 4
