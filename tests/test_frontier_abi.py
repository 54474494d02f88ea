"""The boundary of the frontier voxels (include/tsdf_hip_frontier.h): one more feature header beside
the tsdf_hip.h contract, which stays as it is.  No compute calls here — CPU suite."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
FRONTIER_HEADER = os.path.join(REPO, "include", "tsdf_hip_frontier.h")
FRONTIER_FUNCTIONS = ["tsdf_frontier_count", "tsdf_frontier_voxels", "tsdf_frontier_voxels_device"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_frontier_header_declares_the_frontier_table():
    from tsdf_map import _abi
    fns = functions_of(FRONTIER_HEADER)
    assert fns == sorted(_abi.FRONTIER_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == FRONTIER_FUNCTIONS
    txt = open(FRONTIER_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_FRONTIER_API 1\b", txt)
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "The map is never modified" in flat
    assert "l = z*64 + y*8 + x" in flat and "space carving" in flat
    for rule in ("obs = W > 0 && W >= min_weight", "free = obs && S >= free_band",
                 "unknown = !obs"):
        assert rule in flat
    fields = re.search(r"typedef struct tsdf_frontier_counts \{(.*?)\}", txt, re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", fields) == [k for k, _ in _abi.FrontierCounts._fields_]
    assert ctypes.sizeof(_abi.FrontierCounts) == 32


def test_frontier_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_frontier.h"\n'
                   "#if TSDF_FRONTIER_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "typedef int (*cfn)(tsdf_ctx*, const int64_t*, const int64_t*, float, float,\n"
                   "                   int32_t, int32_t, tsdf_frontier_counts*);\n"
                   "typedef int (*vfn)(tsdf_ctx*, const int64_t*, const int64_t*, float, float,\n"
                   "                   int32_t, int32_t, int32_t*, uint8_t*, int8_t*, uint64_t,\n"
                   "                   tsdf_frontier_counts*);\n"
                   "int main(void) {\n"
                   "    cfn c = tsdf_frontier_count;\n"
                   "    vfn h = tsdf_frontier_voxels;\n"
                   "    vfn d = tsdf_frontier_voxels_device;\n"
                   "    tsdf_frontier_counts n = {0, 0, 0, 0};\n"
                   "    return c == 0 || h == 0 || d == 0 || n.n_free != 0 ||\n"
                   "           sizeof n != 32;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_frontier_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in FRONTIER_FUNCTIONS if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.FRONTIER_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES, _abi.ESDF_SIGNATURES, _abi.MERGE_SIGNATURES,
              _abi.MESH_SIGNATURES, _abi.DESKEW_SIGNATURES, _abi.COLUMNS_SIGNATURES,
              _abi.COARSEN_SIGNATURES, _abi.FRONTIER_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_the_python_names_exist():
    import tsdf_map
    from tsdf_map import FrontierSet, HipTSDFVolume, TSDFVolume, frontier, frontiers_around
    assert callable(TSDFVolume.frontiers) and callable(TSDFVolume.frontier_counts)
    assert callable(HipTSDFVolume.frontiers_device)
    assert frontier.FrontierSet is FrontierSet and frontier.frontiers_around is frontiers_around
    assert tsdf_map.FrontierSet is FrontierSet
    for name in ("brick_runs", "clusters"):
        assert callable(getattr(FrontierSet, name))
    for name in ("points", "directions"):
        assert isinstance(getattr(FrontierSet, name), property)


def test_oracle_has_no_frontiers():
    import oracle
    from tsdf_map import frontiers_around
    lib = oracle.load()
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in FRONTIER_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in FRONTIER_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.frontiers()
    with pytest.raises(NotImplementedError):
        v.frontier_counts([0, 0, 0], [1, 1, 1])
    with pytest.raises(NotImplementedError):
        frontiers_around(v, [0.0, 0.0, 0.0], 0.5)
    v.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    box = (ctypes.c_int64 * 3)(0, 0, 0)
    c = np.full(3, 7, np.int32)
    st = _abi.FrontierCounts(9, 9, 9, 9)
    assert lib.tsdf_frontier_count(None, box, box, 0.0, 0.0, 6, 1,
                                   ctypes.byref(st)) == _abi.TSDF_EINVAL
    assert lib.tsdf_frontier_voxels(None, None, None, 0.0, 0.0, 6, 1, c.ctypes.data_as(_abi.I3),
                                    None, None, 1, ctypes.byref(st)) == _abi.TSDF_EINVAL
    assert lib.tsdf_frontier_voxels_device(None, None, None, 0.0, 0.0, 6, 1, None, None, None, 0,
                                           None) == _abi.TSDF_EINVAL
    assert c.tolist() == [7, 7, 7] and st.n_voxels == 9
