"""The boundary of prune and evict (include/tsdf_hip_prune.h): a fourth header beside the
tsdf_hip.h contract, the sampling header and the raycast header, all of which stay as they are.
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
PRUNE_FUNCTIONS = ["tsdf_count_outside", "tsdf_evict_outside", "tsdf_prune"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_prune_header_declares_the_prune_table():
    from tsdf_map import _abi
    fns = functions_of(PRUNE_HEADER)
    assert fns == sorted(_abi.PRUNE_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == PRUNE_FUNCTIONS
    txt = open(PRUNE_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_PRUNE_API 1\b", txt)
    # VDBFusion is not among the restated sources: the header says that its rule is the contract,
    # and that capacity is not shrunk
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "Capacity is not shrunk" in flat


def test_prune_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_prune.h"\n'
                   "#if TSDF_PRUNE_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*p)(tsdf_ctx*, float, uint64_t*) = tsdf_prune;\n"
                   "    int (*n)(tsdf_ctx*, const int32_t*, const int32_t*, uint64_t*)\n"
                   "        = tsdf_count_outside;\n"
                   "    int (*e)(tsdf_ctx*, const int32_t*, const int32_t*, int32_t*, float*,\n"
                   "             float*, uint64_t, uint64_t*) = tsdf_evict_outside;\n"
                   "    return p == 0 || n == 0 || e == 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)])


def test_hip_library_exports_the_prune_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.PRUNE_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.PRUNE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_four_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert functions_of(SAMPLE_HEADER) == sorted(_abi.SAMPLE_SIGNATURES)
    assert functions_of(RAYCAST_HEADER) == sorted(_abi.RAYCAST_SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_oracle_does_not_prune():
    import oracle
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in PRUNE_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in PRUNE_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.prune(1.0)
    with pytest.raises(NotImplementedError):
        v.evict_outside([0, 0, 0], [1, 1, 1])
    with pytest.raises(NotImplementedError):
        v.count_outside([0, 0, 0], [1, 1, 1])
    from tsdf_map import SlidingWindow
    with pytest.raises(NotImplementedError):
        SlidingWindow(v, 5.0)


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    n = ctypes.c_uint64(7)
    box = (ctypes.c_int32 * 3)(0, 0, 0)
    assert lib.tsdf_prune(None, 1.0, ctypes.byref(n)) == _abi.TSDF_EINVAL
    assert lib.tsdf_count_outside(None, box, box, ctypes.byref(n)) == _abi.TSDF_EINVAL
    assert lib.tsdf_evict_outside(None, box, box, None, None, None, 0,
                                  ctypes.byref(n)) == _abi.TSDF_EINVAL
    assert n.value == 7


def test_archives_keep_generations(tmp_path):
    """The two archives of tsdf_map.window hold one entry per append, duplicates included."""
    import numpy as np
    from tsdf_map import MemoryArchive, NpzArchive
    c = np.array([[0, 0, 0], [1, -2, 3]], np.int32)
    s = np.arange(2 * 512, dtype=np.float32).reshape(2, 8, 8, 8)
    w = s + 1
    for arch in (MemoryArchive(), NpzArchive(tmp_path / "a")):
        arch.append(c, s, w)
        arch.append(c[:0], s[:0], w[:0])  # an eviction that removed nothing leaves no part
        arch.append(c[1:], 2 * s[1:], w[1:])
        parts = list(arch)
        assert len(arch) == len(parts) == 2 and arch.num_bricks() == 3
        assert np.array_equal(parts[0][0], c) and np.array_equal(parts[1][1], 2 * s[1:])
        assert np.array_equal(parts[1][0], c[1:]) and np.array_equal(parts[0][2], w)
    again = NpzArchive(tmp_path / "a")  # reopened: the parts are still there, numbering goes on
    again.append(c[:1], s[:1], w[:1])
    assert len(again) == 3 and again.num_bricks() == 4
