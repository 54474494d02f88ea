"""The boundary of the 2:1 coarsening (include/tsdf_hip_coarsen.h): a further feature header beside
the tsdf_hip.h contract, which stays as it is.  No compute calls here -- CPU suite."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

INC = os.path.join(REPO, "include")
HEADER = os.path.join(INC, "tsdf_hip.h")
COARSEN_HEADER = os.path.join(INC, "tsdf_hip_coarsen.h")
COARSEN_FUNCTIONS = ["tsdf_coarsen_count", "tsdf_coarsen_into"]
FIELDS = ["src_bricks", "parent_bricks", "touched_bricks", "new_bricks", "coarse_voxels",
          "overlap_voxels", "child_voxels"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_coarsen_header_declares_the_coarsen_table():
    from tsdf_map import _abi
    fns = functions_of(COARSEN_HEADER)
    assert fns == sorted(_abi.COARSEN_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == COARSEN_FUNCTIONS
    txt = open(COARSEN_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_COARSEN_API 1\b", txt)
    assert re.search(r"#define TSDF_COARSEN_INSIDE 0\b", txt)
    assert re.search(r"#define TSDF_COARSEN_OUTSIDE 1\b", txt)
    assert _abi.COARSEN_SIDES == {"inside": 0, "outside": 1}
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "Partition." in flat and "Determinism." in flat
    assert "src is never modified" in flat and "no floating-point atomics" in flat
    assert "k = a + 2 b + 4 c" in flat and "w = sw / (float)n" in flat
    assert [f for f, _ in _abi.CoarsenStats._fields_] == FIELDS


def test_coarsen_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_coarsen.h"\n'
                   "#if TSDF_COARSEN_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "#if TSDF_COARSEN_INSIDE != 0 || TSDF_COARSEN_OUTSIDE != 1\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*c)(tsdf_ctx*, tsdf_ctx*, const int32_t*, const int32_t*, int32_t,\n"
                   "             uint32_t, float, tsdf_coarsen_stats*) = tsdf_coarsen_count;\n"
                   "    int (*t)(tsdf_ctx*, tsdf_ctx*, const int32_t*, const int32_t*, int32_t,\n"
                   "             uint32_t, float, tsdf_coarsen_stats*) = tsdf_coarsen_into;\n"
                   "    tsdf_coarsen_stats s = {0, 0, 0, 0, 0, 0, 0};\n"
                   "    return c == 0 || t == 0 || s.child_voxels != 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(src),
                           "-o", str(obj)])


def test_struct_layout_matches_the_header(tmp_path):
    from tsdf_map import _abi
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tsdf_hip_coarsen.h"',
             "int main(void) {", 'printf("sizeof %zu\\n", sizeof(tsdf_coarsen_stats));']
    for f in FIELDS:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(tsdf_coarsen_stats, %s), '
                     "sizeof(((tsdf_coarsen_stats*)0)->%s));" % (f, f, f))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", INC, str(src), "-o", str(exe)])
    got = dict((ln.split()[0], [int(v) for v in ln.split()[1:]])
               for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["sizeof"] == [ctypes.sizeof(_abi.CoarsenStats)] == [56]
    for f in FIELDS:
        fld = getattr(_abi.CoarsenStats, f)
        assert got[f] == [fld.offset, fld.size], f
    s = _abi.CoarsenStats(1, 2, 3, 4, 5, 6, 7)
    assert s.as_dict() == dict(zip(FIELDS, range(1, 8)))


def test_hip_library_exports_the_coarsen_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.COARSEN_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.COARSEN_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = [getattr(_abi, n) for n in dir(_abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 9 and _abi.COARSEN_SIGNATURES in tables
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert functions_of(os.path.join(INC, "tsdf_hip_merge.h")) == sorted(_abi.MERGE_SIGNATURES)
    assert functions_of(os.path.join(INC, "tsdf_hip_prune.h")) == sorted(_abi.PRUNE_SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())
    assert "coarsen" not in open(HEADER).read()


def test_oracle_cannot_coarsen_maps():
    import oracle
    from tsdf_map import lod_pyramid
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in COARSEN_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in COARSEN_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    a = oracle.OracleTSDFVolume(0.2, 0.3)
    b = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        a.coarsen_from(b)
    with pytest.raises(NotImplementedError):
        a.coarsen_from(b, min_children=8, min_weight=1.0, box=((0, 0, 0), (1, 1, 1)),
                       side="outside", dry_run=True)
    with pytest.raises(NotImplementedError):
        lod_pyramid(b, 2)
    assert not hasattr(a, "coarsened")  # HipTSDFVolume's
    with pytest.raises(ValueError):
        a.coarsen_from(b, side="around")
    a.close()
    b.close()


def test_a_sliding_window_checks_its_coarse_volume():
    import oracle
    from tsdf_map import SlidingWindow
    a = oracle.OracleTSDFVolume(0.1, 0.3)
    # (the oracle cannot evict either: the window says so before it looks at `coarse`)
    with pytest.raises(NotImplementedError):
        SlidingWindow(a, 5.0, coarse=a)
    a.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    st = _abi.CoarsenStats(7, 7, 7, 7, 7, 7, 7)
    box = (ctypes.c_int32 * 3)(0, 0, 0)
    for fn in (lib.tsdf_coarsen_count, lib.tsdf_coarsen_into):
        assert fn(None, None, None, None, 0, 1, 0.0, ctypes.byref(st)) == _abi.TSDF_EINVAL
        assert fn(None, None, box, None, 5, 0, -1.0, None) == _abi.TSDF_EINVAL
    assert st.as_dict() == dict(zip(FIELDS, [7] * 7))
    assert np.dtype(np.uint64).itemsize * 7 == ctypes.sizeof(_abi.CoarsenStats)
