"""The boundary of the map merge (include/tsdf_hip_merge.h): a sixth header beside the tsdf_hip.h
contract and the sampling, raycast, prune and distance-field headers, all of which stay as they
are.  No compute calls here -- CPU suite."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

INC = os.path.join(REPO, "include")
HEADER = os.path.join(INC, "tsdf_hip.h")
MERGE_HEADER = os.path.join(INC, "tsdf_hip_merge.h")
OTHERS = {"SAMPLE": "tsdf_hip_sample.h", "RAYCAST": "tsdf_hip_raycast.h", "PRUNE": "tsdf_hip_prune.h",
          "ESDF": "tsdf_hip_esdf.h"}
MERGE_FUNCTIONS = ["tsdf_merge_count", "tsdf_merge_transformed"]
FIELDS = ["src_bricks", "candidate_bricks", "touched_bricks", "new_bricks", "merged_voxels",
          "overlap_voxels"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_merge_header_declares_the_merge_table():
    from tsdf_map import _abi
    fns = functions_of(MERGE_HEADER)
    assert fns == sorted(_abi.MERGE_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == MERGE_FUNCTIONS
    txt = open(MERGE_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r'#include "tsdf_hip_sample\.h"', txt)  # the modes are the sample's
    assert re.search(r"#define TSDF_MERGE_API 1\b", txt)
    assert not re.search(r"#define TSDF_SAMPLE_", txt)
    flat = " ".join(txt.split())
    assert "ARE the contract" in flat and "Resampling is not copying" in flat
    assert "src is never modified" in flat and "no floating-point atomics" in flat
    assert [f for f, _ in _abi.MergeStats._fields_] == FIELDS


def test_merge_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_merge.h"\n'
                   "#if TSDF_MERGE_API != 1 || TSDF_ABI_VERSION != 10 || TSDF_SAMPLE_API != 1\n"
                   "#error\n#endif\n"
                   "#if TSDF_SAMPLE_NEAREST != 0 || TSDF_SAMPLE_TRILINEAR != 1\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*c)(tsdf_ctx*, tsdf_ctx*, const double*, int32_t, float,\n"
                   "             tsdf_merge_stats*) = tsdf_merge_count;\n"
                   "    int (*t)(tsdf_ctx*, tsdf_ctx*, const double*, int32_t, float,\n"
                   "             tsdf_merge_stats*) = tsdf_merge_transformed;\n"
                   "    tsdf_merge_stats s = {0, 0, 0, 0, 0, 0};\n"
                   "    return c == 0 || t == 0 || s.overlap_voxels != 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(src),
                           "-o", str(obj)])


def test_struct_layout_matches_the_header(tmp_path):
    from tsdf_map import _abi
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tsdf_hip_merge.h"',
             "int main(void) {", 'printf("sizeof %zu\\n", sizeof(tsdf_merge_stats));']
    for f in FIELDS:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(tsdf_merge_stats, %s), '
                     "sizeof(((tsdf_merge_stats*)0)->%s));" % (f, f, f))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", INC, str(src), "-o", str(exe)])
    got = dict((ln.split()[0], [int(v) for v in ln.split()[1:]])
               for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["sizeof"] == [ctypes.sizeof(_abi.MergeStats)] == [48]
    for f in FIELDS:
        fld = getattr(_abi.MergeStats, f)
        assert got[f] == [fld.offset, fld.size], f
    s = _abi.MergeStats(1, 2, 3, 4, 5, 6)
    assert s.as_dict() == dict(zip(FIELDS, range(1, 7)))


def test_hip_library_exports_the_merge_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.MERGE_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.MERGE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_six_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES, _abi.ESDF_SIGNATURES, _abi.MERGE_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    for key, name in OTHERS.items():
        assert functions_of(os.path.join(INC, name)) == sorted(getattr(_abi, key + "_SIGNATURES"))
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())
    assert "merge_transformed" not in open(HEADER).read()


def test_oracle_cannot_merge_maps():
    import oracle
    from tsdf_map import fuse_submaps
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in MERGE_FUNCTIONS)
    assert not any(hasattr(lib, f) for f in MERGE_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    a = oracle.OracleTSDFVolume(0.1, 0.3)
    b = oracle.OracleTSDFVolume(0.1, 0.3)
    eye = np.eye(4)
    with pytest.raises(NotImplementedError):
        a.merge_from(b, eye)
    with pytest.raises(NotImplementedError):
        a.merge_from(b, eye[:3], mode="nearest", dry_run=True)
    with pytest.raises(NotImplementedError):
        fuse_submaps([b], [eye], into=a)
    assert not hasattr(a, "transformed")  # HipTSDFVolume's
    with pytest.raises(ValueError):
        a.merge_from(b, eye, mode="cubic")
    a.close()
    b.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    pose = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    st = _abi.MergeStats(7, 7, 7, 7, 7, 7)
    for fn in (lib.tsdf_merge_count, lib.tsdf_merge_transformed):
        assert fn(None, None, pose, 1, 0.0, ctypes.byref(st)) == _abi.TSDF_EINVAL
        assert fn(None, None, None, 5, -1.0, None) == _abi.TSDF_EINVAL
    assert st.as_dict() == dict(zip(FIELDS, [7] * 6))
