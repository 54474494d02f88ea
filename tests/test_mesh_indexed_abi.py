"""The boundary of the indexed mesh (include/tsdf_hip_mesh.h): a seventh header beside the
tsdf_hip.h contract and the sampling, raycast, prune, distance-field and merge headers, all of which
stay as they are.  No compute calls here -- CPU suite."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

INC = os.path.join(REPO, "include")
HEADER = os.path.join(INC, "tsdf_hip.h")
MESH_HEADER = os.path.join(INC, "tsdf_hip_mesh.h")
OTHERS = {"SAMPLE": "tsdf_hip_sample.h", "RAYCAST": "tsdf_hip_raycast.h", "PRUNE": "tsdf_hip_prune.h",
          "ESDF": "tsdf_hip_esdf.h", "MERGE": "tsdf_hip_merge.h"}
MESH_FUNCTIONS = ["tsdf_mesh_indexed", "tsdf_mesh_indexed_count", "tsdf_mesh_indexed_device"]
FIELDS = ["n_bricks", "n_vertices", "n_triangles"]


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_mesh_header_declares_the_mesh_table():
    from tsdf_map import _abi
    fns = functions_of(MESH_HEADER)
    assert fns == sorted(_abi.MESH_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == MESH_FUNCTIONS
    txt = open(MESH_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_MESH_API 1\b", txt)
    assert not re.search(r"#define TSDF_MC_", txt)  # the tables are tsdf_hip.h's
    flat = " ".join(txt.replace("\n *", "\n").split())  # the comment's text, line breaks gone
    for rule in ("ARE the contract", "bit for bit", "no unreferenced vertices",
                 "two vertices even where their positions coincide", "no floating-point atomics",
                 "2^32 vertices or more", "TSDF_EOVERFLOW and write nothing",
                 "The map is never modified", "exactly one of lo / hi NULL",
                 "an extent of 2^31 voxels or more", "n_sectors > 1", "open border reduce",
                 "tsdf_extract_mesh_local", "out of scope", "launches nothing",
                 "the box restricts cubes only", "224 bytes per listed brick"):
        assert rule in flat, rule
    assert [f for f, _ in _abi.MeshCounts._fields_] == FIELDS


def test_mesh_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_mesh.h"\n'
                   "#if TSDF_MESH_API != 1 || TSDF_ABI_VERSION != 10\n"
                   "#error\n#endif\n"
                   "int main(void) {\n"
                   "    int (*c)(tsdf_ctx*, float, int32_t, const int64_t*, const int64_t*,\n"
                   "             tsdf_mesh_counts*) = tsdf_mesh_indexed_count;\n"
                   "    int (*h)(tsdf_ctx*, float, int32_t, const int64_t*, const int64_t*, float*,\n"
                   "             float*, uint32_t*, uint64_t, uint64_t, tsdf_mesh_counts*)\n"
                   "        = tsdf_mesh_indexed;\n"
                   "    int (*d)(tsdf_ctx*, float, int32_t, const int64_t*, const int64_t*, float*,\n"
                   "             float*, uint32_t*, uint64_t, uint64_t, tsdf_mesh_counts*)\n"
                   "        = tsdf_mesh_indexed_device;\n"
                   "    tsdf_mesh_counts s = {0, 0, 0};\n"
                   "    return c == 0 || h == 0 || d == 0 || s.n_triangles != 0;\n}\n")
    obj = tmp_path / "use.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(src),
                           "-o", str(obj)])


def test_struct_layout_matches_the_header(tmp_path):
    from tsdf_map import _abi
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tsdf_hip_mesh.h"',
             "int main(void) {", 'printf("sizeof %zu\\n", sizeof(tsdf_mesh_counts));']
    for f in FIELDS:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(tsdf_mesh_counts, %s), '
                     "sizeof(((tsdf_mesh_counts*)0)->%s));" % (f, f, f))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", INC, str(src), "-o", str(exe)])
    got = dict((ln.split()[0], [int(v) for v in ln.split()[1:]])
               for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["sizeof"] == [ctypes.sizeof(_abi.MeshCounts)] == [24]
    for f in FIELDS:
        fld = getattr(_abi.MeshCounts, f)
        assert got[f] == [fld.offset, fld.size], f
    assert _abi.MeshCounts(1, 2, 3).as_dict() == dict(zip(FIELDS, range(1, 4)))


def test_hip_library_exports_the_mesh_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.MESH_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.MESH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_seven_tables_are_disjoint_and_the_contract_is_untouched():
    from tsdf_map import _abi
    tables = (_abi.SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.RAYCAST_SIGNATURES,
              _abi.PRUNE_SIGNATURES, _abi.ESDF_SIGNATURES, _abi.MERGE_SIGNATURES,
              _abi.MESH_SIGNATURES)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    for key, name in OTHERS.items():
        assert functions_of(os.path.join(INC, name)) == sorted(getattr(_abi, key + "_SIGNATURES"))
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())
    assert "mesh_indexed" not in open(HEADER).read()


def test_oracle_has_no_indexed_mesh():
    import oracle
    import pytest
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    assert not any(f in syms for f in MESH_FUNCTIONS)
    # the feature is detected by the symbol: a library without it refuses, loudly
    a = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        a.extract_indexed_mesh()
    with pytest.raises(NotImplementedError):
        a.indexed_mesh_counts()
    assert not hasattr(a, "indexed_mesh_device")  # HipTSDFVolume's
    assert "extract_indexed_mesh" in type(a).extract_triangle_mesh.__doc__
    a.close()


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    st = _abi.MeshCounts(7, 7, 7)
    assert lib.tsdf_mesh_indexed_count(None, 0.0, 0, None, None, ctypes.byref(st)) == _abi.TSDF_EINVAL
    for fn in (lib.tsdf_mesh_indexed, lib.tsdf_mesh_indexed_device):
        assert fn(None, 0.0, 0, None, None, None, None, None, 0, 0,
                  ctypes.byref(st)) == _abi.TSDF_EINVAL
        assert fn(None, -1.0, 9, None, None, None, None, None, 0, 0, None) == _abi.TSDF_EINVAL
    assert st.as_dict() == dict(zip(FIELDS, [7] * 3))
