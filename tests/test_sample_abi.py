"""The sparse map queries' boundary (include/tsdf_hip_sample.h): a header of their own beside the
tsdf_hip.h contract, which stays as it is — same function set, same ABI version, and the oracle
still exports its subset of it.  No compute calls here — CPU suite."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, "include", "tsdf_hip.h")
SAMPLE_HEADER = os.path.join(REPO, "include", "tsdf_hip_sample.h")


def functions_of(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z_]+)\s*\(", txt)))


def dynamic_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_sample_header_declares_the_sample_table():
    from tsdf_map import _abi
    fns = functions_of(SAMPLE_HEADER)
    assert fns == sorted(_abi.SAMPLE_SIGNATURES), "ctypes table out of sync with the header"
    assert fns == ["tsdf_align_terms_device", "tsdf_sample", "tsdf_sample_device"]
    txt = open(SAMPLE_HEADER).read()
    assert re.search(r'#include "tsdf_hip\.h"', txt)
    assert re.search(r"#define TSDF_SAMPLE_API 1\b", txt)
    consts = dict(re.findall(r"#define (TSDF_(?:SAMPLE_NEAREST|SAMPLE_TRILINEAR|ALIGN_WORDS)) (\d+)",
                             txt))
    assert int(consts["TSDF_SAMPLE_NEAREST"]) == _abi.SAMPLE_NEAREST == 0
    assert int(consts["TSDF_SAMPLE_TRILINEAR"]) == _abi.SAMPLE_TRILINEAR == 1
    assert int(consts["TSDF_ALIGN_WORDS"]) == _abi.ALIGN_WORDS == 44


def test_sample_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "tsdf_hip_sample.h"\n'
                   "#if TSDF_SAMPLE_API != 1 || TSDF_ABI_VERSION != 10\n#error\n#endif\n"
                   "int main(void) { double out[TSDF_ALIGN_WORDS]; return sizeof out != 352; }\n")
    exe = tmp_path / "use"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
                           "-o", str(exe)])
    subprocess.check_call([str(exe)])


def test_hip_library_exports_the_sample_symbols():
    from tsdf_map import HIP_LIB, _abi, load_hip_library
    assert os.path.exists(HIP_LIB), "run __graft_entry__.build() first"
    syms = dynamic_symbols(HIP_LIB)
    missing = [f for f in _abi.SAMPLE_SIGNATURES if f not in syms]
    assert not missing, missing
    lib = load_hip_library()
    for name, (res, args) in _abi.SAMPLE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.tsdf_abi_version() == 10


def test_the_contract_is_untouched():
    from tsdf_map import _abi
    assert set(functions_of(HEADER)) == set(_abi.SIGNATURES)
    assert not set(_abi.SAMPLE_SIGNATURES) & set(_abi.SIGNATURES)
    assert _abi.ABI_VERSION == 10
    assert re.search(r"#define TSDF_ABI_VERSION 10\b", open(HEADER).read())


def test_oracle_still_loads_and_does_not_sample():
    import pytest

    import oracle
    lib = oracle.load()
    assert lib.tsdf_abi_version() == 10
    syms = dynamic_symbols(oracle.LIB_PATH)
    for f in functions_of(HEADER):
        if f not in oracle.HOST_ONLY:
            assert f in syms, f
    # the feature is detected by the symbol: a library without it refuses to sample, loudly
    assert not any(hasattr(lib, f) for f in ("tsdf_sample", "tsdf_sample_device"))
    v = oracle.OracleTSDFVolume(0.1, 0.3)
    with pytest.raises(NotImplementedError):
        v.sample([[0.0, 0.0, 0.0]])


def test_null_context_is_refused():
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    out = (ctypes.c_double * 44)()
    pose = (ctypes.c_double * 12)()
    assert lib.tsdf_sample_device(None, None, 0, 1, 0.0, None, None, None, None) == _abi.TSDF_EINVAL
    assert lib.tsdf_sample(None, None, 0, 12, 0, 0, 1, 0.0, None, None, None,
                           None) == _abi.TSDF_EINVAL
    assert lib.tsdf_align_terms_device(None, None, 0, pose, 0.0, out) == _abi.TSDF_EINVAL
