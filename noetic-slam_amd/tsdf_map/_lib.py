"""Loader for the in-tree HIP library (noetic-slam_amd/lib/libtsdf_hip.so)."""
import ctypes
import os

from . import _abi

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_ROOT, "lib")
HIP_LIB = os.path.join(LIB_DIR, "libtsdf_hip.so")

ABI_VERSION = 10  # TSDF_ABI_VERSION of include/tsdf_hip.h

_hip = None


def load_hip_library(path=None):
    """Load and declare libtsdf_hip.so; raises (never falls back) when it is missing."""
    global _hip
    if _hip is not None and path is None:
        return _hip
    # TSDF_HIP_LIB: load another build of the same ABI (A/B kernel experiments, profiles/)
    p = path or os.environ.get("TSDF_HIP_LIB") or HIP_LIB
    if not os.path.exists(p):
        raise RuntimeError("libtsdf_hip.so not built (%s); run `python -c 'import __graft_entry__ "
                           "as g; g.build()'` or `make -C noetic-slam_amd/csrc`" % p)
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7, but
    # needed as "libamdhip64.so"), so it is loaded first and the library's libamdhip64.so.7 then
    # resolves to that copy.  Loaded the other way round, the process holds two runtimes and
    # torch finds no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = _abi.declare(ctypes.CDLL(p))
    # the sparse map queries (include/tsdf_hip_sample.h): part of this library, not of the ABI
    _abi.declare(lib, table=_abi.SAMPLE_SIGNATURES)
    # ... and the raycast (include/tsdf_hip_raycast.h)
    _abi.declare(lib, table=_abi.RAYCAST_SIGNATURES)
    # ... and removing bricks (include/tsdf_hip_prune.h)
    _abi.declare(lib, table=_abi.PRUNE_SIGNATURES)
    # ... and the distance field of a box (include/tsdf_hip_esdf.h)
    _abi.declare(lib, table=_abi.ESDF_SIGNATURES)
    # ... and the column maps of a box (include/tsdf_hip_columns.h)
    _abi.declare(lib, table=_abi.COLUMNS_SIGNATURES)
    # ... and merging a map into another under a rigid transform (include/tsdf_hip_merge.h)
    _abi.declare(lib, table=_abi.MERGE_SIGNATURES)
    # ... and coarsening a map 2:1 into a map of twice the voxel size (include/tsdf_hip_coarsen.h)
    _abi.declare(lib, table=_abi.COARSEN_SIGNATURES,
                 optional=tuple(_abi.COARSEN_SIGNATURES))
    # ... and the indexed triangle mesh (include/tsdf_hip_mesh.h)
    _abi.declare(lib, table=_abi.MESH_SIGNATURES)
    # ... and the frontier voxels of a box (include/tsdf_hip_frontier.h)
    _abi.declare(lib, table=_abi.FRONTIER_SIGNATURES,
                 optional=tuple(_abi.FRONTIER_SIGNATURES))
    # ... and motion-compensated Ouster frames (include/tsdf_hip_deskew.h)
    _abi.declare(lib, table=_abi.DESKEW_SIGNATURES)
    if lib.tsdf_abi_version() != ABI_VERSION:
        raise RuntimeError("libtsdf_hip.so ABI version mismatch")
    if path is None:
        _hip = lib
    return lib
