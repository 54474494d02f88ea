"""Times tsdf_mesh_indexed against tsdf_extract_mesh_table on a bench-like map (5 cm voxels,
128 x 1024 scans): medians of warm, alternated calls.  Usage:
    python profiles/mesh_bench.py [scans] [out.json]
One JSON line at the end, also written to the output file (default profiles/mesh/mesh_bench.json).
No GPU: the script fails."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "noetic-slam_amd"), os.path.join(REPO, "oracle"), REPO):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tsdf_map import HipTSDFVolume, _abi  # noqa: E402
from tsdf_map.scan_gen import TorchOusterSim  # noqa: E402

N_SCANS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
BATCH = 16
dev = torch.device("cuda", 0)
sim = TorchOusterSim(dev)
vol = HipTSDFVolume(0.05, 0.15, max_points=1 << 18, max_bricks=1 << 20, max_batch=BATCH)
for k0 in range(0, N_SCANS, BATCH):
    x, offs, org = sim.scans(k0, BATCH)
    vol.integrate_batch_device(x.data_ptr(), offs, org)
vol.sync()
nb = vol.num_bricks()
lib, ctx = vol._lib, vol._ctx

n = C.c_uint64()
assert lib.tsdf_extract_mesh_table(ctx, 0.0, 0, None, 0, C.byref(n)) == 0
T = n.value
soup = np.empty((T, 9), np.float32)
cnt = _abi.MeshCounts()
assert lib.tsdf_mesh_indexed_count(ctx, 0.0, 0, None, None, C.byref(cnt)) == 0
V = cnt.n_vertices
assert cnt.n_triangles == T
vert = np.empty((V, 3), np.float32)
nrm = np.empty((V, 3), np.float32)
tri = np.empty((T, 3), np.uint32)
dvert = torch.empty((V, 3), dtype=torch.float32, device=dev)
dnrm = torch.empty((V, 3), dtype=torch.float32, device=dev)
dtri = torch.empty((T, 3), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
FP, U32P = _abi.FP, _abi.U32P


def run_soup():
    assert lib.tsdf_extract_mesh_table(ctx, 0.0, 0, soup.ctypes.data_as(FP), T, C.byref(n)) == 0


def run_soup_count():
    assert lib.tsdf_extract_mesh_table(ctx, 0.0, 0, None, 0, C.byref(n)) == 0


def run_indexed():
    assert lib.tsdf_mesh_indexed(ctx, 0.0, 0, None, None, vert.ctypes.data_as(FP),
                                 nrm.ctypes.data_as(FP), tri.ctypes.data_as(U32P), V, T,
                                 C.byref(cnt)) == 0


def run_indexed_nonormals():
    assert lib.tsdf_mesh_indexed(ctx, 0.0, 0, None, None, vert.ctypes.data_as(FP), None,
                                 tri.ctypes.data_as(U32P), V, T, C.byref(cnt)) == 0


def run_indexed_count():
    assert lib.tsdf_mesh_indexed_count(ctx, 0.0, 0, None, None, C.byref(cnt)) == 0


def run_indexed_device():
    assert lib.tsdf_mesh_indexed_device(ctx, 0.0, 0, None, None, C.c_void_p(dvert.data_ptr()),
                                        C.c_void_p(dnrm.data_ptr()), C.c_void_p(dtri.data_ptr()),
                                        V, T, C.byref(cnt)) == 0


legs = {"soup": run_soup, "indexed": run_indexed, "indexed_no_normals": run_indexed_nonormals,
        "indexed_device": run_indexed_device, "soup_count": run_soup_count,
        "indexed_count": run_indexed_count}
times = {k: [] for k in legs}
for rep in range(2 + 11):  # two warm rounds, then eleven timed, the legs alternating
    for k, fn in legs.items():
        t0 = time.perf_counter()
        fn()  # every call ends in a stream synchronise and its copies
        dt = time.perf_counter() - t0
        if rep >= 2:
            times[k].append(dt * 1e3)
same = bool(np.array_equal(vert[tri.reshape(-1).astype(np.int64)].view(np.uint32).reshape(-1, 9),
                           soup.view(np.uint32)))
out = {"scans": N_SCANS, "bricks": nb, "triangles": T, "vertices": V,
       "soup_bytes": T * 36, "indexed_bytes": T * 12 + V * 24,
       "indexed_bytes_no_normals": T * 12 + V * 12,
       "bytes_per_triangle": round((T * 12 + V * 24) / max(T, 1), 2),
       "deindexed_equals_soup": same,
       "ms_median": {k: round(statistics.median(v), 3) for k, v in times.items()},
       "ms_min": {k: round(min(v), 3) for k, v in times.items()},
       "ms_max": {k: round(max(v), 3) for k, v in times.items()}}
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "mesh", "mesh_bench.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
