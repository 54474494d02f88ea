#!/usr/bin/env python3
"""Time of the column maps (include/tsdf_hip_columns.h) on the GPU against the dense read-out.

The map is the benchmark's C1 workload (bench.py: --scans synthetic Ouster scans at 5 cm, one
batch).  Two boxes: 40 m x 40 m x 3 m around the last scan's origin ("robot"), and the map's whole
x, y extent by 10 m around that origin's height ("whole").  Per box the script times, as a
device-synchronised host clock after a warm-up, with enough repeats to fill about --seconds, the
two routes alternating call by call in one process:

  column_map_device   tsdf_column_map_device into resident device buffers (all five outputs)
  query_dense         tsdf_query_dense of the same box into host arrays: the only route to the
                      same answer without this feature, its read-out alone (no host reduction)

and, once the alternation is done, column_map (tsdf_column_map into host arrays) the same way.
Each entry holds the median and [min, max] of the repeats.  The kernel's algorithmic bytes are 8 B
per voxel of the held bricks inside the box plus 15 B per column; they are reported over the
column_map_device time as a share of the 8 TB/s HBM peak.  The device result of a 400 x 400
sub-box of the robot box is compared bit for bit with tests/colref.py before anything is timed.
One JSON line on stdout, and the same object in --out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "noetic-slam_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8.0e12  # bytes / s (MI355X, HBM3E spec)


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", type=int, default=64, help="scans fused into the map (C1: 64)")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--trunc", type=float, default=0.15)
    ap.add_argument("--seconds", type=float, default=1.0, help="time to fill per route and box")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "columns", "columns_time.json"))
    return ap.parse_args()


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "repeats": len(t)}


def clock(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, seconds, warmup, sync):
    """The calls of `fns` in turn, round after round, until the slowest has filled `seconds`."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    while max(sum(v) for v in t.values()) < seconds * 1e3 or len(next(iter(t.values()))) < 3:
        for k, fn in fns.items():
            t[k].append(clock(fn, sync))
    return {k: summary(v) for k, v in t.items()}


def held_voxels(coords, lo, hi):
    """Voxels of the held bricks that lie inside the box."""
    b0 = coords.astype(np.int64) * 8
    ov = np.clip(np.minimum(b0 + 8, hi) - np.maximum(b0, lo), 0, 8)
    return int(ov.prod(1).sum())


def main():
    args = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit("columns_time needs a GPU: nothing is measured without one")
    import colref as cr
    from tsdf_map import HipTSDFVolume, _abi
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    cloud, offs, origins = sim.scans(0, args.scans)
    torch.cuda.synchronize()
    v = HipTSDFVolume(args.voxel, args.trunc, max_points=1 << 17, max_batch=min(args.scans, 512),
                      semantics="vdbfusion_f64")
    v.integrate_batch_device(cloud.data_ptr(), offs, origins)
    v.sync()
    coords = v.export_bricks()[0]
    c = np.floor(np.asarray(origins, np.float64)[-1] / args.voxel).astype(np.int64)
    vox = lambda m: int(round(m / args.voxel))  # noqa: E731
    boxes = {"robot": (c - [vox(20), vox(20), vox(1.5)], c + [vox(20), vox(20), vox(1.5)])}
    ext_lo, ext_hi = coords.min(0).astype(np.int64) * 8, coords.max(0).astype(np.int64) * 8 + 8
    boxes["whole"] = (np.array([ext_lo[0], ext_lo[1], c[2] - vox(5)]),
                      np.array([ext_hi[0], ext_hi[1], c[2] + vox(5)]))
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    res = {"scans": args.scans, "voxel": args.voxel, "bricks": int(v.num_bricks()),
           "hbm_peak_bytes_per_s": HBM_PEAK, "boxes": {}}

    # bit for bit against the reference, on a sub-box the host reduction takes in a few seconds
    lo, hi = boxes["robot"]
    slo, shi = lo + [vox(10), vox(10), 0], hi - [vox(10), vox(10), 0]
    ref = cr.of_volume(v, slo, shi, args.voxel, 0.0, 2, 2)
    d = v.column_map_device(slo, shi, occ_band=args.voxel, min_occ=2, min_free=2)
    cr.assert_same([t.cpu().numpy() for t in d], ref)
    res["bitwise"] = {"box": [int(e) for e in shi - slo],
                      "elev": int((ref[4] & cr.HAS_ELEV != 0).sum()),
                      "ceil": int((ref[4] & cr.HAS_CEIL != 0).sum()),
                      "occupied": int((ref[4] & cr.OCCUPIED != 0).sum()),
                      "free": int((ref[4] & cr.FREE != 0).sum())}
    del ref, d

    for name, (lo, hi) in boxes.items():
        lo, hi = np.ascontiguousarray(lo, np.int64), np.ascontiguousarray(hi, np.int64)
        n = hi - lo
        cells = int(n[0] * n[1])
        tt = (torch.float32, torch.float32, torch.uint16, torch.uint16, torch.uint8)
        out = [torch.empty(cells, dtype=dt, device=dev) for dt in tt]
        S = np.empty((n[2], n[1], n[0]), np.float32)
        W = np.empty_like(S)
        pl, ph = lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3)

        def columns():
            v._check(v._lib.tsdf_column_map_device(
                v._ctx, pl, ph, args.voxel, 0.0, 2, 2, *[C.c_void_p(t.data_ptr()) for t in out]),
                "column_map_device")

        def dense():
            v._check(v._lib.tsdf_query_dense(v._ctx, pl, ph, S.ctypes.data_as(_abi.FP),
                                             W.ctypes.data_as(_abi.FP)), "query_dense")

        r = alternate({"column_map_device": columns, "query_dense": dense}, args.seconds,
                      args.warmup, sync)
        del S, W
        r.update(alternate({"column_map": lambda: v.column_map(lo, hi, occ_band=args.voxel,
                                                               min_occ=2, min_free=2)},
                           args.seconds, args.warmup, sync))
        held = held_voxels(coords, lo, hi)
        alg = 8 * held + 15 * cells
        t = r["column_map_device"]["median_ms"] * 1e-3
        r.update({"box": [int(e) for e in n], "voxels": int(n.prod()), "columns": cells,
                  "held_voxels": held, "algorithmic_bytes": alg,
                  "bytes_per_s": alg / t, "share_of_hbm_peak": alg / t / HBM_PEAK,
                  "dense_bytes": 8 * int(n.prod()),
                  "query_dense_over_device": r["query_dense"]["median_ms"] /
                  r["column_map_device"]["median_ms"],
                  "query_dense_over_host": r["query_dense"]["median_ms"] /
                  r["column_map"]["median_ms"]})
        res["boxes"][name] = r
        del out
    v.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
