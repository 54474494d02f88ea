#!/usr/bin/env python3
"""Time of the distance field (include/tsdf_hip_esdf.h) on the GPU.

The map is the benchmark's C1 workload (bench.py: --scans synthetic Ouster scans at 5 cm, one
batch).  The box is 20 m x 20 m x 4 m around the last scan's origin: 400 x 400 x 80 = 12.8 M voxels.
For each radius (20 and 40 voxels: 1 m and 2 m) the script reports, as a host clock around
synchronous calls after a warm-up, the median and [min, max] of --rounds rounds:

  esdf_device   tsdf_esdf_dense_device into resident device buffers
  esdf_host     tsdf_esdf_dense into host arrays
  query_dense   tsdf_query_dense of the same box: the floor any dense read-out pays
  parent_route  what a user did before the library had this: query_dense, then the distance
                transform on the host (tests/esdfref.py, numpy); timed once per radius

The GPU result is compared bit for bit with the reference before anything is timed.  One JSON line
on stdout, and the same object in --out.  For kernel times run it alone under
`rocprofv3 --kernel-trace --stats -- python profiles/esdf_bench.py --rounds 3`.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", type=int, default=64, help="scans fused into the map (C1: 64)")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--trunc", type=float, default=0.15)
    ap.add_argument("--half", type=int, nargs=3, default=[200, 200, 40],
                    help="half extents of the box in voxels")
    ap.add_argument("--radius", type=int, nargs="+", default=[20, 40])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-parent", action="store_true",
                    help="skip the host reference (no bitwise check, no parent_route)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "esdf", "esdf_bench.json"))
    return ap.parse_args()


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    args = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit("esdf_bench needs a GPU: nothing is measured without one")
    import esdfref as er
    from tsdf_map import HipTSDFVolume
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    cloud, offs, origins = sim.scans(0, args.scans)
    torch.cuda.synchronize()
    v = HipTSDFVolume(args.voxel, args.trunc, max_points=1 << 17, max_batch=min(args.scans, 512),
                      semantics="vdbfusion_f64")
    v.integrate_batch_device(cloud.data_ptr(), offs, origins)
    v.sync()
    c = np.floor(np.asarray(origins, np.float64)[-1] / args.voxel).astype(np.int64)
    half = np.array(args.half, np.int64)
    lo, hi = c - half, c + half
    n = int(np.prod(hi - lo))
    res = {"scans": args.scans, "voxel": args.voxel, "bricks": v.num_bricks(),
           "box": [int(e) for e in hi - lo], "voxels": n, "rounds": args.rounds, "radius": {}}

    res["query_dense"] = timed(lambda: v.query_dense(lo, hi), args.rounds, args.warmup)
    for radius in args.radius:
        md = (radius - 0.5) * args.voxel
        r = {}
        if not args.no_parent:
            t0 = time.perf_counter()
            S, W = v.query_dense(lo, hi)
            ref = er.esdf(S, W, args.voxel, radius, args.voxel)
            r["parent_route"] = {"ms": (time.perf_counter() - t0) * 1e3}
            got = v.esdf(lo, hi, md)
            er.assert_same(got, ref)
            d, f = v.esdf_device(lo, hi, md)
            er.assert_same((d.cpu().numpy(), f.cpu().numpy()), ref)
            fl = ref[1]
            r["sites"] = int(((fl & er.SITE) != 0).sum())
            r["capped"] = int(((fl & er.CAPPED) != 0).sum())
            r["bitwise"] = True
            del S, W, ref, got, d, f
        dd = torch.empty(n, dtype=torch.float32, device=dev)
        df = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        from tsdf_map import _abi
        a, b = np.ascontiguousarray(lo), np.ascontiguousarray(hi)

        def device_call():
            v._check(v._lib.tsdf_esdf_dense_device(
                v._ctx, a.ctypes.data_as(_abi.L3), b.ctypes.data_as(_abi.L3), radius,
                args.voxel, 0.0, C.c_void_p(dd.data_ptr()), C.c_void_p(df.data_ptr())), "esdf")
        r["esdf_device"] = timed(device_call, args.rounds, args.warmup)
        r["esdf_host"] = timed(lambda: v.esdf(lo, hi, md), args.rounds, args.warmup)
        q = res["query_dense"]["median_ms"]
        r["device_over_query_dense"] = r["esdf_device"]["median_ms"] / q
        r["host_over_query_dense"] = r["esdf_host"]["median_ms"] / q
        if "parent_route" in r:
            r["parent_over_device"] = r["parent_route"]["ms"] / r["esdf_device"]["median_ms"]
            r["parent_over_host"] = r["parent_route"]["ms"] / r["esdf_host"]["median_ms"]
        res["radius"][str(radius)] = r
    v.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
