#!/usr/bin/env python3
"""The device 2:1 coarsening against the only route there was before it.

Source: the bench workload's map after --scans scans (bench.py's sensor, trajectory and parameters;
64 scans at 5 cm: the C1 map of §11, §14 and §15).  It is coarsened (a) into an empty context of
10 cm voxels and (b) into a copy of that result, two ways:

  coarsen  tsdf_coarsen_into: parents, flags, counts, insert, reduce + fuse, all in HBM; the counts
           are the only bytes that cross PCIe
  route    what a caller had to do before: tsdf_export_bricks (the source over PCIe), the numpy
           restatement of the header's rules 1-7 on the host (tests/coarsenref.py), and
           tsdf_import_bricks of the coarse bricks (the result up)

Before anything is timed the two results are compared bitwise (export_bricks of both
destinations).  Then both are timed in the same process, rounds alternating, with a host clock over
calls that end in a device synchronise: one warm-up round, then --rounds rounds; median [min, max].
The destination of every round is created (and, for (b), filled) outside the timed region.

Bytes are computed from the brick counts.  Kernel times are not measured here: run the script with
--rounds 1 under `rocprofv3 --kernel-trace` in a run of its own and give the trace to
--kernel-trace, which prints the coarsening kernels' calls, mean and least times (the unique
bytes to set against them are in this script's "bytes").  TSDF_HIP_LIB selects another build of the library (how the A/B of the
two access patterns in DESIGN.md §24 was run).

One JSON line at the end, also written to --out.  No GPU: the script fails.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "noetic-slam_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

F = np.float32
VS, TAU = 0.05, 0.15
BRICK_BYTES = 2 * 512 * 4  # sdf + weight
KERNELS = ("k_coarsen_parents", "k_coarsen_flag", "k_merge_insert", "k_coarsen_apply",
           "k_import_insert", "k_import_merge", "k_fill")


def kernel_times(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            kind = next((k for k in KERNELS if k in name), None)
            if kind is None:
                continue
            e = out.setdefault(kind, {"calls": 0, "ns": 0, "min_ns": None})
            dt = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            e["calls"] += 1
            e["ns"] += dt
            e["min_ns"] = dt if e["min_ns"] is None else min(e["min_ns"], dt)
    for e in out.values():
        e["us_per_call"] = round(e["ns"] / 1e3 / e["calls"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-bricks", type=int, default=1 << 18)
    ap.add_argument("--skip-route", action="store_true",
                    help="time the device call only (a kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "coarsen", "coarsen_bench.json"))
    ap.add_argument("--kernel-trace", default=None, metavar="CSV",
                    help="a rocprofv3 kernel trace of an earlier run of this script: print the "
                         "coarsening kernels' calls and mean times, and exit")
    args = ap.parse_args()
    if args.kernel_trace:
        print(json.dumps({"kernels": kernel_times(args.kernel_trace)}))
        return

    import torch
    assert torch.cuda.is_available(), "coarsen_bench needs a GPU"
    import coarsenref as cr
    from tsdf_map import HipTSDFVolume
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    steps = [sim.scans(k0, args.batch) for k0 in range(0, args.scans, args.batch)]
    torch.cuda.synchronize()
    max_pts = max(int(np.diff(o).max()) for _, o, _ in steps)

    def make(vs):
        return HipTSDFVolume(vs, TAU, max_points=max(max_pts, 1 << 20),
                             max_bricks=args.max_bricks, max_batch=args.batch, pipeline=2)

    src = make(VS)
    for x, offs, org in steps:
        src.integrate_batch_device(x.data_ptr(), offs, org)
    src.sync()
    nb = src.num_bricks()
    first = make(2 * VS)
    first.coarsen_from(src)
    held = first.export_bricks()
    first.close()

    def fresh(into):
        d = make(2 * VS)
        if into == "copy":
            d.import_bricks(*held)
        return d

    def route(dst):
        """The parent's route; returns the PCIe bytes it moved."""
        own = src.export_bricks()
        exp = cr.coarsen(cr.empty_bricks(), own, F(TAU))
        dst.import_bricks(*exp[:3])
        return BRICK_BYTES * (len(own[0]) + len(exp[0]))

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def same(a, b):
        return (np.array_equal(a[0], b[0]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
                and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))

    out = {"scans": args.scans, "src_bricks": nb, "rounds": args.rounds, "max_bricks": args.max_bricks,
           "library": os.environ.get("TSDF_HIP_LIB", "default"), "workloads": {}}
    legs = ("coarsen",) if args.skip_route else ("coarsen", "route")
    for into in ("empty", "copy"):
        a = fresh(into)
        st = a.coarsen_from(src)
        pcie = 0
        if not args.skip_route:  # the comparison first
            b = fresh(into)
            pcie = route(b)
            assert same(a.export_bricks(), b.export_bricks()), into
            b.close()
        a.close()
        t = {k: [] for k in legs}
        for rnd in range(args.rounds + 1):  # round 0 warms both paths up and is not reported
            for leg in legs:
                d = fresh(into)
                if leg == "coarsen":
                    dt, _ = clock(lambda: d.coarsen_from(src))
                else:
                    dt, _ = clock(lambda: route(d))
                d.close()
                if rnd:
                    t[leg].append(dt)
        ms = {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        touched = st["touched_bricks"]
        w = {
            "counts": st, "bitwise_equal_to_route": not args.skip_route, "ms": ms,
            "median_min_max_ms": {k: [round(1e3 * med[k], 3), min(ms[k]), max(ms[k])] for k in t},
            # unique bytes: flag reads the source's weights and the held parents' weights; apply
            # reads the source's (S, W) -- 8 B per child voxel -- and reads and writes the touched
            # bricks' (S, W) -- 8 B per destination voxel each way; the route's PCIe traffic
            # against the call's 56 B of counts
            "bytes": {"flag_read": nb * BRICK_BYTES // 2
                      + (touched - st["new_bricks"]) * BRICK_BYTES // 2,
                      "apply_src_read": nb * BRICK_BYTES, "apply_dst_read": touched * BRICK_BYTES,
                      "apply_dst_write": touched * BRICK_BYTES,
                      "route_pcie": pcie, "coarsen_pcie": 56 + 16},
        }
        if not args.skip_route:
            w["route_over_coarsen"] = round(med["route"] / med["coarsen"], 1)
        out["workloads"][into] = w
        print(into, w["median_min_max_ms"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
