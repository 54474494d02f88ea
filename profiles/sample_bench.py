#!/usr/bin/env python3
"""Throughput of the sparse map queries (include/tsdf_hip_sample.h) on the GPU.

The map is the benchmark's C1 workload (bench.py: --scans synthetic Ouster scans at 5 cm, one
batch); the queries are one fresh scan of 131072 points, resident in HBM.  Reported per entry point
(tsdf_sample_device nearest / trilinear, tsdf_align_terms_device): microseconds per call and
points per second, as a host clock around calls that each end in a device synchronise.

With --variant PATH (a library built with other knobs, e.g. `make -C noetic-slam_amd/csrc variants
VARIANTS="sample_shared:-DTSDF_SAMPLE_SHARED=1"` -> lib/var/libtsdf_hip_sample_shared.so) both
libraries are loaded into this process, each builds the same map in a context of its own, and the
timed rounds alternate between them: the A/B of the shipped per-lane brick probes against the
wave-shared lookup.  Their outputs are compared bit for bit first.  "call_floor" is the trilinear
call on 64 points: what a call costs before the cloud's size matters (flush, launch, synchronise).

Every shape is warmed up; each figure is the median over --rounds rounds of --reps calls, with the
rounds' minimum and maximum as the spread.  One JSON line on stdout, and the same object in --out.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", type=int, default=64, help="scans fused into the map (C1: 64)")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--trunc", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=2000, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--variant", default=None, metavar="LIB",
                    help="a second libtsdf_hip.so to interleave with the shipped one")
    ap.add_argument("--variant-name", default="shared")
    ap.add_argument("--integrate-ms-per-scan", type=float, default=None,
                    help="bench.py's ms_per_step / batch on the same machine: the yardstick")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample", "sample_bench.json"))
    return ap.parse_args()


class Side:
    """One library, its context and map, and its output buffers."""

    def __init__(self, name, lib, args, cloud, offs, origins, dev):
        import torch
        from tsdf_map.volume import TSDFVolume
        self.name = name
        self.vol = TSDFVolume(lib, args.voxel, args.trunc, max_points=1 << 17,
                              max_batch=min(args.scans, 512), semantics="vdbfusion_f64")
        v = self.vol
        org = np.ascontiguousarray(origins, np.float64)
        o = np.ascontiguousarray(offs, np.uint64)
        from tsdf_map import _abi
        v._check(lib.tsdf_integrate_batch_device(v._ctx, C.c_void_p(cloud.data_ptr()),
                                                 o.ctypes.data_as(_abi.U64P), org.shape[0],
                                                 org.ctypes.data_as(_abi.D3)), "integrate")
        v.sync()
        n = 1 << 17
        self.s = torch.zeros(n, dtype=torch.float32, device=dev)
        self.w = torch.zeros(n, dtype=torch.float32, device=dev)
        self.g = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.out = np.empty(44, np.float64)
        self.pose = np.ascontiguousarray(np.eye(4)[:3])
        torch.cuda.synchronize()

    def sample(self, q, n, mode):
        v = self.vol
        v._check(v._lib.tsdf_sample_device(v._ctx, C.c_void_p(q), n, mode, 0.0,
                                           C.c_void_p(self.s.data_ptr()),
                                           C.c_void_p(self.w.data_ptr()),
                                           C.c_void_p(self.g.data_ptr()),
                                           C.c_void_p(self.v.data_ptr())), "sample_device")

    def align(self, q, n):
        from tsdf_map import _abi
        v = self.vol
        v._check(v._lib.tsdf_align_terms_device(v._ctx, C.c_void_p(q), n,
                                                self.pose.ctypes.data_as(_abi.D3), 0.0,
                                                self.out.ctypes.data_as(_abi.D3)), "align_terms")

    def run(self, op, q, n):
        if op == "call_floor":
            self.sample(q, min(n, 64), 1)
        elif op == "align_terms":
            self.align(q, n)
        else:
            self.sample(q, n, 0 if op == "nearest" else 1)


def main():
    args = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sample_bench needs a GPU: nothing is measured without one")
    from tsdf_map import load_hip_library
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    cloud, offs, origins = sim.scans(0, args.scans)
    q_t, _ = sim.scan(args.scans)  # a fresh scan: the next pose on the circle
    q_t = q_t.contiguous()
    n = int(q_t.shape[0])
    torch.cuda.synchronize()
    q = q_t.data_ptr()

    libs = [("per_lane", load_hip_library())]
    if args.variant:
        vlib = load_hip_library(os.path.abspath(args.variant))
        libs.append((args.variant_name, vlib))
    sides = [Side(name, lib, args, cloud, offs, origins, dev) for name, lib in libs]
    ops = ("call_floor", "nearest", "trilinear", "align_terms")

    # outputs agree bit for bit between the libraries (and the warm-up of every shape)
    check = {}
    for sd in sides:
        got = {}
        for op in ops:
            for _ in range(args.warmup):
                sd.run(op, q, n)
            if op == "align_terms":
                got[op] = sd.out.copy().view(np.uint64)
            else:
                got[op] = [t.cpu().numpy().view(np.uint8).copy() for t in (sd.s, sd.w, sd.g, sd.v)]
        check[sd.name] = got
    valid_share = float(sides[0].v.float().mean().item())  # trilinear was the last sample call
    same = True
    for sd in sides[1:]:
        for op in ops:
            a, b = check[sides[0].name][op], check[sd.name][op]
            same &= (np.array_equal(a, b) if op == "align_terms"
                     else all(np.array_equal(x, y) for x, y in zip(a, b)))
    if not same:
        sys.exit("the libraries' outputs differ: not an A/B of the same computation")

    us = {sd.name: {op: [] for op in ops} for sd in sides}
    for _ in range(args.rounds):
        for op in ops:
            for sd in sides:  # alternate the libraries within every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    sd.run(op, q, n)
                us[sd.name][op].append((time.perf_counter() - t0) / args.reps * 1e6)

    res = {"workload": "C1 map: %d synthetic os1_128_1024 scans at %g m; queries: scan %d, %d points"
                       % (args.scans, args.voxel, args.scans, n),
           "timing": "host clock over %d calls, each ending in a stream synchronise; median "
                     "[min, max] of %d interleaved rounds" % (args.reps, args.rounds),
           "n_points": n, "bricks": sides[0].vol.num_bricks(),
           "trilinear_valid_share": round(valid_share, 4),
           "align_n_valid": int(sides[0].out[43]),
           "outputs_bitwise_equal_across_variants": bool(same) if len(sides) > 1 else None,
           "shipped": libs[0][0], "variants": {}}
    for sd in sides:
        r = {}
        for op in ops:
            v = us[sd.name][op]
            med = statistics.median(v)
            r[op] = {"us_per_call": round(med, 2), "us_min": round(min(v), 2),
                     "us_max": round(max(v), 2)}
            if op == "call_floor":
                continue
            r[op]["mpoints_per_s"] = round(n / med, 1)
            if args.integrate_ms_per_scan:
                r[op]["share_of_integrate"] = round(med / 1e3 / args.integrate_ms_per_scan, 4)
        res["variants"][sd.name] = r
    if args.integrate_ms_per_scan:
        res["integrate_ms_per_scan"] = args.integrate_ms_per_scan
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for sd in sides:
        sd.vol.close()


if __name__ == "__main__":
    main()
