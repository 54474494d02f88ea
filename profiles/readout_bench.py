#!/usr/bin/env python3
"""Host-clock cost of the map read-out and exchange calls, one build of libtsdf_hip.so against
another: readout_bench.py NAME=LIB NAME=LIB ... (the first is the yardstick).

The map is the benchmark's C1 workload (bench.py: --scans synthetic Ouster scans at 5 cm, one
batch).  Every library is loaded into this process and builds the same map in a context of its
own; the timed rounds alternate between the libraries, which take turns to go first (the second
to run a call finds the host's caches warm).  Timed per call, each ending synchronised:

  export_bricks        tsdf_export_bricks of the whole map into host arrays
  extract_mesh         tsdf_extract_mesh_table into a host array sized by a count call before
  sample               tsdf_sample, host pointers, the next scan's 131072 points, trilinear
  raycast              tsdf_raycast, host pointers, the same scan's rays from its origin, nearest
  import_bricks        tsdf_import_bricks of the exported map into a fresh context (its creation
                       is not timed)
  border_reduce_local  tsdf_border_reduce_local of two contexts on this GPU that hold the first
                       and the last 60 % of the map's bricks (a call moves the shared fifth)

The libraries' outputs are compared bit for bit first.  A call passes when the median of a later
library lies within the yardstick's own minimum and maximum over its rounds.  One JSON line on
stdout, and the same object with every round in --out.
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

OPS = ("export_bricks", "extract_mesh", "sample", "raycast", "import_bricks", "border_reduce_local")


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("libs", nargs="+", metavar="NAME=LIB")
    ap.add_argument("--scans", type=int, default=64, help="scans fused into the map (C1: 64)")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--trunc", type=float, default=0.15)
    ap.add_argument("--t-max", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readout_refactor", "readout.json"))
    return ap.parse_args()


class Side:
    """One library: its map, the two half maps of the border reduce, and its output arrays."""

    def __init__(self, name, lib, args, cloud, offs, origins, pts, org):
        from tsdf_map import _abi
        from tsdf_map.volume import TSDFVolume
        self.name, self.lib, self.args, self.abi, self.Volume = name, lib, args, _abi, TSDFVolume
        self.vol = v = TSDFVolume(lib, args.voxel, args.trunc, max_points=1 << 17,
                                  max_batch=min(args.scans, 512), semantics="vdbfusion_f64")
        o = np.ascontiguousarray(offs, np.uint64)
        og = np.ascontiguousarray(origins, np.float64)
        v._check(lib.tsdf_integrate_batch_device(v._ctx, C.c_void_p(cloud.data_ptr()),
                                                 o.ctypes.data_as(_abi.U64P), og.shape[0],
                                                 og.ctypes.data_as(_abi.D3)), "integrate")
        v.sync()
        nb = self.nb = v.num_bricks()
        self.coords = np.zeros((nb, 3), np.int32)
        self.sdf = np.zeros((nb, 512), np.float32)
        self.weight = np.zeros((nb, 512), np.float32)
        self.export_bricks()
        n_tri = C.c_uint64()
        v._check(lib.tsdf_extract_mesh_table(v._ctx, 0.0, 0, None, 0, C.byref(n_tri)), "mesh count")
        self.tri = np.zeros((n_tri.value, 9), np.float32)
        # the query: a scan's points, and the rays to them from its origin
        self.pts = np.ascontiguousarray(pts, np.float32)
        n = self.n = self.pts.shape[0]
        d = self.pts.astype(np.float64) - np.asarray(org, np.float64)
        self.dirs = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), np.float32)
        self.orgs = np.ascontiguousarray(np.broadcast_to(np.asarray(org, np.float32), (n, 3)))
        self.q_sdf, self.q_w = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.q_grad, self.q_ok = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        self.depth, self.normal = np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        self.hit = np.zeros(n, np.uint8)
        # two contexts on this GPU sharing a fifth of the bricks
        p = TSDFVolume.make_params(lib, args.voxel, args.trunc, max_bricks=self.room(),
                                   max_points=1 << 12, max_batch=4, semantics="vdbfusion_f64")
        out = (C.c_void_p * 2)()
        ids = (C.c_int32 * 2)(0, 0)
        if lib.tsdf_create_sharded(C.byref(p), 2, ids, out) != _abi.TSDF_OK:
            sys.exit("tsdf_create_sharded failed")
        self.pair = out
        cut = (0, nb * 3 // 5), (nb * 2 // 5, nb)
        for k, (a, b) in enumerate(cut):
            self.load(C.c_void_p(out[k]), a, b)
        self.moved = C.c_uint64()
        self.fresh = None

    def room(self):
        return max(1 << 12, 1 << int(2 * self.nb).bit_length())

    def fp(self, a):
        return a.ctypes.data_as(self.abi.FP)

    def ok(self, rc, what):
        if rc != self.abi.TSDF_OK:
            sys.exit("%s: %s failed (%d)" % (self.name, what, rc))

    def load(self, ctx, a, b):
        self.ok(self.lib.tsdf_import_bricks(ctx, self.coords[a:b].ctypes.data_as(self.abi.I3),
                                            self.fp(self.sdf[a:b]), self.fp(self.weight[a:b]), b - a),
                "import_bricks")

    def export_bricks(self):
        n = C.c_uint64()
        self.ok(self.lib.tsdf_export_bricks(self.vol._ctx, self.coords.ctypes.data_as(self.abi.I3),
                                            self.fp(self.sdf), self.fp(self.weight), self.nb,
                                            C.byref(n)), "export_bricks")

    def extract_mesh(self):
        n = C.c_uint64()
        self.ok(self.lib.tsdf_extract_mesh_table(self.vol._ctx, 0.0, 0, self.fp(self.tri),
                                                 self.tri.shape[0], C.byref(n)), "extract_mesh")

    def sample(self):
        self.ok(self.lib.tsdf_sample(self.vol._ctx, self.pts.ctypes.data_as(C.c_void_p), self.n, 12, 0,
                                     0, 1, 0.0, self.fp(self.q_sdf), self.fp(self.q_w),
                                     self.fp(self.q_grad), self.q_ok.ctypes.data_as(self.abi.U8P)),
                "sample")

    def raycast(self):
        a = self.args
        self.ok(self.lib.tsdf_raycast(self.vol._ctx, self.fp(self.orgs), self.fp(self.dirs), self.n,
                                      None, 0.0, a.t_max, a.voxel / 2, 0, 0.0, self.fp(self.depth),
                                      self.fp(self.normal), self.hit.ctypes.data_as(self.abi.U8P)),
                "raycast")

    def prepare(self, op):
        """What a call needs and the clock must not see: import's fresh context."""
        if op == "import_bricks":
            a = self.args
            self.fresh = self.Volume(self.lib, a.voxel, a.trunc, max_bricks=self.room(),
                                     max_points=1 << 12, max_batch=4, semantics="vdbfusion_f64")

    def import_bricks(self):
        self.load(self.fresh._ctx, 0, self.nb)

    def border_reduce_local(self):
        self.ok(self.lib.tsdf_border_reduce_local(self.pair, 2, C.byref(self.moved)),
                "border_reduce_local")

    def finish(self, op):
        if op == "import_bricks":
            self.fresh.close()
            self.fresh = None

    def outputs(self):
        return [x.view(np.uint8).copy() for x in (self.coords, self.sdf, self.weight, self.tri,
                                                  self.q_sdf, self.q_w, self.q_grad, self.q_ok,
                                                  self.depth, self.normal, self.hit)]

    def close(self):
        self.vol.close()
        for k in range(2):
            self.lib.tsdf_destroy(C.c_void_p(self.pair[k]))


def main():
    args = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit("readout_bench needs a GPU: nothing is measured without one")
    from tsdf_map import load_hip_library
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    cloud, offs, origins = sim.scans(0, args.scans)
    q_t, q_org = sim.scan(args.scans)  # a fresh scan: the next pose on the circle
    pts = q_t.cpu().numpy()
    torch.cuda.synchronize()
    sides = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        sides.append(Side(name, load_hip_library(os.path.abspath(path)), args, cloud, offs, origins,
                          pts, q_org))

    def timed(sd, op, reps):
        t = 0.0
        for _ in range(reps):
            sd.prepare(op)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            getattr(sd, op)()
            t += time.perf_counter() - t0
            sd.finish(op)
        return t / reps * 1e3

    for sd in sides:  # warm-up, and the outputs to compare
        for op in OPS:
            timed(sd, op, 1)
    first = sides[0].outputs()
    same = all(np.array_equal(x, y) for sd in sides[1:] for x, y in zip(first, sd.outputs()))
    same = same and all(sd.moved.value == sides[0].moved.value for sd in sides)
    if not same:
        sys.exit("the libraries' outputs differ: not an A/B of the same computation")

    ms = {sd.name: {op: [] for op in OPS} for sd in sides}
    for r in range(args.rounds):
        k = r % len(sides)  # the libraries alternate within a round, and take turns to go first
        for op in OPS:
            for sd in sides[k:] + sides[:k]:
                ms[sd.name][op].append(round(timed(sd, op, args.reps), 4))

    base = sides[0].name
    res = {"workload": "C1 map: %d synthetic os1_128_1024 scans at %g m, %d bricks, %d triangles; "
                       "queries: scan %d's %d points and the rays to them"
                       % (args.scans, args.voxel, sides[0].nb, sides[0].tri.shape[0], args.scans,
                          sides[0].n),
           "timing": "host clock per call in ms, mean of %d calls per round, %d rounds alternating "
                     "between the libraries; pass: median within %s's [min, max]"
                     % (args.reps, args.rounds, base),
           "outputs_bitwise_equal": bool(same), "border_tiles_moved": sides[0].moved.value,
           "rounds_ms": ms, "median_ms": {}, "verdict": {}}
    for sd in sides:
        res["median_ms"][sd.name] = {op: round(statistics.median(ms[sd.name][op]), 4) for op in OPS}
    for sd in sides[1:]:
        v = {}
        for op in OPS:
            lo, hi = min(ms[base][op]), max(ms[base][op])
            med = res["median_ms"][sd.name][op]
            v[op] = {"median_ms": med, "yardstick_min_ms": lo, "yardstick_max_ms": hi,
                     "pass": bool(lo <= med <= hi),
                     "over_yardstick_median": round(med / res["median_ms"][base][op], 4)}
        res["verdict"][sd.name] = v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("workload", "outputs_bitwise_equal", "median_ms", "verdict")}))
    for sd in sides:
        sd.close()


if __name__ == "__main__":
    main()
