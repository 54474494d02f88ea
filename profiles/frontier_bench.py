#!/usr/bin/env python3
"""The frontier voxels on the device against the only route there was before them.

Maps: the bench workload's map after --scans scans (bench.py's sensor, trajectory and parameters;
64 scans at 5 cm: the C1 map of §11, §14 and §15), built twice: as benchmarked, and with
space_carving=True and --max-range (the maps frontiers are meant for).  On each, at connectivity 6 and 26:

  device_box   tsdf_frontier_voxels_device of a --box-m box (40 m x 40 m x 3 m) around the map's
               middle brick, into buffers allocated beforehand
  device_map   the same for the whole map (lo = hi = NULL)
  route_box    what a caller had to do before, for the box only: tsdf_query_dense of the box grown
               by one voxel (8 B per voxel over PCIe) and the numpy restatement of the header's
               rules on the host (tests/frontierref.py), at connectivity 6 only (the host stencil
               at 26 takes several times as long and adds nothing to the comparison).  The whole
               map has no dense route: there is nothing to time.

Before anything is timed the device result is compared with the route's, every output as integers.
Then the legs are timed in one process, rounds alternating, with a host clock over calls that end
in a device synchronise: one warm-up round, then --rounds rounds (the route: --route-rounds);
median [min, max].

Bytes are computed from the brick counts: 8 B per voxel of the listed bricks and of their
one-voxel halos (10^3 cells per brick), read once by the count pass and once more by the emit pass
for the bricks that have frontier voxels, plus 16 B per frontier voxel written.  "floor_ms" sets
them against --hbm-gbs (the HBM peak of MI355X_MICROARCH: 8 TB/s); the call also holds two host
round trips (counts down, offsets up) that no kernel time contains.

--ab: the two kernel variants of DESIGN.md §25 against the base kernel, on both maps.  It needs
a build of the library with -DTSDF_FRONTIER_AB=1 (TSDF_HIP_LIB), in which TSDF_FRONTIER_VARIANT
selects the variant per launch (bit 0: leave early when the brick holds no free voxel of the box;
bit 1: load only the 6 face neighbours' cells at connectivity 6); the shipped library has neither
the switch nor the losers' code.  Variants alternate within every round, on the same map, and
their outputs are compared bitwise first.

One JSON line at the end, also written to --out.  No GPU: the script fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "noetic-slam_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

VS, TAU = 0.05, 0.15
VOXEL_BYTES = 8        # sdf + weight
TILE_CELLS = 1000      # a brick and its one-voxel halo
OUT_BYTES = 12 + 1 + 3
VARIANTS = {"base": 0, "early": 1, "face6": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--route-rounds", type=int, default=2)
    ap.add_argument("--max-bricks", type=int, default=1 << 18)
    ap.add_argument("--max-bricks-carved", type=int, default=1 << 20)
    ap.add_argument("--max-range", type=float, default=30.0,
                    help="the carved map's max_range (space carving needs a finite one)")
    ap.add_argument("--box-m", type=float, nargs=3, default=[40.0, 40.0, 3.0])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--skip-route", action="store_true")
    ap.add_argument("--ab", action="store_true", help="time the kernel variants (an A/B build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "frontier",
                                "frontier_ab.json" if args.ab else "frontier_bench.json")

    import torch
    assert torch.cuda.is_available(), "frontier_bench needs a GPU"
    import frontierref as fr
    from tsdf_map import HipTSDFVolume, _abi
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    steps = [sim.scans(k0, args.batch) for k0 in range(0, args.scans, args.batch)]
    torch.cuda.synchronize()
    max_pts = max(int(np.diff(o).max()) for _, o, _ in steps)

    def build(carve):
        v = HipTSDFVolume(VS, TAU, space_carving=carve, **({"max_range": args.max_range} if carve else {}),
                          max_points=max(max_pts, 1 << 20),
                          max_bricks=args.max_bricks_carved if carve else args.max_bricks,
                          max_batch=args.batch, pipeline=2)
        t0 = time.perf_counter()
        for x, offs, org in steps:
            v.integrate_batch_device(x.data_ptr(), offs, org)
        v.sync()
        return v, time.perf_counter() - t0

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def buffers(n):
        return (torch.empty((n, 3), dtype=torch.int32, device=dev),
                torch.empty((n,), dtype=torch.uint8, device=dev),
                torch.empty((n, 3), dtype=torch.int8, device=dev))

    def device_call(v, lo, hi, conn, buf):
        """tsdf_frontier_voxels_device through ctypes into buf; returns the counts."""
        st = _abi.FrontierCounts()
        plo = None if lo is None else lo.ctypes.data_as(_abi.L3)
        phi = None if hi is None else hi.ctypes.data_as(_abi.L3)
        rc = v._lib.tsdf_frontier_voxels_device(v._ctx, plo, phi, VS, 0.0, conn, 1,
                                                *[C.c_void_p(t.data_ptr()) for t in buf],
                                                buf[0].shape[0], C.byref(st))
        assert rc == _abi.TSDF_OK, v._lib.tsdf_last_error(v._ctx).decode()
        return st.as_dict()

    def route(v, lo, hi, conn):
        S, W = v.query_dense(lo - 1, hi + 1)
        return fr.dense(S, W, lo, hi, VS, 0.0, conn, 1)

    def box_of(v):
        c = v.brick_coords().astype(np.int64)
        mid = 8 * np.median(c, axis=0).astype(np.int64) + 4
        half = np.round(np.asarray(args.box_m) / VS / 2).astype(np.int64)
        return np.ascontiguousarray(mid - half), np.ascontiguousarray(mid + half)

    def bytes_of(st):
        read = (st["n_bricks"] + st["n_frontier_bricks"]) * TILE_CELLS * VOXEL_BYTES
        return {"read": read, "written": st["n_voxels"] * OUT_BYTES,
                "floor_ms": round((read + st["n_voxels"] * OUT_BYTES) / (args.hbm_gbs * 1e9) * 1e3, 4)}

    def stats(ts):
        ms = [round(1e3 * x, 3) for x in ts]
        return {"ms": ms, "median_min_max_ms": [round(float(np.median(ms)), 3), min(ms), max(ms)]}

    out = {"scans": args.scans, "rounds": args.rounds, "box_m": args.box_m,
           "library": os.environ.get("TSDF_HIP_LIB", "default"), "maps": {}}

    if args.ab:
        from tsdf_map import load_hip_library
        probe = getattr(load_hip_library(), "tsdf_frontier_ab_variant", None)
        assert probe is not None, "--ab needs a -DTSDF_FRONTIER_AB=1 build (TSDF_HIP_LIB)"
        for name, k in VARIANTS.items():
            os.environ["TSDF_FRONTIER_VARIANT"] = str(k)
            assert probe() == k, name

    for carve in (False, True):
        v, t_build = build(carve)
        lo, hi = box_of(v)
        m = {"bricks": v.num_bricks(), "build_s": round(t_build, 3), "box_lo": lo.tolist(),
             "box_hi": hi.tolist(), "legs": {}}
        for conn in (6, 26):
            st_box = v.frontier_counts(lo, hi, VS, 0.0, conn, 1)
            st_map = v.frontier_counts(None, None, VS, 0.0, conn, 1)
            buf = buffers(max(st_box["n_voxels"], st_map["n_voxels"], 1))
            cases = {"box": (lo, hi, st_box), "map": (None, None, st_map)}
            if args.ab:
                want = {}
                for name, k in VARIANTS.items():  # the same bits from every variant
                    os.environ["TSDF_FRONTIER_VARIANT"] = str(k)
                    for cname, (a, b, st) in cases.items():
                        assert device_call(v, a, b, conn, buf) == st, (name, cname)
                        got = [t[:st["n_voxels"]].cpu().numpy().tobytes() for t in buf]
                        assert want.setdefault(cname, got) == got, (name, cname)
                t = {(name, cname): [] for name in VARIANTS for cname in cases}
                for rnd in range(args.rounds + 1):  # round 0 warms up and is not reported
                    for cname, (a, b, st) in cases.items():
                        for name, k in VARIANTS.items():
                            os.environ["TSDF_FRONTIER_VARIANT"] = str(k)
                            dt, _ = clock(lambda: device_call(v, a, b, conn, buf))
                            if rnd:
                                t[(name, cname)].append(dt)
                for (name, cname), ts in t.items():
                    m["legs"]["%s_%s_conn%d" % (name, cname, conn)] = {
                        **stats(ts), "counts": cases[cname][2]}
                continue
            with_route = not args.skip_route and conn == 6  # (the route is timed at 6 only)
            if with_route:  # the comparison first
                ref = route(v, lo, hi, conn)
                assert device_call(v, lo, hi, conn, buf) == {**ref.counts,
                                                             "n_bricks": st_box["n_bricks"]}
                n = st_box["n_voxels"]
                fr.assert_same([t[:n].cpu().numpy() for t in buf], ref)
            t = {"device_box": [], "device_map": [], "route_box": []}
            for rnd in range(args.rounds + 1):  # round 0 warms up and is not reported
                for leg in t:
                    if leg == "route_box":
                        if not with_route or rnd > args.route_rounds:
                            continue
                        dt, _ = clock(lambda: route(v, lo, hi, conn))
                    else:
                        a, b, _ = cases[leg[7:]]
                        dt, _ = clock(lambda: device_call(v, a, b, conn, buf))
                    if rnd:
                        t[leg].append(dt)
            for leg, ts in t.items():
                if not ts:
                    continue
                st = st_map if leg == "device_map" else st_box
                e = {**stats(ts), "counts": st}
                if leg == "route_box":
                    n = np.prod((hi - lo + 2).astype(np.float64))
                    e["pcie_bytes"] = int(n * VOXEL_BYTES)
                else:
                    e["bytes"] = bytes_of(st)
                    e["pcie_bytes"] = 8 * st["n_bricks"] * 3 + 32  # keys up, counts down, offsets up
                m["legs"]["%s_conn%d" % (leg, conn)] = e
            if t["route_box"]:
                m["legs"]["route_over_device_box_conn%d" % conn] = round(
                    float(np.median(t["route_box"]) / np.median(t["device_box"])), 1)
        out["maps"]["carved" if carve else "bench"] = m
        print("carved" if carve else "bench",
              {k: e.get("median_min_max_ms") if isinstance(e, dict) else e
               for k, e in m["legs"].items()}, file=sys.stderr, flush=True)
        v.close()
    os.environ.pop("TSDF_FRONTIER_VARIANT", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
