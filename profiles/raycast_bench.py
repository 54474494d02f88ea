#!/usr/bin/env python3
"""Throughput of the raycast (include/tsdf_hip_raycast.h) on the GPU.

The map is the benchmark's C1 workload (bench.py: --scans synthetic Ouster scans at 5 cm, one
batch); the rays are the next scan's 131072 directions from its origin, resident in HBM, cast to
--t-max with step = voxel / 2 in both modes.  Reported per mode: microseconds per call and rays
per second, as a host clock around calls that each end in a device synchronise.

The yardstick is what the library could do before it had a raycast: tsdf_sample_device over the
full lattice of march points (every --emulate-every-th ray, all of its lattice samples, resident
in HBM before the clock starts; the time is scaled to all rays and the hit test on the host side
of the emulation is not counted at all).  Its hits are compared with the raycast's.

With --variant NAME=PATH (e.g. `make -C noetic-slam_amd/csrc variants
VARIANTS="raycast_noskip:-DTSDF_RAYCAST_SKIP=0"` -> lib/var/libtsdf_hip_raycast_noskip.so) the
libraries are loaded into this process, each builds the same map in a context of its own, and the
timed rounds alternate between them.  Their outputs are compared bit for bit first.  With --count
PATH (a -DTSDF_RAYCAST_COUNT=1 build) the samples a lane really evaluates are counted against the
lattice samples a full march takes.  "call_floor" is the nearest call on 64 rays: what a call
costs before the rays matter (flush, launch, synchronise).

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
    ap.add_argument("--t-max", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--emulate-every", type=int, default=17,
                    help="the parent emulation samples the lattice of every k-th ray")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB",
                    help="another libtsdf_hip.so to interleave with the shipped one (repeatable)")
    ap.add_argument("--count", default=None, metavar="LIB",
                    help="a -DTSDF_RAYCAST_COUNT=1 build: samples evaluated per ray")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raycast", "raycast_bench.json"))
    return ap.parse_args()


class Side:
    """One library, its context and map, and its output buffers."""

    def __init__(self, name, lib, args, cloud, offs, origins, dev, n):
        import torch
        from tsdf_map import _abi
        from tsdf_map.volume import TSDFVolume
        self.name = name
        self.vol = TSDFVolume(lib, args.voxel, args.trunc, max_points=1 << 17,
                              max_batch=min(args.scans, 512), semantics="vdbfusion_f64")
        v = self.vol
        org = np.ascontiguousarray(origins, np.float64)
        o = np.ascontiguousarray(offs, np.uint64)
        v._check(lib.tsdf_integrate_batch_device(v._ctx, C.c_void_p(cloud.data_ptr()),
                                                 o.ctypes.data_as(_abi.U64P), org.shape[0],
                                                 org.ctypes.data_as(_abi.D3)), "integrate")
        v.sync()
        self.depth = torch.zeros(n, dtype=torch.float32, device=dev)
        self.normal = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        self.hit = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.args = args
        torch.cuda.synchronize()

    def cast(self, o, d, n, mode):
        v, a = self.vol, self.args
        v._check(v._lib.tsdf_raycast_device(v._ctx, C.c_void_p(o), C.c_void_p(d), n, None, 0.0,
                                            a.t_max, a.voxel / 2, mode, 0.0,
                                            C.c_void_p(self.depth.data_ptr()),
                                            C.c_void_p(self.normal.data_ptr()),
                                            C.c_void_p(self.hit.data_ptr())), "raycast_device")

    def run(self, op, o, d, n):
        if op == "call_floor":
            self.cast(o, d, min(n, 64), 0)
        else:
            self.cast(o, d, n, 0 if op == "nearest" else 1)

    def outputs(self):
        return [t.cpu().numpy().view(np.uint8).copy() for t in (self.depth, self.normal, self.hit)]


def lattice_points(torch, o, d, t_max, step):
    """The march points of every ray, as the raycast forms them: p_k = o + t_k d, t_k = (float)k *
    step (t_min = 0) while t_k <= t_max, each product and sum rounded to fp32.  (rays, k, 3)."""
    n_k = int(t_max / step) + 2
    t = torch.arange(n_k, dtype=torch.float32, device=o.device) * np.float32(step)
    t = t[t <= np.float32(t_max)]
    p = t[None, :, None] * d[:, None, :]
    p += o[:, None, :]
    return p.contiguous(), int(t.shape[0])


def main():
    args = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit("raycast_bench needs a GPU: nothing is measured without one")
    from tsdf_map import load_hip_library
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    cloud, offs, origins = sim.scans(0, args.scans)
    q_t, q_org = sim.scan(args.scans)  # a fresh scan: the next pose on the circle
    org_t = torch.as_tensor(q_org, dtype=torch.float64, device=dev)
    v = q_t.to(torch.float64) - org_t
    d_t = (v / v.norm(dim=1, keepdim=True)).to(torch.float32).contiguous()
    n = int(d_t.shape[0])
    o_t = org_t.to(torch.float32).expand(n, 3).contiguous()
    torch.cuda.synchronize()
    o, d = o_t.data_ptr(), d_t.data_ptr()
    step = args.voxel / 2

    libs = [("shipped", load_hip_library())]
    for v in args.variant:
        name, path = v.split("=", 1)
        libs.append((name, load_hip_library(os.path.abspath(path))))
    sides = [Side(name, lib, args, cloud, offs, origins, dev, n) for name, lib in libs]
    ops = ("call_floor", "nearest", "trilinear")

    # outputs agree bit for bit between the libraries (and the warm-up of every shape)
    check, hits = {}, {}
    for sd in sides:
        got = {}
        for op in ops:
            for _ in range(args.warmup):
                sd.run(op, o, d, n)
            got[op] = sd.outputs()
            hits[op] = int(sd.hit.sum().item())
        check[sd.name] = got
    same = all(np.array_equal(x, y) for sd in sides[1:] for op in ops
               for x, y in zip(check[sides[0].name][op], check[sd.name][op]))
    if not same:
        sys.exit("the libraries' outputs differ: not an A/B of the same computation")

    # the parent's emulation: tsdf_sample_device over the whole lattice of a subsample of the rays
    sub = slice(0, n, args.emulate_every)
    pts, n_k = lattice_points(torch, o_t[sub], d_t[sub], args.t_max, step)
    n_sub, n_pts = int(pts.shape[0]), int(pts.shape[0] * pts.shape[1])
    es = torch.zeros(n_pts, dtype=torch.float32, device=dev)
    ew = torch.zeros(n_pts, dtype=torch.float32, device=dev)
    ev = torch.zeros(n_pts, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    vol0 = sides[0].vol

    def emulate(mode):
        vol0._check(vol0._lib.tsdf_sample_device(vol0._ctx, C.c_void_p(pts.data_ptr()), n_pts, mode,
                                                 0.0, C.c_void_p(es.data_ptr()),
                                                 C.c_void_p(ew.data_ptr()), None,
                                                 C.c_void_p(ev.data_ptr())), "sample_device")

    emu_hits_equal, first_hit_k = {}, {}
    for op, mode in (("nearest", 0), ("trilinear", 1)):
        emulate(mode)
        S, V = es.view(n_sub, n_k), ev.view(n_sub, n_k).bool()
        cross = V[:, :-1] & V[:, 1:] & (S[:, :-1] > 0) & (S[:, 1:] <= 0)
        sides[0].run(op, o, d, n)
        emu_hits_equal[op] = bool(torch.equal(cross.any(1), sides[0].hit[sub].bool()))
        # lattice samples a full march takes: up to and including the hit's second sample
        k_hit = torch.where(cross.any(1), cross.float().argmax(1) + 2,
                            torch.full((n_sub,), n_k, device=dev))
        first_hit_k[op] = float(k_hit.float().mean().item())

    us = {sd.name: {op: [] for op in ops} for sd in sides}
    emu = {"nearest": [], "trilinear": []}
    emu_reps = max(1, args.reps // 20)
    for _ in range(args.rounds):
        for op in ops:
            for sd in sides:  # alternate the libraries within every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    sd.run(op, o, d, n)
                us[sd.name][op].append((time.perf_counter() - t0) / args.reps * 1e6)
            if op in emu:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(emu_reps):
                    emulate(0 if op == "nearest" else 1)
                emu[op].append((time.perf_counter() - t0) / emu_reps * 1e6)

    res = {"workload": "C1 map: %d synthetic os1_128_1024 scans at %g m; rays: scan %d's %d "
                       "directions from its origin, t in [0, %g], step %g"
                       % (args.scans, args.voxel, args.scans, n, args.t_max, step),
           "timing": "host clock over %d calls (emulation: %d), each ending in a stream "
                     "synchronise; median [min, max] of %d interleaved rounds"
                     % (args.reps, emu_reps, args.rounds),
           "n_rays": n, "bricks": sides[0].vol.num_bricks(), "lattice_samples_per_ray": n_k,
           "hits": {op: hits[op] for op in ("nearest", "trilinear")},
           "full_march_samples_per_ray": {k: round(x, 1) for k, x in first_hit_k.items()},
           "emulation_hits_equal_raycast": emu_hits_equal,
           "outputs_bitwise_equal_across_variants": bool(same) if len(sides) > 1 else None,
           "variants": {}}
    for sd in sides:
        r = {}
        for op in ops:
            x = us[sd.name][op]
            med = statistics.median(x)
            r[op] = {"us_per_call": round(med, 2), "us_min": round(min(x), 2),
                     "us_max": round(max(x), 2)}
            if op != "call_floor":
                r[op]["mrays_per_s"] = round(n / med, 2)
        res["variants"][sd.name] = r
    res["parent_emulation"] = {
        "what": "tsdf_sample_device over all %d lattice samples of every %dth ray (%d rays, %d "
                "points resident in HBM), time scaled by %d to all rays; the host-side hit test "
                "is not counted" % (n_k, args.emulate_every, n_sub, n_pts, args.emulate_every)}
    for op, x in emu.items():
        scaled = [t * n / n_sub for t in x]
        med = statistics.median(scaled)
        ship = res["variants"][sides[0].name][op]["us_per_call"]
        res["parent_emulation"][op] = {"us_per_call_scaled": round(med, 1),
                                       "us_min": round(min(scaled), 1),
                                       "us_max": round(max(scaled), 1),
                                       "us_per_call_subsample": round(statistics.median(x), 1),
                                       "mrays_per_s": round(n / med, 3),
                                       "emulation_over_raycast": round(med / ship, 1)}

    if args.count:
        cs = Side("count", load_hip_library(os.path.abspath(args.count)), args, cloud, offs,
                  origins, dev, n)
        res["samples_per_ray"] = {}
        for op in ("nearest", "trilinear"):
            cs.run(op, o, d, n)
            nm = cs.normal.double().mean(0).cpu().numpy()
            # a wave runs as long as its busiest lane: field evaluations (march + skip probes)
            # summed over the lanes, against 64 times each wave's maximum
            ev_l = (cs.depth.double() + cs.normal[:, 0].double())[: n - n % 64].view(-1, 64)
            util = float((ev_l.sum() / (64 * ev_l.max(1).values.sum())).item())
            res["samples_per_ray"][op] = {
                "marched": round(float(cs.depth.double().mean().item()), 2),
                "skip_probes": round(float(nm[0]), 2), "table_probes": round(float(nm[1]), 2),
                "full_march": round(float(nm[2]), 2), "lattice": n_k,
                "wave_lane_utilisation": round(util, 3),
                "busiest_lane_evaluations": int(ev_l.max().item())}
        cs.vol.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for sd in sides:
        sd.vol.close()


if __name__ == "__main__":
    main()
