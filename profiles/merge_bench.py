#!/usr/bin/env python3
"""The device merge against the only route there was before it.

Source: the bench workload's map after --scans scans (bench.py's sensor, trajectory and parameters;
64 scans at 5 cm: the C1 map of §11 and §14).  It is merged under a general pose (a) into an empty
context and (b) into a copy of itself, in both modes, two ways:

  merge   tsdf_merge_transformed: candidates, flags, counts, insert, sample + fuse, all in HBM; the
          counts are the only bytes that cross PCIe
  route   what a caller had to do before: tsdf_export_bricks (the source over PCIe), the host works
          out the destination bricks the source's bricks reach and the fp32 preimages of their
          voxel centres (header rule 2, numpy), tsdf_sample on them (points up, samples down),
          tsdf_import_bricks of the bricks with a valid sample (the result up)

Before anything is timed the two results are compared bitwise (export_bricks of both
destinations).  Then both are timed in the same process, rounds alternating, with a host clock over
calls that end in a device synchronise: one warm-up round, then --rounds rounds; median [min, max].
The destination of every round is created (and, for (b), filled) outside the timed region.

Bytes are computed from the brick counts.  Kernel times are not measured here: run the script with
--rounds 1 under `rocprofv3 --kernel-trace` in a run of its own and give the trace to
--kernel-trace, which prints the merge kernels' calls and mean times.

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

F = np.float32
VS, TAU = 0.05, 0.15
BRICK_BYTES = 2 * 512 * 4  # sdf + weight
KERNELS = ("k_merge_candidates", "k_merge_flag", "k_merge_insert", "k_merge_apply", "k_sample",
           "k_import_insert", "k_import_merge", "k_fill")


def kernel_times(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            kind = next((k for k in KERNELS if k in name), None)
            if kind is None:
                continue
            if kind in ("k_merge_candidates", "k_merge_flag", "k_merge_apply", "k_sample"):
                kind += "<1>" if ("ILi1E" in name or "ILb1E" in name or "<1>" in name
                                  or "<true>" in name) else "<0>"
            e = out.setdefault(kind, {"calls": 0, "ns": 0})
            e["calls"] += 1
            e["ns"] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    for e in out.values():
        e["us_per_call"] = round(e["ns"] / 1e3 / e["calls"], 2)
    return out


def general_pose():
    w = np.deg2rad([10.0, -20.0, 30.0])
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.empty((3, 4))
    T[:, :3] = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)
    T[:, 3] = (1.234, -2.345, 0.456)
    return T


def inverse_f32(T):
    """Header rule 1."""
    Ri, t = T[:, :3].T, T[:, 3]
    m = np.empty((3, 4))
    m[:, :3] = Ri
    for r in range(3):
        m[r, 3] = -((Ri[r, 0] * t[0] + Ri[r, 1] * t[1]) + Ri[r, 2] * t[2])
    return m.astype(F)


def reached_bricks(coords, T):
    """The destination bricks the source's bricks may reach: the bounding box of each brick's
    image, a voxel wider on every side (the trilinear cube, the rounding), as unique rows."""
    c = coords.astype(np.float64) * 8
    corners = np.stack([c + 8.5 * np.array([i, j, k]) for i in (0, 1) for j in (0, 1)
                        for k in (0, 1)], 1)                      # (n, 8, 3) voxel units
    img = corners @ T[:, :3].T + T[:, 3] / float(F(VS))
    lo = np.floor((img.min(1) - 1.5) / 8).astype(np.int64)
    hi = np.floor((img.max(1) + 1.5) / 8).astype(np.int64)
    ext = int((hi - lo).max()) + 1
    r = np.arange(ext)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    b = lo[:, None, :] + off[None, :, :]
    b = b[np.all(b <= hi[:, None, :], axis=2)]
    mn = b.min(0)
    e = [int(x) for x in (b.max(0) - mn + 1)]
    k = np.unique(((b[:, 0] - mn[0]) * e[1] + (b[:, 1] - mn[1])) * e[2] + (b[:, 2] - mn[2]))
    return np.stack([k // (e[1] * e[2]), (k // e[2]) % e[1], k % e[2]], 1) + mn


LZ, LY, LX = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
LOCAL = np.stack([LX, LY, LZ], -1).reshape(512, 3)  # voxel l = z * 64 + y * 8 + x


def route(src, dst, T, mode, chunk=4096):
    """The parent's route; returns the PCIe bytes it moved."""
    coords, _, _ = src.export_bricks()                       # the source over PCIe
    pcie = BRICK_BYTES * len(coords)
    m = inverse_f32(T)
    cand = reached_bricks(coords, T)
    for i0 in range(0, len(cand), chunk):
        b = cand[i0:i0 + chunk]
        v = (b[:, None, :] * 8 + LOCAL[None, :, :]).reshape(-1, 3)
        c = ((v.astype(F) + F(0.5)).astype(F) * F(VS)).astype(F)  # rule 2
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        q = np.stack([(((m[r, 0] * x + m[r, 1] * y).astype(F) + m[r, 2] * z).astype(F)
                       + m[r, 3]).astype(F) for r in range(3)], 1)
        s, w, _, valid = src.sample(np.ascontiguousarray(q), mode=mode)
        pcie += q.nbytes + 21 * len(q)
        valid = valid.reshape(-1, 512)
        keep = valid.any(1)
        if not keep.any():
            continue
        S = np.where(valid, s.reshape(-1, 512), F(TAU))[keep]
        W = np.where(valid, w.reshape(-1, 512), F(0))[keep]
        dst.import_bricks(b[keep], S, W)
        pcie += BRICK_BYTES * int(keep.sum())
    return pcie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-bricks", type=int, default=1 << 18)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "merge", "merge_bench.json"))
    ap.add_argument("--kernel-trace", default=None, metavar="CSV",
                    help="a rocprofv3 kernel trace of an earlier run of this script: print the "
                         "merge kernels' calls and mean times, and exit")
    args = ap.parse_args()
    if args.kernel_trace:
        print(json.dumps({"kernels": kernel_times(args.kernel_trace)}))
        return

    import torch
    assert torch.cuda.is_available(), "merge_bench needs a GPU"
    from tsdf_map import HipTSDFVolume
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    steps = [sim.scans(k0, args.batch) for k0 in range(0, args.scans, args.batch)]
    torch.cuda.synchronize()
    max_pts = max(int(np.diff(o).max()) for _, o, _ in steps)

    def make():
        return HipTSDFVolume(VS, TAU, max_points=max(max_pts, 1 << 20),
                             max_bricks=args.max_bricks, max_batch=args.batch, pipeline=2)

    src = make()
    for x, offs, org in steps:
        src.integrate_batch_device(x.data_ptr(), offs, org)
    src.sync()
    own = src.export_bricks()
    nb = len(own[0])
    T = general_pose()

    def fresh(into):
        d = make()
        if into == "copy":
            d.import_bricks(*own)
        return d

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
           "pose": "rotvec (10, -20, 30) deg, t (1.234, -2.345, 0.456) m", "workloads": {}}
    for into in ("empty", "copy"):
        for mode in ("nearest", "trilinear"):
            # the comparison first
            a, b = fresh(into), fresh(into)
            st = a.merge_from(src, T, mode=mode)
            pcie = route(src, b, T, mode)
            ea, eb = a.export_bricks(), b.export_bricks()
            if not same(ea, eb):  # say where before failing
                if ea[0].shape == eb[0].shape and np.array_equal(ea[0], eb[0]):
                    ds = ea[1].view(np.uint32) != eb[1].view(np.uint32)
                    dw = ea[2].view(np.uint32) != eb[2].view(np.uint32)
                    i = np.argwhere(ds | dw)
                    print("differ: %d sdf, %d weight voxels in %d bricks; first %s: merge (%r, %r) "
                          "route (%r, %r)" % (ds.sum(), dw.sum(), len(np.unique(i[:, 0])),
                                              (ea[0][i[0][0]].tolist(), i[0][1:].tolist()),
                                              ea[1][tuple(i[0])], ea[2][tuple(i[0])],
                                              eb[1][tuple(i[0])], eb[2][tuple(i[0])]),
                          file=sys.stderr, flush=True)
                else:
                    print("brick sets differ: %d against %d" % (len(ea[0]), len(eb[0])),
                          file=sys.stderr, flush=True)
            assert same(ea, eb), (into, mode)
            a.close()
            b.close()
            t = {"merge": [], "route": []}
            for rnd in range(args.rounds + 1):  # round 0 warms both paths up and is not reported
                for leg in ("merge", "route"):
                    d = fresh(into)
                    if leg == "merge":
                        dt, _ = clock(lambda: d.merge_from(src, T, mode=mode))
                    else:
                        dt, _ = clock(lambda: route(src, d, T, mode))
                    d.close()
                    if rnd:
                        t[leg].append(dt)
            ms = {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in t.items()}
            touched, held = st["touched_bricks"], st["touched_bricks"] - st["new_bricks"]
            out["workloads"]["%s/%s" % (into, mode)] = {
                "counts": st, "bitwise_equal_to_route": True, "ms": ms,
                "median_min_max_ms": {k: [round(1e3 * med[k], 3), min(ms[k]), max(ms[k])] for k in t},
                "route_over_merge": round(med["route"] / med["merge"], 1),
                # unique bytes: flag reads the source's weights and the held candidates' weights;
                # apply reads the source's (S, W), reads the held touched bricks and writes every
                # touched brick; the route's PCIe traffic against the merge's 48 B of counts
                "bytes": {"flag_read": nb * BRICK_BYTES // 2 + held * BRICK_BYTES // 2,
                          "apply_read": nb * BRICK_BYTES + held * BRICK_BYTES,
                          "apply_write": touched * BRICK_BYTES,
                          "route_pcie": pcie, "merge_pcie": 48 + 8 + 4},
            }
            print(into, mode, out["workloads"]["%s/%s" % (into, mode)]["median_min_max_ms"],
                  file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
