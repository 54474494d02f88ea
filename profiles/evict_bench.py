#!/usr/bin/env python3
"""Eviction against the only route there was before it.

The bench workload's map after --scans scans (bench.py's sensor, trajectory and parameters), cut at
the median brick x into two halves.  Every leg drops one half, and the legs take the halves in
turn: a re-imported half lies at the pool's tail, so dropping the same half again would remove the
tail only and move nothing, while dropping the other half empties the pool's head and moves every
kept brick -- the most a removal can move.  Timed with a host clock around calls that end in a
device synchronise, --reps times each, alternating:

  evict+copy   evict_outside(lo, hi): the dropped half gathered on the GPU and copied to the host
  evict        evict_outside(lo, hi, copy_out=False)
  baseline     export_bricks(), destroy, create, import_bricks(kept): the whole map over PCIe once
               and the kept half once more, plus a context's allocation and fills

After each leg the map is put back (import_bricks of the dropped half into absent bricks is a
plain copy), so every leg starts from the same field.

Bytes are computed from the brick counts.  Kernel times are not measured here: run the script
under `rocprofv3 --kernel-trace` in a run of its own and give the trace to --kernel-trace, which
prints the removal kernels' times, and k_rm_gather's and k_rm_move's rates (their bricks from
the launch's grid).

One JSON line at the end.  No GPU: the script fails.
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

BRICK_BYTES = 2 * 512 * 4  # sdf + weight


def kernel_rates(path):
    """The removal's kernels in a rocprofv3 kernel trace: calls and mean time per kernel, and for
    k_rm_gather / k_rm_move the rate.  Those two run a wave per brick: a launch of g work-items
    handles g / 64 bricks (the last workgroup may be short of up to 3), and reads and writes both
    arrays of each."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            kind = next((k for k in ("k_rm_flag_box", "k_rm_sum", "k_rm_scan", "k_rm_apply",
                                     "k_rm_gather", "k_rm_move", "k_rehash", "k_fill")
                         if k in name), None)
            if kind is None:
                continue
            e = out.setdefault(kind, {"calls": 0, "ns": 0, "bytes": 0})
            e["calls"] += 1
            e["ns"] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            if kind in ("k_rm_gather", "k_rm_move"):
                e["bytes"] += 2 * BRICK_BYTES * (int(row["Grid_Size_X"]) // 64)
    for e in out.values():
        e["us_per_call"] = round(e["ns"] / 1e3 / e["calls"], 2)
        e["GB_per_s"] = round(e["bytes"] / e["ns"], 1) if e["bytes"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=128)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-bricks", type=int, default=1 << 20)
    ap.add_argument("--kernel-trace", default=None, metavar="CSV",
                    help="a rocprofv3 kernel trace of an earlier run of this script: print the "
                         "removal kernels' times and rates, and exit")
    args = ap.parse_args()
    if args.kernel_trace:
        print(json.dumps({"kernels": kernel_rates(args.kernel_trace)}))
        return

    import torch
    assert torch.cuda.is_available(), "evict_bench needs a GPU"
    from tsdf_map import HipTSDFVolume
    from tsdf_map.scan_gen import TorchOusterSim
    dev = torch.device("cuda", 0)
    sim = TorchOusterSim(dev)
    steps = [sim.scans(k0, args.batch) for k0 in range(0, args.scans, args.batch)]
    torch.cuda.synchronize()
    max_pts = max(int(np.diff(o).max()) for _, o, _ in steps)

    def make():
        return HipTSDFVolume(0.05, 0.15, max_points=max(max_pts, 1 << 17),
                             max_bricks=args.max_bricks, max_batch=args.batch, pipeline=2)

    vol = make()
    for x, offs, org in steps:
        vol.integrate_batch_device(x.data_ptr(), offs, org)
    vol.sync()
    coords, sdf, w = vol.export_bricks()
    nb = len(coords)
    lo = coords.min(0).astype(np.int64)
    hi = coords.max(0).astype(np.int64) + 1
    med = int(np.median(coords[:, 0]))
    boxes = [(lo, np.array([med, hi[1], hi[2]])), (np.array([med, lo[1], lo[2]]), hi)]
    inside = [np.all((coords >= a) & (coords < b), axis=1) for a, b in boxes]
    assert np.array_equal(inside[0], ~inside[1])
    # leg with box h keeps half h and drops the other one
    dropped = [(coords[~m], sdf[~m], w[~m]) for m in inside]
    n_drop = [int((~m).sum()) for m in inside]
    assert all(vol.count_outside(*boxes[h]) == n_drop[h] for h in (0, 1))

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def baseline(h):
        nonlocal vol
        c, s, ww = vol.export_bricks()
        k = np.all((c >= boxes[h][0]) & (c < boxes[h][1]), axis=1)
        vol.close()
        vol = make()
        vol.import_bricks(c[k], s[k], ww[k])

    t = {"evict_copy": [], "evict": [], "baseline": [], "restore_import": []}
    turn = 0
    for rep in range(args.reps + 1):  # rep 0 warms every path up and is not reported
        for leg in ("evict_copy", "evict", "baseline"):
            h = turn & 1
            turn += 1
            if leg == "evict_copy":
                dt, ev = clock(lambda: vol.evict_outside(*boxes[h]))
                assert np.array_equal(ev[0], dropped[h][0])
                assert np.array_equal(ev[1].view(np.uint32), dropped[h][1].view(np.uint32))
            elif leg == "evict":
                dt, n = clock(lambda: vol.evict_outside(*boxes[h], copy_out=False))
                assert n == n_drop[h]
            else:
                dt, _ = clock(lambda: baseline(h))
            assert vol.num_bricks() == nb - n_drop[h]
            dr, _ = clock(lambda: vol.import_bricks(*dropped[h]))
            assert vol.num_bricks() == nb
            if rep:
                t[leg].append(dt)
                t["restore_import"].append(dr)
    # the field is what it was (slot order aside)
    c2, s2, w2 = vol.export_bricks()
    assert np.array_equal(c2, coords) and np.array_equal(w2, w)
    assert np.array_equal(s2.view(np.uint32), sdf.view(np.uint32))
    n_ev = max(n_drop)

    ms = {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}
    best = {k: min(v) for k, v in t.items()}
    out = {
        "scans": args.scans, "bricks": nb, "evicted": n_ev, "kept": nb - n_ev,
        "max_bricks": args.max_bricks, "reps": args.reps, "ms": ms,
        "best_ms": {k: round(1e3 * v, 3) for k, v in best.items()},
        # bytes: the copy-out gathers the evicted bricks (read + write on the GPU) and carries them
        # over PCIe once; the move reads and writes min(kept, evicted) bricks when the evicted
        # ones fill the pool's head; the baseline carries the whole map out and the kept bricks back
        "bytes": {"gather_device": 2 * BRICK_BYTES * n_ev, "evict_copy_pcie": BRICK_BYTES * n_ev,
                  "baseline_pcie": BRICK_BYTES * (nb + nb - n_ev),
                  "move_device": 2 * BRICK_BYTES * min(n_ev, nb - n_ev)},
        "evict_copy_pcie_GB_per_s": round(BRICK_BYTES * n_ev / best["evict_copy"] / 1e9, 2),
        "baseline_over_evict_copy": round(best["baseline"] / best["evict_copy"], 2),
        "baseline_over_evict": round(best["baseline"] / best["evict"], 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
