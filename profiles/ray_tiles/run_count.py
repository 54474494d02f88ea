"""Runs per scan under different block shapes (DESIGN.md §5 "ray tiles", §10), on the CPU.

A run is one (workgroup, brick) pair of one scan: what k_count pays a global find-or-insert, a
cell atomic and a run record for, and k_place a run-list entry, a cell gather and a separately
aligned stretch of the copy-out.  The script places 25 positions along every ray's truncation band
(hit -tau .. +tau; the band is 6 voxels long, so 25 positions see every brick it crosses up to
corner clips), and counts the distinct (unit, brick) pairs of a scan, where a unit is a k_count
block or a k_place half under the given layout:

    columns x beams of the unit; "8 x 128" and "4 x 128" are today's consecutive 1024 and 512 rays

Usage:  python3 profiles/ray_tiles/run_count.py [--scans 0 300 700] [--drop 0.01]
--drop removes that fraction of each scan's points at random first (the units are then formed by
index, as the kernels would form them if they tiled such a scan).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "noetic-slam_amd"))

VS, TAU, H = 0.05, 0.15, 128


def brick_ids(pts, org):
    d = pts.astype(np.float64) - org
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    s = np.linspace(-TAU, TAU, 25)
    pos = pts[:, None, :].astype(np.float64) + s[None, :, None] * u[:, None, :]
    b = np.floor(pos / (8 * VS)).astype(np.int64) + (1 << 20)
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]  # (n, 25)


def unit_of(n, cols, beams):
    """Unit index of every point under a cols x beams layout of an H-beam column-major scan."""
    i = np.arange(n)
    c, b = i // H, i % H
    return (c // cols) * (H // beams) + b // beams


def runs(bricks, unit):
    key = np.stack([np.broadcast_to(unit[:, None], bricks.shape).ravel(), bricks.ravel()], 1)
    return np.unique(key, axis=0).shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, nargs="+", default=[0, 300, 700])
    ap.add_argument("--drop", type=float, default=0.0)
    a = ap.parse_args()
    from tsdf_map.scan_gen import OusterSim
    sim = OusterSim()
    layouts = [("k_count block", 8, 128), ("k_count block", 32, 32), ("k_count block", 64, 16),
               ("k_count 2048", 16, 128),
               ("k_place half", 4, 128), ("k_place half", 16, 32), ("k_place half", 32, 16)]
    tot = {l: 0 for l in layouts}
    rng = np.random.default_rng(1)
    for k in a.scans:
        pts, org = sim.scan(k)
        if a.drop > 0:
            pts = pts[rng.random(pts.shape[0]) >= a.drop]
        br = brick_ids(pts, org)
        for l in layouts:
            tot[l] += runs(br, unit_of(pts.shape[0], l[1], l[2]))
    print("scans %s, drop %g: runs per scan" % (a.scans, a.drop))
    for l in layouts:
        print("  %-14s %3d x %3d  %8.1f k" % (l[0], l[1], l[2], tot[l] / len(a.scans) / 1e3))


if __name__ == "__main__":
    main()
