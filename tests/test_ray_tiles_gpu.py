"""Ray tiles on the GPU (noetic-slam_amd/csrc/ray_tile.h): k_count and k_place walk a
column-regular scan in 32 x 32 tiles of (column, beam) instead of 1024 consecutive points.  The
field cannot change: every case is compared bit for bit (voxel set, W bits, S bits) with the CPU
oracle and with a context created under TSDF_RAY_TILES=0, and the metrics log's `tiled_scans` says
that the tiles were in fact on (and off) where the case means them to be.

Scans are small grids of the synthetic sensor (128 beams x W columns, or every second beam: 64 x W),
so a case takes a fraction of a second; each runs with the 1024-lane k_count of small batches and,
under TSDF_COUNT_WIDE=0, with the 256-lane k_count of the bench's batches.
"""
import json

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

VS, TAU = 0.05, 0.15
_SIMS = {}


def grid_scan(h, w, k):
    """Scan k of a sensor of h beams (128, or 64: every second beam) x w columns, column-major."""
    from tsdf_map.scan_gen import OusterSim
    if w not in _SIMS:
        _SIMS[w] = OusterSim(columns=w)
    pts, org = _SIMS[w].scan(k)
    assert pts.shape[0] == 128 * w  # every ray of the scene returns: intact columns
    if h == 64:
        pts = np.ascontiguousarray(pts.reshape(w, 128, 3)[:, ::2].reshape(-1, 3))
    return pts, org


def run_gpu(scans, log, monkeypatch, tiles=None, wide=True, **kw):
    """The scans through a fresh context (host queue: max_batch scans per GPU batch); returns the
    exported field and the committed batches' tiled_scans."""
    from tsdf_map import HipTSDFVolume
    for name, val in (("TSDF_RAY_TILES", tiles), ("TSDF_COUNT_WIDE", None if wide else "0")):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    kw.setdefault("max_bricks", 1 << 15)
    kw.setdefault("max_points", 1 << 14)
    g = HipTSDFVolume(VS, TAU, **kw)
    g.set_metrics_log(log)
    for p, org in scans:
        g.integrate(p, org)
    g.sync()
    out = g.export_voxels()
    g.set_metrics_log(None)
    g.close()
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    return out, [r["tiled_scans"] for r in recs if r["committed"]]


def run_oracle(scans, **kw):
    for drop in ("max_batch", "pipeline", "max_bricks"):
        kw.pop(drop, None)
    o = oracle.OracleTSDFVolume(VS, TAU, **kw)
    for p, org in scans:
        o.integrate(p, org)
    return o.export_voxels()


def assert_same_field(got, ref, what):
    gi, gs, gw = got
    ri, rs, rw = ref
    assert gi.shape == ri.shape and np.array_equal(gi, ri), what
    assert np.array_equal(gw.view(np.uint32), rw.view(np.uint32)), what
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), what


def check(scans, tiled, tmp_path, monkeypatch, **kw):
    """Tiles on (auto) and off, wide and narrow k_count, against the oracle; `tiled`: the tiled
    scans of each GPU batch with tiles on."""
    ref = run_oracle(scans, **kw)
    assert ref[0].shape[0] > 1000
    for wide in (True, False):
        on, n_on = run_gpu(scans, tmp_path / ("on%d.jsonl" % wide), monkeypatch, wide=wide, **kw)
        off, n_off = run_gpu(scans, tmp_path / ("off%d.jsonl" % wide), monkeypatch, tiles="0",
                             wide=wide, **kw)
        assert n_on == tiled and n_off == [0] * len(tiled), (wide, n_on, n_off)
        assert_same_field(on, ref, "tiles on vs oracle (wide %d)" % wide)
        assert_same_field(off, ref, "tiles off vs oracle (wide %d)" % wide)
        assert_same_field(on, off, "tiles on vs off (wide %d)" % wide)


def test_one_group_four_blocks(tmp_path, monkeypatch):
    """128 beams x 32 columns: one group, its four blocks 32 x 32 tiles."""
    check([grid_scan(128, 32, 0)], [1], tmp_path, monkeypatch, max_batch=1)


def test_two_groups_of_64_beams(tmp_path, monkeypatch):
    """64 beams x 64 columns: two groups of two blocks."""
    check([grid_scan(64, 64, 3)], [1], tmp_path, monkeypatch, max_batch=1)


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "vdbfusion", "voxblox"])
def test_group_and_remainder(tmp_path, monkeypatch, semantics):
    """128 x 40: one group plus a 1024-point remainder of consecutive rays, in every semantics."""
    check([grid_scan(128, 40, 1)], [1], tmp_path, monkeypatch, max_batch=1, semantics=semantics)


def test_mixed_batch(tmp_path, monkeypatch):
    """One batch of a regular scan, the same sensor with a point removed (not a grid: consecutive
    blocks) and a second regular one."""
    a, b, c = grid_scan(128, 40, 0), grid_scan(128, 40, 1), grid_scan(64, 64, 2)
    b = (np.ascontiguousarray(np.delete(b[0], 777, axis=0)), b[1])
    check([a, b, c], [2], tmp_path, monkeypatch, max_batch=3)


def test_two_pipelined_batches(tmp_path, monkeypatch):
    """Two batches of two scans under pipeline 2: the second batch's detection runs ahead of its
    wait on the first."""
    scans = [grid_scan(128, 40, k) for k in range(4)]
    check(scans, [2, 2], tmp_path, monkeypatch, max_batch=2, pipeline=2)


def test_carving_context(tmp_path, monkeypatch):
    """Space carving (long rays: the per-pair walk of k_count and k_place, fallback pairs)."""
    check([grid_scan(128, 32, 0), grid_scan(128, 32, 5)], [2], tmp_path, monkeypatch, max_batch=2,
          space_carving=True, max_range=20.0, max_bricks=1 << 17)


def test_forced_height_on_any_cloud(tmp_path, monkeypatch, scan0):
    """TSDF_RAY_TILES=64 tiles every scan, column-regular or not: the map is a bijection for any
    point count, so the field is the oracle's all the same."""
    pts, org = scan0
    scans = [(np.ascontiguousarray(pts[5:9000:2]), org)]  # 4498 points: two groups and a remainder
    ref = run_oracle(scans)
    got, n = run_gpu(scans, tmp_path / "f.jsonl", monkeypatch, tiles="64", max_batch=1)
    assert n == [1]
    assert_same_field(got, ref, "forced tiles vs oracle")
