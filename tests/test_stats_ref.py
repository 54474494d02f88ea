"""The counter reference alone (tests/statsref.py): its two routes agree, it equals
the oracle's own counters, it gives the answers worked out by hand, and every input of
tests/test_stats_gpu.py is non-vacuous.  CPU only."""
import numpy as np
import pytest

import statsref as S

VS, TAU = S.VS, S.TAU
BATCHINGS = {"seq11": (1, 3, 9), "seq70": (64,), "seq6": (1, 2, 3, 4), "seq3": (3,)}


@pytest.mark.parametrize("semantics", S.SEMANTICS)
@pytest.mark.parametrize("name", sorted(BATCHINGS))
def test_routes_agree_and_inputs_are_nonvacuous(sim, name, semantics):
    """Routes A and B: the same points, rays and voxel sets per scan, hence the same U_vox, dirty,
    active and new for every batching the GPU tests use; route A's U_vox is the oracle's own
    n_voxels_last.  The inputs keep the counters apart (assert_nonvacuous)."""
    A = S.refs_oracle(sim, name, **S.sem_kw(semantics))
    B = S.refs_numpy(sim, name, semantics)
    assert len(A) == len(B) == len(S.INPUTS[name][0])
    for a, b in zip(A, B):
        assert (a.points, a.rays) == (b.points, b.rays)
        assert np.array_equal(a.vox, b.vox)
        assert a.u_vox == a.oracle_vox > 0
    for mb in BATCHINGS[name]:
        part = S.partition_of(len(A), mb)
        ra, held_a = S.batch_refs(A, part)
        rb, held_b = S.batch_refs(B, part)
        assert np.array_equal(held_a, held_b)
        for x, y in zip(ra, rb):
            assert {k: v for k, v in x.items() if k != "pairs"} == \
                {k: v for k, v in y.items() if k != "pairs"}
        S.assert_nonvacuous(B, part, rb)
        if len(part) > 1:  # *_last must tell the last batch from the others
            if part[-1] < part[0]:  # a short last batch is not the largest one
                assert rb[-1]["voxel_updates"] < max(r["voxel_updates"] for r in rb[:-1])
            assert rb[-1]["voxel_updates"] != rb[0]["voxel_updates"]


@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_cumulative_vox_is_the_oracles_total(sim, semantics):
    """One oracle volume fed the whole sequence: n_voxels_last per scan and n_voxels_total are route
    A's U_vox and their running sum; its brick count is the reference's."""
    kw = S.sem_kw(semantics)
    refs = S.refs_oracle(sim, "seq6", **kw)
    o = S.oracle_volume(**kw)
    total = 0
    for (p, org), r in zip(S.scans_of(sim, "seq6"), refs):
        o.integrate(p, org)
        st = o.stats()
        total += r.u_vox
        assert st["n_voxels_last"] == r.u_vox and st["n_voxels_total"] == total
    recs, held = S.batch_refs(refs, [1] * len(refs))
    assert o.num_bricks() == recs[-1]["bricks"] == held.shape[0]
    assert np.array_equal(np.sort(S.bkey(o.brick_coords())), held)
    assert S.totals(recs)["n_rays_total"] == o.stats()["n_rays_total"]


@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_per_ray_oracle_pairs_equal_numpy_pairs(sim, semantics):
    """Where both apply (no carving, no range limits) the one-ray-at-a-time oracle route and route
    B give every ray the same number of bricks."""
    p, org = S.scans_of(sim, "seq3")[1]
    p = np.ascontiguousarray(p[7::14])  # 293 rays
    a = S.pairs_per_ray_oracle(p, org, **S.sem_kw(semantics))
    b = S.pairs_per_ray_numpy(p, org, semantics)
    assert np.array_equal(a, b)
    assert a.min() >= 1 and a.max() >= 3 and a.sum() > a.shape[0]
    assert S.scan_ref_numpy(p, org, semantics).pairs == a.sum()


@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_axis_ray_across_a_brick_face(semantics):
    """By hand: a ray along +x from (-1, y, z) to x = 0.43 m.  Its band [0.28, 0.58] m is walked
    through the voxels 5..11 on x (5 cm voxels; 0.28 / 0.05 = 5.6, 0.58 / 0.05 = 11.6).  The gate
    keeps a voxel whose centre lies less than tau behind the hit: voxel 11's centre, 0.575 m, is
    0.145 m behind it (kept; Voxblox's dropoff weight there is 0.005 / 0.1 = 0.05 >= 2^-16), and
    voxel 5's, 0.275 m, is in front.  Seven voxels, 5..7 in brick 0 and 8..11 in brick 1: 2 pairs.
    (A hit at 0.41 m would walk voxel 11 too, 0.165 m behind the hit, and the gate would drop it.)"""
    y = z = np.float32(0.126)  # voxel 2 on both axes, off every voxel face
    p = np.array([[0.43, y, z]], np.float32)
    org = np.array([-1.0, float(y), float(z)])
    want = S.vkey(np.array([[i, 2, 2] for i in range(5, 12)]))
    b = S.scan_ref_numpy(p, org, semantics)
    a = S.scan_ref_oracle(p, org, **S.sem_kw(semantics))
    for r in (a, b):
        assert np.array_equal(r.vox, np.sort(want)) and (r.points, r.rays, r.u_vox) == (1, 1, 7)
    assert b.pairs == 2
    assert S.pairs_per_ray_oracle(p, org, **S.sem_kw(semantics)).tolist() == [2]
    rec, _ = S.batch_refs([b], [1])
    assert rec[0] == dict(scans=1, points=1, rays=1, pairs=2, voxel_updates=7, dirty_voxels=7,
                          active_bricks=2, new_bricks=2, bricks=2, algorithmic_bytes=12 + 16 * 7)


@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_identical_scans_double_vox_not_dirty(sim, semantics):
    p, org = S.scans_of(sim, "seq3")[0]
    r = S.scan_ref_numpy(p, org, semantics)
    one, _ = S.batch_refs([r], [1])
    two, _ = S.batch_refs([r, r], [2])
    assert two[0]["voxel_updates"] == 2 * one[0]["voxel_updates"]
    assert two[0]["rays"] == 2 * one[0]["rays"] and two[0]["pairs"] == 2 * one[0]["pairs"]
    for k in ("dirty_voxels", "active_bricks", "new_bricks", "bricks"):
        assert two[0][k] == one[0][k]


@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_range_filtered_ray_counts_nowhere(semantics):
    """A ray shorter than min_range or longer than max_range: no ray, no voxel, no brick (Voxblox
    without allow_clear: with it a long ray would become a clearing ray)."""
    org = np.zeros(3)
    p = np.array([[0.3, 0.01, 0.02], [30.0, 0.5, 0.2], [4.0, 0.3, 0.1]], np.float32)
    kw = dict(min_range=1.0, max_range=20.0, allow_clear=False, **S.sem_kw(semantics))
    for i in (0, 1):
        r = S.scan_ref_oracle(p[i:i + 1], org, **kw)
        assert (r.points, r.rays, r.u_vox) == (1, 0, 0)
        assert S.pairs_per_ray_oracle(p[i:i + 1], org, **kw).tolist() == [0]
    allr = S.scan_ref_oracle(p, org, **kw)
    kept = S.scan_ref_oracle(p[2:], org, **kw)
    assert (allr.points, allr.rays) == (3, 1) and np.array_equal(allr.vox, kept.vox)
    assert kept.u_vox > 0
    rec, _ = S.batch_refs([S.scan_ref_oracle(p[:2], org, **kw)], [1])
    assert rec[0]["rays"] == rec[0]["voxel_updates"] == rec[0]["active_bricks"] == 0


def test_variant_inputs_are_nonvacuous(sim):
    """The inputs of the GPU file that lie outside route B: Voxblox 1/z^2 weights, merged bundles,
    clearing rays, carving and sector shards, through route A."""
    pose = lambda o: np.concatenate([o, [0.0, 0.0, 0.0, 1.0]])  # noqa: E731
    scans = S.scans_of(sim, "seq3")
    for kw in (dict(semantics="voxblox"), dict(semantics="voxblox", method="merged"),
               dict(semantics="voxblox", use_const_weight=True, max_range=12.0)):
        refs = [S.scan_ref_oracle(p, pose(o), **kw) for p, o in scans]
        assert all(r.u_vox == r.oracle_vox for r in refs)  # vox as the oracle's stats count it
        recs, _ = S.batch_refs(refs, [3])
        S.assert_nonvacuous(refs, [3], recs)
        if kw.get("method") == "merged":  # bundles: fewer rays than points
            assert all(r.rays < r.points for r in refs)
        if "max_range" in kw:  # clearing rays and hits: no ray is dropped
            far = sum(int(np.count_nonzero(np.linalg.norm(p - o.astype(np.float32), axis=1) > 12.0))
                      for p, o in scans)
            assert 1000 < far < recs[0]["rays"] - 1000 and recs[0]["rays"] == recs[0]["points"]
    for sem in ("vdbfusion_f64", "vdbfusion"):
        carve = S.carve_kw(sem)
        refs = S.refs_oracle(sim, "carve16", **carve)
        band = S.refs_oracle(sim, "carve16", semantics=sem, max_range=20.0)
        recs, _ = S.batch_refs(refs, [16])
        S.assert_nonvacuous(refs, [16], recs)
        assert all(c.u_vox > 4 * b.u_vox and c.rays == b.rays for c, b in zip(refs, band))
    for rule, name in [(r, n) for r in ("world", "index") for n in ("seq3", "seq6")]:
        n = len(S.INPUTS[name][0])
        full = S.refs_oracle(sim, name, semantics="vdbfusion_f64")
        shard = [S.refs_oracle(sim, name, semantics="vdbfusion_f64", n_sectors=4, sector=k,
                               sector_rule=rule) for k in range(4)]
        for s in shard:
            S.assert_nonvacuous(s, [n], S.batch_refs(s, [n])[0], shards=name == "seq6")
        recs = [S.batch_refs(s, [n])[0][0] for s in shard]
        whole = S.batch_refs(full, [n])[0][0]
        assert sum(r["rays"] for r in recs) == whole["rays"]
        assert all(r["rays"] > 0 and r["active_bricks"] >= 64 for r in recs)
        # a scan's U_vox adds up over the shards unless two shards' rays sample one voxel
        vox = sum(r["voxel_updates"] for r in recs)
        assert vox == whole["voxel_updates"] if name == "seq3" else vox > whole["voxel_updates"]
        # border voxels and bricks are counted by two shards
        assert sum(r["dirty_voxels"] for r in recs) > whole["dirty_voxels"]
        assert sum(r["active_bricks"] for r in recs) > whole["active_bricks"]


@pytest.mark.parametrize("case", ["clear", "carve-vdbfusion_f64", "carve-vdbfusion"])
def test_few_ray_inputs_are_nonvacuous(sim, case):
    """The inputs whose pairs come from the oracle one ray at a time (at most 300 rays)."""
    if case == "clear":
        (name, step), kw = S.CLEAR_FEW, S.CLEAR_KW
    else:
        (name, step), kw = S.CARVE_FEW, S.carve_kw(case.split("-")[1])
    scans, refs = S.refs_few_rays(sim, name, step, **kw)
    S.assert_few_rays_nonvacuous(scans, refs, kw)


def test_an_empty_scan_counts_nothing(sim):
    """A batch of empty scans between two real ones: nothing counted, the pool as it was."""
    refs = S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    a = S.scan_ref_oracle(np.zeros((0, 3), np.float32), np.zeros(3))
    e = S.empty_ref()
    assert (a.points, a.rays, a.u_vox, a.oracle_vox) == (e.points, e.rays, e.u_vox, e.oracle_vox)
    recs, _ = S.batch_refs([refs[0], e, e, refs[1]], [1, 2, 1])
    assert recs[1]["bricks"] == recs[0]["bricks"] > 0
    assert all(recs[1][k] == 0 for k in ("points", "rays", "pairs", "voxel_updates",
                                         "dirty_voxels", "active_bricks", "new_bricks"))
    assert 0 < recs[2]["new_bricks"] < recs[2]["active_bricks"]


@pytest.mark.parametrize("semantics", ["vdbfusion", "vdbfusion_f64", "voxblox"])
def test_dense_brick_has_every_voxel_in_every_scan(semantics):
    pts, org, want = S.dense_brick_scan()
    r = S.scan_ref_oracle(pts, org, **S.sem_kw(semantics))
    assert pts.shape[0] == 512 and r.rays == 512
    assert np.isin(want, r.vox).all()  # all 512 voxels of the brick are sampled
    assert np.array_equal(np.unique(S.brick_of(want)), np.unique(S.brick_of(want))[:1])
    b = S.scan_ref_numpy(pts, org, semantics)
    assert np.array_equal(b.vox, r.vox)
