"""The inputs of tests/pastcap.py do what the GPU tests need of them, shown on the numpy and oracle
references alone: each is larger than its kernel's grid cap, and the region that the later trips
handle -- by the restated index arithmetic -- holds enough of every kind of work for a wrong
second trip to show in a bitwise comparison.  The counts are printed (pytest -s)."""
import numpy as np
import pytest

import meshref
import mergeref as mr
import oracle
import pastcap as pc
import rayref as rr
import sampleref as sr

F = np.float32


# ---- the indexed mesh ---------------------------------------------------------------------------

MESH_CASES = [("full", "generated", 0.0, False), ("holed", "lorensen", 0.75, False),
              ("full", "generated", 0.0, True)]


@pytest.mark.parametrize("kind,tname,min_weight,boxed", MESH_CASES)
def test_mesh_reference_has_work_either_side_of_the_cap(kind, tname, min_weight, boxed):
    ref, sides = pc.mesh_case(kind, tname, min_weight, boxed)
    print("mesh %s %s min_weight %g %s: %s" % (kind, tname, min_weight,
                                               "box" if boxed else "whole", sides))
    pc.assert_mesh_past_cap(sides)
    if not boxed:
        assert sides["n_bricks"] == 18 ** 3 and sides["brick_at_cap"] == (1, 2, 3)
    if (kind, boxed) == ("full", False):
        assert (sides["n_vertices"], sides["n_triangles"]) == (52546, 105088)


def test_mesh_box_cuts_bricks_and_lists_more_than_the_cap():
    lo, hi = pc.MESH_BOX
    assert np.all(lo % 8 != 0) and np.all(hi % 8 != 0)
    c = pc.mesh_map("full")[0]
    listed = pc.mesh_listed(c, lo, hi)
    assert pc.MESH_CAP < listed.shape[0] < c.shape[0]
    # a cube of the reference in the box's last layer of voxels, none beyond it
    info = {}
    meshref.indexed_mesh_ref(*meshref.dense_from_bricks(*pc.mesh_map("full")), pc.MESH_VS,
                             pc.mc_table("generated"), lo=lo, hi=hi, info=info)
    z = info["edges"][:, 2]
    assert (z == hi[2] - 1).sum() >= 100 and z.max() == hi[2]  # (a cube's far corners: + 1)


def test_large_sphere_deindexed_is_the_oracles_soup():
    """The reference on the large sphere, de-indexed, against the oracle's own marching cubes."""
    b = pc.mesh_map("full")
    o = oracle.OracleTSDFVolume(pc.MESH_VS, 3 * pc.MESH_VS)
    o.import_bricks(*b)
    soup, _ = o.extract_triangle_mesh()
    (v, _, t), _ = pc.mesh_case("full", "generated", 0.0, False)
    got = meshref.deindex(v, t)
    assert got.shape == soup.shape and np.array_equal(got.view(np.uint32), soup.view(np.uint32))


def test_big_sphere_has_vertices_past_the_vcount_trip():
    sides = pc.mesh_big_sides()
    print("mesh 26^3: %s" % sides)
    assert sides["n_bricks"] == 26 ** 3
    pc.assert_mesh_vcount_past_cap(sides)


# ---- the distance field -------------------------------------------------------------------------

def test_esdf_tile_mapping_on_known_voxels():
    """The restated tile -> voxel mapping at the places esdf_plan.h's formulas put the cap."""
    tile, tiles = pc.esdf_tile_of("classify", (725, 725, 5), 12)
    assert tiles == 10267
    assert tile[3, 717, 451] == 8191 and tile[3, 717, 452] == 8192  # linear index 2 097 152
    tile, tiles = pc.esdf_tile_of("z", (725, 725, 5), 12)
    assert tiles == 8213 and (tile[:, 723, 112] == 8191).all() and (tile[:, 723, 113] == 8192).all()
    tile, tiles = pc.esdf_tile_of("x", (5, 364, 364), 4)
    assert tiles == 8281 and (tile[360, 31] == 8191).all() and (tile[360, 32] == 8192).all()
    tile, tiles = pc.esdf_tile_of("y", (3, 33, 4100), 12)
    assert tiles == 8200 and (tile[4095, 32] == 8191).all() and (tile[4096, 0] == 8192).all()
    # a box with more than one tile along every index, against the plan's counts
    for r, seg in ((12, 32), (49, 64)):
        n = (130, 70, 67)
        want = {"classify": -(-130 * 70 * 67 // 256), "x": 3 * -(-70 * 67 // 16),
                "y": 3 * -(-70 // seg) * 67, "z": -(-130 * 70 // 64) * -(-67 // seg)}
        for kernel, cnt in want.items():
            tile, tiles = pc.esdf_tile_of(kernel, n, r)
            assert tiles == cnt and np.unique(tile).size == cnt, (kernel, r)


@pytest.mark.parametrize("name", list(pc.ESDF_BOXES))
def test_esdf_reference_has_work_either_side_of_the_cap(name):
    voxels, lo, hi, radius, (S, W), ref = pc.esdf_case(name)
    sides = pc.esdf_sides(name)
    print("esdf %s %s R %d: %d seeded voxels" % (name, tuple((hi - lo).tolist()), radius,
                                                 len(voxels)))
    for kernel, d in sides.items():
        print("  %-8s %s" % (kernel, d))
    pc.assert_esdf_past_cap(name, sides)
    assert len(voxels) == int((W > 0).sum())
    bricks = {(x >> 3, y >> 3, z >> 3) for x, y, z in voxels}
    assert len(bricks) < 1 << 12  # fits the GPU test's volume


# ---- the raycast --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scan0_map(scan0):
    """The oracle's scan-0 map (the merge tests' source): (export_bricks, export_voxels)."""
    v = oracle.OracleTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, semantics="vdbfusion_f64")
    v.integrate(*scan0)
    return v.export_bricks(), v.export_voxels()


def test_rays_past_the_cap_hit_and_miss(sim):
    scans = [sim.scan(k) for k in range(rr.N_SCANS)]
    v = oracle.OracleTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, semantics="vdbfusion_f64")
    for pts, org in scans:
        v.integrate(pts, org)
    refs = pc.ray_references(sr.field_of(v), scans[0])
    idx, rot = pc.ray_tiling(refs)
    sides = pc.ray_sides(refs, idx)
    print("raycast: rotation %d, %s" % (rot, sides))
    pc.assert_rays_past_cap(sides)
    assert idx.size == pc.RAY_N == 8192 * 256 + 77 and rr.lattice(*pc.RAY_T).size <= 64
    # a lane one stride back holds another ray
    assert np.all(idx[pc.RAY_STRIDE:] != idx[:pc.RAY_N - pc.RAY_STRIDE])
    o, d = pc.ray_distinct(scans[0])
    assert np.unique(np.concatenate([o, d], 1), axis=0).shape[0] == pc.RAY_K


# ---- the merge ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(pc.MERGE_MODES))
@pytest.mark.parametrize("case", list(pc.MERGE_CASES))
def test_merge_reference_past_the_cap(scan0_map, case, mode):
    full, voxels = scan0_map
    assert full[0].shape[0] == 8693
    pose = pc.MERGE_CASES[case][0]
    cand = pc.merge_candidates(full[0], pose, mode)
    exp = mr.merge(pc.merge_destination(full, case), voxels, pose, pc.MERGE_VS, F(pc.MERGE_TAU),
                   pc.MERGE_MODES[mode])
    print("merge %s %s: %d candidate bricks, %s" % (case, mode, cand, exp.counts))
    pc.assert_merge_past_cap(case, cand, exp.counts)
    assert exp.coords.shape[0] < 1 << 15  # fits the GPU test's destination


# ---- the indexed mesh on changed maps -----------------------------------------------------------

@pytest.fixture(scope="module")
def changed(sim, scan0):
    """(probes, name -> (oracle twin, cut)) of the maps tests/test_queries_after_change_gpu.py
    queries, by that module's own builders."""
    import test_queries_after_change_gpu as q
    return (sr.jitter_queries(*scan0), scan0), q.twins(q.decimated_scans(sim))


@pytest.mark.parametrize("name", ["evict vdbfusion_f64", "evict voxblox", "growth", "prune",
                                  "pipelined", "import", "evict, integrate, evict"])
def test_changed_maps_have_triangles_in_the_probe_box(changed, name):
    import test_queries_after_change_gpu as q
    probes, maps = changed
    twin, cut = maps[name]
    refs = q.Refs(twin, cut, probes)
    v, n, t = refs.get("imesh")
    soup = twin.extract_triangle_mesh()[0]
    print("%s: %d vertices and %d triangles in the box %s .. %s, %d triangles in the map" % (
        name, len(v), len(t), refs.box[0].tolist(), refs.box[1].tolist(), len(soup) // 3))
    assert len(t) >= 50 and len(soup) >= 300
    # the box reference is part of the twin's mesh: its triangles are the soup's, in its order
    box = meshref.deindex(v, t).view(np.uint32).reshape(-1, 9)
    whole = {r.tobytes() for r in soup.view(np.uint32).reshape(-1, 9)}
    assert all(r.tobytes() in whole for r in box)
