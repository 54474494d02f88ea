"""Inputs that take the read-side kernels past their grid caps (test helper).

Every per-brick, per-tile and per-ray kernel on the read side launches a capped grid and strides
over the rest; a workgroup's second trip reuses its LDS and recomputes its origin from a larger
index.  This module builds inputs larger than each cap, restates the index -> trip mapping of each
kernel in plain numpy (as tests/test_esdf_plan.py restates the plan), and states the conditions
under which a comparison on such an input says something about the second trip.  It reads no GPU:
tests/test_pastcap_inputs.py asserts the conditions on the numpy and oracle references alone, the
GPU tests assert them again and then compare the kernels with those references bit for bit.

    kernels                                   first trip                input here
    k_mesh_mark, _vertices, _indices          4096 bricks               a sphere of 18^3 bricks
    k_mesh_vcount (4 bricks a workgroup)      16 384 bricks             a sphere of 26^3 bricks
    k_mesh_slot_index (256 a workgroup)       1 048 576 bricks          none: no test passes it
    k_esdf_classify, _x, _axis<0>, _axis<1>   8192 tiles                three thin boxes
    k_raycast                                 8192 x 256 rays           2039 distinct rays, tiled
    k_merge_flag, k_merge_apply               8192 candidate bricks     the full scan-0 map
"""
import functools

import numpy as np

import esdfref as er
import meshref
import mergeref as mr
import rayref as rr
import sampleref as sr
from test_mesh import VS as MESH_VS, sphere_bricks

F = np.float32

MESH_CAP = 4096             # tsdf_mesh.hip: workgroups of k_mesh_mark, _vertices, _indices, a brick each
MESH_VCOUNT_CAP = 4096 * 4  # k_mesh_vcount: a wave per brick, four to a workgroup
ESDF_CAP = 8192             # esdf_plan.h ESDF_GRID_CAP
RAY_STRIDE = 8192 * 256     # tsdf_raycast.hip: rays per trip
MERGE_CAP = 8192            # tsdf_merge.hip MERGE_GRID_CAP


def _key(c):
    """Brick keys whose integer order is the (z, y, x) order of the sorted brick list."""
    c = np.asarray(c, np.int64).reshape(-1, 3) + (1 << 20)
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


# ---- the indexed mesh ---------------------------------------------------------------------------

# the surface crosses the brick faces at voxel 0 on every axis (tests/test_mesh_indexed_gpu.py)
MESH_CENTER = (0.113, -0.121, 0.207)
MESH_RADIUS = 52.8 * MESH_VS  # 18^3 = 5832 bricks
# A box whose planes are no multiples of 8.  It holds a voxel of every brick in x and y and of
# the 15 layers z = -9 .. 5, so the call lists 4860 bricks and passes the cap itself (a box that
# lists fewer than 4097 bricks has no second trip, wherever it lies in the map); its plane z = 45
# cuts the sphere and the bricks of layer 5.
MESH_BOX = (np.array([-67, -69, -70], np.int64), np.array([67, 66, 45], np.int64))


def mc_table(name):
    """Case table `name` of the oracle library (tests/test_mesh.py holds the product's to it)."""
    import oracle
    from tsdf_map import _abi
    return meshref.mc_table(oracle.load(), _abi.MC_TABLES[name])


@functools.lru_cache(maxsize=None)
def mesh_map(kind):
    """(coords, sdf, weight) of the large sphere, every voxel observed ("full"), or with a seeded
    10 % of the voxels unobserved and 5 % at W = 0.5 ("holed", as the `holed` fixture)."""
    c, s, w = sphere_bricks(MESH_RADIUS, center=MESH_CENTER)
    if kind == "holed":
        w = meshref.holed(w)
        low = np.random.default_rng(3).random(w.shape) < 0.05
        w = np.where(low & (w > 0), F(0.5), w).astype(F)
    else:
        assert kind == "full"
    return c, s, w


def mesh_listed(coords, lo=None, hi=None):
    """mesh_plan.h mesh_list_bricks restated: the bricks the kernels list, in (z, y, x) order --
    all of them, or those that hold a voxel of [lo, hi + 1)."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    c = c[np.argsort(_key(c))]
    if lo is None:
        return c
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    return c[np.all((8 * c + 8 > lo) & (8 * c < hi + 1), axis=1)]


@functools.lru_cache(maxsize=None)
def mesh_case(kind, tname, min_weight, boxed):
    """One comparison of the large sphere: (reference (vertices, normals, triangles), sides).
    sides: the listed bricks, and what lies either side of position MESH_CAP of that list --
    vertices by their owner (the brick of the vertex's min voxel) and the triangles that index
    vertices from both sides."""
    b = mesh_map(kind)
    lo, hi = MESH_BOX if boxed else (None, None)
    info = {}
    ref = meshref.indexed_mesh_ref(*meshref.dense_from_bricks(*b), MESH_VS, mc_table(tname),
                                   min_weight=min_weight, lo=lo, hi=hi, info=info)
    listed = mesh_listed(b[0], lo, hi)
    keys = _key(listed)
    own = _key(info["edges"][:, :3] >> 3)
    pos = np.searchsorted(keys, own)
    assert np.array_equal(keys[pos], own)  # every owner is listed
    assert np.all(np.diff(pos) >= 0)       # and the vertices are in the list's order
    past = pos >= MESH_CAP
    tp = past[ref[2].astype(np.int64)]
    sides = dict(n_bricks=int(listed.shape[0]), brick_at_cap=tuple(listed[MESH_CAP].tolist()),
                 n_vertices=int(ref[0].shape[0]), n_triangles=int(ref[2].shape[0]),
                 vertices_below=int((~past).sum()), vertices_past=int(past.sum()),
                 triangles_across=int((tp.any(1) & ~tp.all(1)).sum()),
                 triangles_past=int(tp.all(1).sum()))
    return ref, sides


# 26^3 = 17 576 bricks, more than k_mesh_vcount's first trip.  The centre lies 12 voxels up, so
# that the last two brick layers (z >= 88 voxels, the bricks from position 16 384 on) hold the
# sphere's top 10 voxels.  No numpy reference at this size: the comparison is with the soup.
MESH_BIG_CENTER = (0.113, -0.121, 0.607)
MESH_BIG_RADIUS = 86 * MESH_VS


def mesh_big_map():
    return sphere_bricks(MESH_BIG_RADIUS, center=MESH_BIG_CENTER)


@functools.lru_cache(maxsize=None)
def mesh_big_sides():
    """The 26^3-brick sphere either side of position MESH_VCOUNT_CAP of its sorted brick list:
    the vertices of the cubes in the top 10 voxels of the sphere (z >= 88) that bricks from that
    position on own, and those of the bottom 10 (z < -64) that earlier bricks own -- by the
    reference on the three brick layers around each, which hold every voxel those cubes read."""
    c, s, w = mesh_big_map()
    listed = mesh_listed(c)
    keys = _key(listed)
    far = 1 << 20
    out = dict(n_bricks=int(listed.shape[0]), brick_at_cap=tuple(listed[MESH_VCOUNT_CAP].tolist()))
    for side, keep, lo, hi in (("past", c[:, 2] >= 10, (-far, -far, 88), (far, far, far)),
                               ("below", c[:, 2] <= -8, (-far, -far, -far), (far, far, -64))):
        info = {}
        meshref.indexed_mesh_ref(*meshref.dense_from_bricks(c[keep], s[keep], w[keep]), MESH_VS,
                                 mc_table("generated"), lo=lo, hi=hi, info=info)
        pos = np.searchsorted(keys, _key(info["edges"][:, :3] >> 3))
        own = pos >= MESH_VCOUNT_CAP if side == "past" else pos < MESH_VCOUNT_CAP
        out["vertices_" + side] = int(own.sum())
    return out


def assert_mesh_vcount_past_cap(sides):
    assert sides["n_bricks"] > MESH_VCOUNT_CAP, sides
    assert sides["vertices_past"] >= 1000 and sides["vertices_below"] >= 1000, sides


def assert_mesh_past_cap(sides):
    assert sides["n_bricks"] > MESH_CAP, sides
    assert sides["vertices_past"] >= 1000 and sides["vertices_below"] >= 1000, sides
    assert sides["triangles_across"] >= 100, sides


# ---- the distance field -------------------------------------------------------------------------

ESDF_VS, ESDF_TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC
ESDF_LANES, ESDF_X_LINES, ESDF_THREADS = 64, 16, 256

# name -> extents (x, y, z), radius, the box's low corner (no multiples of 8, both signs), the
# kernels it takes past the cap with their tile counts, and where the voxels are seeded: regions
# [z, y, x] of the box as (slices, share of the voxels observed).  The regions lie around each
# trip-2 region's boundary and in the first tiles.
ESDF_BOXES = {
    # classify: linear index >= 2 097 152 is the end of z-layer 3 (from y = 717, x = 452) and
    # layer 4; z pass: plane index >= 524 288 is y = 723 from x = 113, and y = 724
    "wide": dict(n=(725, 725, 5), radius=12, lo=(-100, 43, -2),
                 past={"classify": 10267, "z": 8213},
                 seed=[((slice(0, 5), slice(705, 725), slice(380, 530)), 0.05),
                       ((slice(0, 5), slice(712, 725), slice(60, 170)), 0.15),
                       ((slice(0, 5), slice(0, 12), slice(0, 80)), 0.05)]),
    # x pass: lines z * 364 + y >= 131 072 are z = 360 from y = 32, and z >= 361
    "tall": dict(n=(5, 364, 364), radius=4, lo=(3, -201, -179),
                 past={"x": 8281},
                 seed=[((slice(352, 364), slice(0, 80), slice(0, 5)), 0.12),
                       ((slice(0, 6), slice(100, 140), slice(0, 5)), 0.12)]),
    # y pass: tiles (z, y segment) >= 8192 are z >= 4096; its x pass is past the cap as well:
    # lines z * 33 + y >= 131 072 are z = 3971 from y = 29, and z >= 3972
    "long": dict(n=(3, 33, 4100), radius=12, lo=(-1, -17, -2051),
                 past={"x": 8457, "y": 8200},
                 seed=[((slice(4080, 4100), slice(0, 33), slice(0, 3)), 0.3),
                       ((slice(3962, 3982), slice(0, 33), slice(0, 3)), 0.3),
                       ((slice(0, 20), slice(0, 33), slice(0, 3)), 0.3)]),
}


def _cd(a, b):
    return -(-a // b)


def esdf_seg(radius):
    return 32 if radius <= 48 else 64


def esdf_tile_of(kernel, n, radius):
    """The tile (classify: the workgroup of the first trip's grid) that handles each voxel of a
    box of extents n = (x, y, z), [z, y, x] int64, and the number of tiles: tsdf_esdf.hip's index
    arithmetic read backwards."""
    nx, ny, nz = n
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    seg = esdf_seg(radius)
    if kernel == "classify":   # one lane per voxel, 256 to a workgroup
        return ((z * ny + y) * nx + x) // ESDF_THREADS, _cd(nx * ny * nz, ESDF_THREADS)
    if kernel == "x":          # 16 lines by 64 voxels of x
        xt = _cd(nx, ESDF_LANES)
        return ((z * ny + y) // ESDF_X_LINES) * xt + x // ESDF_LANES, xt * _cd(ny * nz, ESDF_X_LINES)
    if kernel == "y":          # 64 voxels of x by seg of y, per z
        it, st = _cd(nx, ESDF_LANES), _cd(ny, seg)
        return (z * st + y // seg) * it + x // ESDF_LANES, it * st * nz
    assert kernel == "z"       # 64 voxels of the x-y plane by seg of z
    it = _cd(nx * ny, ESDF_LANES)
    return (z // seg) * it + (y * nx + x) // ESDF_LANES, it * _cd(nz, seg)


def dilate(mask, r):
    """Voxels within r (per axis) of a voxel of `mask`."""
    out = mask.copy()
    for axis in range(3):
        src = out.copy()
        n = src.shape[axis]
        for d in range(1, min(r, n - 1) + 1):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[axis], b[axis] = slice(0, n - d), slice(d, n)
            out[tuple(a)] |= src[tuple(b)]
            out[tuple(b)] |= src[tuple(a)]
    return out


@functools.lru_cache(maxsize=None)
def esdf_case(name):
    """(voxels {(x, y, z): (S, W)} for esdfref.make_bricks, lo, hi, radius, (S, W) dense [z, y, x],
    the reference (dist, flags)) of box `name`."""
    box = ESDF_BOXES[name]
    nx, ny, nz = box["n"]
    lo = np.array(box["lo"], np.int64)
    rng = np.random.default_rng(17)
    S = np.full((nz, ny, nx), F(ESDF_TAU), F)
    W = np.zeros((nz, ny, nx), F)
    band = F(ESDF_VS)
    for sl, share in box["seed"]:
        shape = S[sl].shape
        seen = rng.random(shape) < share
        site = seen & (rng.random(shape) < 0.4)
        s = np.where(site, rng.uniform(-band, band, shape),                  # |S| <= band
                     rng.choice([-1.0, 1.0], shape) * rng.uniform(0.15, 0.3, shape)).astype(F)
        S[sl] = np.where(seen, s, S[sl])
        W[sl] = np.where(seen, rng.integers(1, 3, shape).astype(F), W[sl])
    zz, yy, xx = np.nonzero(W)
    voxels = {(int(x + lo[0]), int(y + lo[1]), int(z + lo[2])): (S[z, y, x], W[z, y, x])
              for z, y, x in zip(zz, yy, xx)}
    ref = er.esdf(S, W, ESDF_VS, box["radius"], ESDF_VS)
    return voxels, lo, lo + np.array(box["n"], np.int64), box["radius"], (S, W), ref


def esdf_sides(name):
    """Per kernel that box `name` takes past the cap: its tiles, and for the voxels of the later
    trips ("past") and of the first ("below") the sites, the uncapped voxels that are no sites and
    the observed non-site voxels of either sign, and the sites within R of the other side."""
    box = ESDF_BOXES[name]
    _, _, _, radius, (S, W), (dist, flags) = esdf_case(name)
    site = (flags & er.SITE) != 0
    free = ((flags & er.CAPPED) == 0) & ~site
    seen = ((flags & er.OBSERVED) != 0) & ~site
    out = {}
    for kernel in ("classify", "x", "y", "z"):
        tile, tiles = esdf_tile_of(kernel, box["n"], radius)
        assert int(tile.max()) + 1 == tiles
        if kernel not in box["past"]:
            assert tiles <= ESDF_CAP, (name, kernel, tiles)
            out[kernel] = dict(tiles=tiles)
            continue
        past = tile >= ESDF_CAP
        d = dict(tiles=tiles, voxels_past=int(past.sum()))
        for side, m in (("past", past), ("below", ~past)):
            d["sites_" + side] = int((site & m).sum())
            d["uncapped_" + side] = int((free & m).sum())
            d["negative_" + side] = int((seen & m & (S < 0)).sum())
            d["positive_" + side] = int((seen & m & (S > 0)).sum())
            d["sites_near_boundary_" + side] = int((site & m & dilate(~m, radius)).sum())
        out[kernel] = d
    return out


def assert_esdf_past_cap(name, sides):
    box = ESDF_BOXES[name]
    for kernel, tiles in box["past"].items():
        d = sides[kernel]
        assert d["tiles"] == tiles > ESDF_CAP, (name, kernel, d)
        for side in ("past", "below"):
            assert d["sites_" + side] >= 20 and d["uncapped_" + side] >= 100, (name, kernel, d)
            assert d["negative_" + side] >= 1 and d["positive_" + side] >= 1, (name, kernel, d)
            assert d["sites_near_boundary_" + side] >= 1, (name, kernel, d)


# ---- the raycast --------------------------------------------------------------------------------

RAY_N = RAY_STRIDE + 77
RAY_K = 2039                 # odd, and no divisor of the stride: lane i - stride holds another ray
RAY_T = (0.0, 3.0, 0.05)     # 61 samples a ray
RAY_TAIL = 77


def ray_distinct(scan):
    """RAY_K distinct rays of a scan, each started 2 m in front of its point
    (tests/test_queries_after_change_gpu.py rays_for), two of three towards the point:
    (origins, unit directions) fp32."""
    assert RAY_K % 2 == 1 and RAY_STRIDE % RAY_K != 0
    p = np.asarray(scan[0], np.float64)
    v = p - np.asarray(scan[1], np.float64)
    r = np.linalg.norm(v, axis=1)
    sel = np.flatnonzero(r > 3.0)
    sel = sel[:: sel.size // RAY_K][:RAY_K]
    assert sel.size == RAY_K
    u = v[sel] / r[sel, None]
    o = p[sel] - 2.0 * u
    # From there every ray finds its point in the nearest mode, so every third ray is turned
    # round: back towards the sensor through observed free space, a miss.
    u[2::3] = -u[2::3]
    return np.ascontiguousarray(o.astype(F)), np.ascontiguousarray(u.astype(F))


def ray_references(field, scan):
    """mode -> (depth, normal, hit) of the RAY_K distinct rays."""
    o, d = ray_distinct(scan)
    return {m: rr.raycast(field, o, d, None, *RAY_T, mode)
            for m, mode in (("nearest", rr.NEAREST), ("trilinear", rr.TRILINEAR))}


def ray_tiling(refs):
    """idx (RAY_N,): ray i is distinct ray idx[i] = (i + rot) % RAY_K, with the first rotation at
    which the last RAY_TAIL rays hold hits and misses in every mode."""
    base = np.arange(RAY_N, dtype=np.int64)
    for rot in range(RAY_K):
        idx = (base + rot) % RAY_K
        tail = idx[-RAY_TAIL:]
        if all(0 < int(r[2][tail].sum()) < RAY_TAIL for r in refs.values()):
            return idx, rot
    raise AssertionError("no rotation leaves hits and misses among the last rays")


def ray_sides(refs, idx):
    out = {"rays": int(idx.size), "distinct": RAY_K}
    for m, r in refs.items():
        out["hit_share_" + m] = float(r[2][idx].mean())
        out["tail_hits_" + m] = int(r[2][idx[-RAY_TAIL:]].sum())
        out["second_trip_hits_" + m] = int(r[2][idx[RAY_STRIDE:]].sum())
    return out


def assert_rays_past_cap(sides):
    assert sides["rays"] > RAY_STRIDE, sides
    for m in ("nearest", "trilinear"):
        assert 0.10 <= sides["hit_share_" + m] <= 0.90, sides
        assert 0 < sides["tail_hits_" + m] < RAY_TAIL, sides


# ---- the merge ----------------------------------------------------------------------------------

MERGE_VS, MERGE_TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC
MERGE_CASES = {
    # name: (pose, the destination's share of the source's bricks)
    "empty_general": (mr.rigid((10.0, -20.0, 30.0), (1.234, -2.345, 0.456)), None),
    "alternate_half_voxel": (mr.rigid(t=(0.05, 0.05, 0.05)), slice(None, None, 2)),
}
MERGE_MODES = {"nearest": sr.NEAREST, "trilinear": sr.TRILINEAR}


def merge_candidates(src_coords, pose, mode):
    """The distinct destination bricks the candidate search lists for the source bricks, by the
    restatement of merge_plan.h in tests/test_merge_plan.py."""
    import test_merge_plan as mp
    rule, _, fwd, ti_vox = mp.xform([float(v) for v in np.asarray(pose, np.float64).reshape(12)],
                                    MERGE_MODES[mode], 0.0, float(F(MERGE_VS)))
    assert rule == mp.OK
    out = set()
    for B in np.asarray(src_coords, np.int64).tolist():
        lo, hi, _, ctr, reach2 = mp.brick_box(fwd, ti_vox, B, MERGE_MODES[mode])
        out.update(mp.box_bricks(lo, hi, ctr, reach2))
    return len(out)


def merge_destination(full, case):
    """The destination's export_bricks() before the merge."""
    held = MERGE_CASES[case][1]
    if held is None:
        return (np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), F), np.zeros((0, 8, 8, 8), F))
    return tuple(a[held] for a in full)


def assert_merge_past_cap(case, candidates, counts):
    assert candidates > MERGE_CAP, candidates
    assert counts["merged_voxels"] >= 1000, counts
    if MERGE_CASES[case][1] is not None:  # held and new candidates alternate
        assert counts["new_bricks"] >= 1000, counts
        assert counts["touched_bricks"] - counts["new_bricks"] >= 1000, counts
        assert counts["overlap_voxels"] >= 1000, counts
