"""The indexed mesh's contract (include/tsdf_hip_mesh.h) as tests/meshref.py restates it, on the
CPU: de-indexed it is the oracle's soup bit for bit, a sphere is closed by its indices alone, the
normals are unit vectors along the radius, coinciding vertices stay distinct, and write_ply
round-trips.  tests/test_mesh_indexed_gpu.py then holds the GPU to this reference bit for bit."""
import math
import os

import numpy as np
import pytest

import meshref
import oracle
from test_mesh import TAU, VS, sphere_bricks

CENTER = np.array([0.013, -0.021, 0.007])  # sphere_bricks' default


def tables():
    lib = oracle.load()
    return {"generated": meshref.mc_table(lib, 0), "lorensen": meshref.mc_table(lib, 1)}


def fields():
    coords, sdf, w = sphere_bricks(0.37)
    return {"sphere": (coords, sdf, w), "holed": (coords, sdf, meshref.holed(w))}


@pytest.mark.parametrize("tname", ["generated", "lorensen"])
@pytest.mark.parametrize("field", ["sphere", "holed"])
def test_reference_deindexed_is_the_oracle_soup(field, tname):
    coords, sdf, w = fields()[field]
    o = oracle.OracleTSDFVolume(VS, TAU)
    o.import_bricks(coords, sdf, w)
    soup, _ = o.extract_triangle_mesh(table=tname)
    info = {}
    v, n, t = meshref.indexed_mesh_ref(*meshref.dense_from_bricks(coords, sdf, w), VS,
                                       tables()[tname], info=info)
    got = meshref.deindex(v, t)
    assert got.shape == soup.shape
    assert np.array_equal(got.view(np.uint32), soup.view(np.uint32))
    assert t.dtype == np.uint32 and n.shape == v.shape
    assert t.max() < v.shape[0] and np.unique(t).shape[0] == v.shape[0]
    if field == "holed":  # the GPU test on this field is not vacuous
        assert t.shape[0] > 50
        assert info["cubes_per_vertex"].min() >= 1 and info["cubes_per_vertex"].max() == 4
        assert np.any(info["cubes_per_vertex"] < 4)
        for k in (1, 2, 3):  # edges with 1, 2 and 3 meshed cubes around them all occur
            assert np.any(info["cubes_per_vertex"] == k), k
    else:
        assert np.all(info["cubes_per_vertex"] == 4)  # a closed surface in a full field


def index_topology(n_vertices, tris):
    """(E, balanced) from the indices alone: no welding by position."""
    t = tris.astype(np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    code = d[:, 0] * n_vertices + d[:, 1]
    rev = d[:, 1] * n_vertices + d[:, 0]
    once = np.unique(code).shape[0] == code.shape[0]  # every directed edge once ...
    balanced = once and np.array_equal(np.sort(code), np.sort(rev))  # ... and its reverse once
    und = np.unique(np.minimum(d[:, 0], d[:, 1]) * n_vertices + np.maximum(d[:, 0], d[:, 1]))
    return und.shape[0], balanced


@pytest.mark.parametrize("radius", [0.37, 1.1])
@pytest.mark.parametrize("tname", ["generated", "lorensen"])
def test_sphere_is_closed_by_its_indices_and_normals_follow_the_radius(radius, tname):
    coords, sdf, w = sphere_bricks(radius)
    v, n, t = meshref.indexed_mesh_ref(*meshref.dense_from_bricks(coords, sdf, w), VS,
                                       tables()[tname])
    V, F = v.shape[0], t.shape[0]
    assert F > 50
    assert t.max() < V
    assert np.unique(t).shape[0] == V  # every vertex is referenced
    E, balanced = index_topology(V, t)
    assert balanced  # closed and consistently oriented
    assert V - E + F == 2
    # unit length within fp32 rounding: three squares and two sums (<= 2.5 ulp on n2, halved by
    # the root), the root and the division (1 ulp each): a few 2^-24; 8 ulp = 4.8e-7 asserted
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 8 * 2.0 ** -24
    # along the radius, outwards.  Measured worst angle of this reference: 0.227 deg at radius
    # 0.37, 0.034 deg at radius 1.1 (mean 0.095 / 0.011 deg); asserted with a margin of a few
    # degrees
    r = v.astype(np.float64) - CENTER
    r /= np.linalg.norm(r, axis=1)[:, None]
    cos = np.einsum("ij,ij->i", r, n.astype(np.float64) / length[:, None])
    worst = math.degrees(math.acos(min(1.0, float(cos.min()))))
    print("radius %g %s: worst normal angle %.4f deg" % (radius, tname, worst))
    assert worst < 3.0


def test_coinciding_vertices_stay_distinct():
    """S_a == 0 gives t = 0 on the three edges that start at a: three vertices, one position."""
    sdf = np.full((1, 8, 8, 8), -0.1, np.float32)
    a = (3, 4, 5)  # (x, y, z)
    sdf[0, a[2], a[1], a[0]] = 0.0  # the one voxel that is not inside
    w = np.ones_like(sdf)
    coords = np.array([[0, 0, 0]], np.int32)
    info = {}
    v, n, t = meshref.indexed_mesh_ref(*meshref.dense_from_bricks(coords, sdf, w), VS,
                                       tables()["generated"], info=info)
    e = info["edges"]
    own = np.nonzero(np.all(e[:, :3] == np.array(a), axis=1))[0]
    assert own.tolist() == list(range(own[0], own[0] + 3)) and e[own, 3].tolist() == [0, 1, 2]
    centre = ((np.array(a, np.float32) + np.float32(0.5)) * np.float32(VS)).astype(np.float32)
    for i in own:
        assert np.array_equal(v[i].view(np.uint32), centre.view(np.uint32))
    assert v.shape[0] == 6 and np.unique(t).shape[0] == 6  # the six edges at a, all referenced
    # de-indexed it is still the oracle's soup
    o = oracle.OracleTSDFVolume(VS, TAU)
    o.import_bricks(coords, sdf, w)
    soup, _ = o.extract_triangle_mesh()
    assert np.array_equal(meshref.deindex(v, t).view(np.uint32), soup.view(np.uint32))


def test_box_restricts_cubes_only():
    """With a box the reference keeps the soup's triangles whose cube lies in it, in order, and
    gradients still read the voxels outside."""
    coords, sdf, w = sphere_bricks(0.37)
    dense = meshref.dense_from_bricks(coords, sdf, w)
    tab = tables()["generated"]
    v, n, t = meshref.indexed_mesh_ref(*dense, VS, tab)
    lo, hi = np.array([-3, -20, 1]), np.array([5, 3, 20])
    vb, nb, tb = meshref.indexed_mesh_ref(*dense, VS, tab, lo=lo, hi=hi)
    assert 0 < tb.shape[0] < t.shape[0]
    full = {p.tobytes(): q.tobytes() for p, q in zip(v, n)}
    assert all(full[p.tobytes()] == q.tobytes() for p, q in zip(vb, nb))  # same normals
    soup = meshref.deindex(v, t).reshape(-1, 9)
    part = meshref.deindex(vb, tb).reshape(-1, 9)
    rows = {r.tobytes(): i for i, r in enumerate(soup)}
    at = [rows[r.tobytes()] for r in part]
    assert at == sorted(at)


def read_ply(path):
    """A small reader of what write_ply writes."""
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n"
        assert f.readline() == b"format binary_little_endian 1.0\n"
        props, counts, elem = {}, {}, None
        while True:
            line = f.readline().decode("ascii").split()
            if line[0] == "end_header":
                break
            if line[0] == "element":
                elem = line[1]
                counts[elem] = int(line[2])
                props[elem] = []
            elif line[0] == "property":
                props[elem].append(line[1:])
        assert props["face"] == [["list", "uchar", "uint", "vertex_indices"]]
        assert all(p[0] == "float" for p in props["vertex"])
        names = [p[1] for p in props["vertex"]]
        vert = np.frombuffer(f.read(4 * len(names) * counts["vertex"]), "<f4")
        vert = vert.reshape(-1, len(names))
        face = np.frombuffer(f.read(13 * counts["face"]),
                             np.dtype([("n", "u1"), ("i", "<u4", (3,))]))
        assert f.read() == b""
    assert np.all(face["n"] == 3)
    return names, vert, face["i"]


@pytest.mark.parametrize("with_normals", [True, False])
def test_write_ply_round_trips(tmp_path, with_normals):
    from tsdf_map.mesh import write_ply
    coords, sdf, w = sphere_bricks(0.37)
    v, n, t = meshref.indexed_mesh_ref(*meshref.dense_from_bricks(coords, sdf, w), VS,
                                       tables()["generated"])
    path = str(tmp_path / "mesh.ply")
    with open(path, "wb") as f:
        f.write(b"stale")
    write_ply(path, v, t, n if with_normals else None)
    assert os.listdir(str(tmp_path)) == ["mesh.ply"]  # the temporary file is gone
    names, vert, face = read_ply(path)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert np.array_equal(vert[:, :3].view(np.uint32), v.view(np.uint32))
    if with_normals:
        assert np.array_equal(vert[:, 3:].view(np.uint32), n.view(np.uint32))
    assert np.array_equal(face, t)
    with pytest.raises(ValueError):
        write_ply(path, v, t + np.uint32(v.shape[0]))
    assert read_ply(path)[2].shape == t.shape  # a refused write leaves the file as it was


def test_tile_boxes_cover_the_bricks():
    from tsdf_map.mesh import tile_boxes
    coords = np.array([[0, 0, 0], [-1, 0, 2], [3, -2, 0]])
    boxes = tile_boxes(coords, 12)
    vox = {tuple(8 * c + np.array(d)) for c in coords for d in np.ndindex(8, 8, 8)}
    covered = set()
    for lo, hi in boxes:
        assert np.all(lo % 12 == 0) and np.all(hi - lo == 12)
        inside = {p for p in vox if all(lo[a] <= p[a] < hi[a] for a in range(3))}
        assert inside  # only boxes a brick touches
        assert not inside & covered
        covered |= inside
    assert covered == vox
    keys = [(int(lo[2]), int(lo[1]), int(lo[0])) for lo, _ in boxes]
    assert keys == sorted(keys)
