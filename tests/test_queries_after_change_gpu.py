"""The read-side kernels on a map whose layout has just changed.

evict_outside and prune compact the pool, move bricks between slots and rebuild the table; growth
reallocates pool and table; import_bricks merges into held bricks; a pipelined context answers
with batches still queued.  A stale slot, a key the rehash left behind or a pointer kept across a
growth shows first in the queries, so after each change the GPU's export must equal the oracle
twin's (the change applied to the oracle the way tests/test_prune_gpu.py does), and then sample,
align_terms, raycast, esdf and query_dense must equal the numpy references run on that export, bit
for bit, and the mesh the twin's.  The indexed mesh, the one query with a slot map of its own (pool
slot -> position in the sorted brick list), de-indexed must be that soup, and in the probes' box it
must equal tests/meshref.py on the export.

For the changes that remove something the same references run on the map before the change, and
the test asserts that the change shows in them (queries, rays and distance-field sites lost)."""
import numpy as np
import pytest

import esdfref
import meshref
import rayref as rr
import sampleref as sr
from conftest import decimate
from test_prune_gpu import (bits, bitwise, cut_box, hip, inside, ora, reference, rows, same_voxels,
                            sem_kw)

pytestmark = pytest.mark.gpu

F = np.float32
BASE = dict(voxel_size=sr.VOXEL_SIZE, sdf_trunc=sr.SDF_TRUNC)
MODES = {"nearest": sr.NEAREST, "trilinear": sr.TRILINEAR}
RADIUS = 12                    # voxels: the distance field is exact up to 1.2 m
T_MIN, T_MAX, STEP = rr.T_MIN, rr.T_MAX, rr.STEP  # 0.5 .. 40 m every 0.05 m
KINDS = ("sample", "align", "raycast", "esdf", "dense", "mesh", "imesh")
MESH_MARGIN = 2                # voxels of field around the box that the mesh reference reads


def kw_of(semantics="vdbfusion_f64", **kw):
    return sem_kw(semantics, **dict(BASE, **kw))


def decimated_scans(sim):
    """Scans 0..5 of the trajectory, every fourth point."""
    return [(decimate(p, 4), o) for p, o in (sim.scan(k) for k in range(6))]


@pytest.fixture(scope="module")
def scans(sim):
    return decimated_scans(sim)


@pytest.fixture(scope="module")
def probes(scan0):
    """(queries (n, 3), the scan): the sampling tests' jittered queries of scan 0, and the scan
    the rays are made of."""
    return sr.jitter_queries(*scan0), scan0


def rays_for(scan, hi):
    """(origins (n, 3), unit directions (n, 3)) fp32.  The raycast tests' 2048 rays of the scan,
    from the sensor (at x = 8 m: towards the kept half they cross the removed one, whose bricks
    the kernel skips); and rays aimed at the kept half alone, where the map is sparse and the
    sensor's rays seldom find two valid samples around the surface: every 16th scan point at
    least half a metre below the cut face x = 8 hi[0] voxels, its ray started 2 m in front of
    the point."""
    org, d, _ = rr.scan_rays(*scan)
    p = np.asarray(scan[0], np.float64)[::16]
    v = p - np.asarray(scan[1], np.float64)
    r = np.linalg.norm(v, axis=1)
    sel = (p[:, 0] < 8 * int(hi[0]) * sr.VOXEL_SIZE - 0.5) & (r > 3.0)
    u = v[sel] / r[sel, None]
    assert sel.sum() >= 1000
    o = np.concatenate([np.broadcast_to(org, d.shape), (p[sel] - 2.0 * u).astype(F)])
    return np.ascontiguousarray(o, F), np.ascontiguousarray(np.concatenate([d, u.astype(F)]), F)


def box_across(lo, hi, scan0):
    """The 97 x 80 x 33 voxel box around the fixture centre's (y, z), centred in x on the face
    hi[0] of the brick box (lo, hi): half of it on either side of the cut."""
    c = esdfref.fixture_centre(scan0)
    c[0] = 8 * int(hi[0])
    return esdfref.fixture_box(c)


def dense_of(field, lo, hi):
    """(S, W) [z, y, x] of voxels lo..hi-1 from an exported field: query_dense's reference."""
    ax = [np.arange(lo[a], hi[a], dtype=np.int64) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return field.lookup(np.stack([x, y, z], -1))


class Refs:
    """The numpy references of every query on one volume's export (a GPU volume's, or the oracle
    twin's where the GPU volume must not be read first), each computed once."""

    def __init__(self, vol, cut, probes):
        """cut: the brick box (lo, hi) whose face hi[0] the probes are laid across."""
        self.field = sr.field_of(vol)
        self.vs = vol.voxel_size
        self.queries, scan = probes
        self.box = box_across(*cut, scan)
        self.org, self.dirs = rays_for(scan, cut[1])
        self.memo = {}

    def get(self, kind, mode=None):
        k = (kind, mode)
        if k not in self.memo:
            if kind == "sample":
                r = sr.sample(self.field, self.queries, MODES[mode])
            elif kind == "align":
                r = sr.align_terms(self.field, self.queries, sr.start_pose())
            elif kind == "raycast":
                r = rr.raycast(self.field, self.org, self.dirs, None, T_MIN, T_MAX, STEP,
                               MODES[mode])
            elif kind == "dense":
                r = dense_of(self.field, *self.box)
            elif kind == "esdf":
                S, W = self.get("dense")
                r = esdfref.esdf(S, W, self.vs, RADIUS, self.vs) + (
                    esdfref.classify(S, W, self.vs, 0.0)[1],)
            elif kind == "imesh":  # (vertices, normals, triangles) of the cubes in the box
                import oracle
                from tsdf_map import _abi
                lo, hi = self.box
                S, W = dense_of(self.field, lo - MESH_MARGIN, hi + MESH_MARGIN)
                # (the oracle's table: tests/test_mesh.py holds the library's to it)
                tab = meshref.mc_table(oracle.load(), _abi.MC_TABLES["generated"])
                r = meshref.indexed_mesh_ref(S, W, lo - MESH_MARGIN, self.vs, tab, lo=lo, hi=hi)
            self.memo[k] = r
        return self.memo[k]


def check(g, refs, twin, kinds=KINDS):
    """Every query of `kinds` on the GPU volume against the references, bitwise."""
    for kind in kinds:
        if kind == "sample":
            for mode in MODES:
                rs, rw, rg, rv = refs.get("sample", mode)
                gs, gw, gg, gv = g.sample(refs.queries, mode=mode)
                assert np.array_equal(gv.astype(np.uint8), rv), mode
                assert np.array_equal(bits(gs), bits(rs)) and np.array_equal(bits(gw), bits(rw))
                assert np.array_equal(bits(gg), bits(rg)), mode
        elif kind == "align":
            H, b, e, nv, ab = refs.get("align")
            gH, gb, ge, gnv = g.align_terms(refs.queries, sr.start_pose())
            assert gnv == nv
            got = np.concatenate([gH.reshape(36), gb, [ge]])
            ref = np.concatenate([H.reshape(36), b, [e]])
            if nv <= 1:
                assert np.array_equal(got, ref)
            else:  # any summation order of the same double terms
                assert np.all(np.abs(got - ref) <= nv * 2.0 ** -52 * ab[:43])
        elif kind == "raycast":
            for mode in MODES:
                rd, rn, rh = refs.get("raycast", mode)
                gd, gn, gh = g.raycast(refs.org, refs.dirs, None, T_MIN, T_MAX, STEP, mode)
                assert np.array_equal(gh.astype(np.uint8), rh), mode
                assert np.array_equal(bits(gd), bits(rd)) and np.array_equal(bits(gn), bits(rn))
        elif kind == "esdf":
            dist, flags, _ = refs.get("esdf")
            # (max_dist half a voxel short of the radius: ceil(max_dist / voxel_size) = RADIUS)
            assert g.esdf_radius((RADIUS - 0.5) * refs.vs) == RADIUS
            esdfref.assert_same(g.esdf(*refs.box, (RADIUS - 0.5) * refs.vs), (dist, flags))
        elif kind == "dense":
            S, W = refs.get("dense")
            gs, gw = g.query_dense(*refs.box)
            assert np.array_equal(bits(gs), bits(S)) and np.array_equal(bits(gw), bits(W))
        elif kind == "mesh":
            vg, _ = g.extract_triangle_mesh()
            vo, _ = twin.extract_triangle_mesh()
            assert len(vo) >= 300 and vg.shape == vo.shape and np.array_equal(bits(vg), bits(vo))
        elif kind == "imesh":
            v, t, n = g.extract_indexed_mesh()
            vo, _ = twin.extract_triangle_mesh()
            soup = meshref.deindex(v, t)
            assert len(vo) >= 300 and soup.shape == vo.shape and np.array_equal(bits(soup), bits(vo))
            assert int(t.max()) + 1 == len(v) == np.unique(t).size
            assert g.indexed_mesh_counts() == {"n_bricks": g.num_bricks(), "n_vertices": len(v),
                                               "n_triangles": len(t)}
            rv, rn, rt = refs.get("imesh")
            assert len(rt) >= 50, len(rt)
            bv, bt, bn = g.extract_indexed_mesh(lo=refs.box[0], hi=refs.box[1])
            assert bt.shape == rt.shape and np.array_equal(bt, rt)
            assert bv.shape == rv.shape and np.array_equal(bits(bv), bits(rv))
            assert np.array_equal(bits(bn), bits(rn))


def counts(refs):
    """What the comparisons had to say: valid samples per mode, ray hits per mode, sites."""
    out = {"valid_" + m: int(refs.get("sample", m)[3].sum()) for m in MODES}
    out.update({"hits_" + m: int(refs.get("raycast", m)[2].sum()) for m in MODES})
    out["n_valid_align"] = refs.get("align")[3]
    out["sites"] = int(refs.get("esdf")[2].sum())
    out["box_triangles"] = int(refs.get("imesh")[2].shape[0])
    out["observed"] = int((refs.get("dense")[1] > 0).sum())
    return out


def assert_not_vacuous(c):
    """The comparisons compare something on every path: valid and invalid samples, hits and
    misses, sites and observed voxels in the box."""
    for m in MODES:  # (trilinear hits need two fully observed cubes in a row: rare after a prune)
        assert c["valid_" + m] >= 100 and c["hits_" + m] >= (100 if m == "nearest" else 10), c
    assert c["n_valid_align"] >= 100 and c["sites"] >= 100 and c["observed"] >= 1000, c
    assert c["box_triangles"] >= 50, c


def assert_change_shows(before, after):
    """The non-vacuity of the removing changes, on the references before and after: >= 100
    queries valid before and invalid after, >= 100 valid both times, >= 100 rays that hit before
    and miss or hit farther after, >= 100 distance-field sites gone.  Returns the counts."""
    out = {}
    vb = before.get("sample", "trilinear")[3].astype(bool)
    va = after.get("sample", "trilinear")[3].astype(bool)
    out["queries_lost"], out["queries_kept"] = int((vb & ~va).sum()), int((vb & va).sum())
    db, _, hb = before.get("raycast", "nearest")
    da, _, ha = after.get("raycast", "nearest")
    hb, ha = hb.astype(bool), ha.astype(bool)
    out["rays_lost"] = int((hb & (~ha | (da > db))).sum())
    sb, sa = before.get("esdf")[2], after.get("esdf")[2]
    out["sites_lost"] = int((sb & ~sa).sum())
    assert all(v >= 100 for v in out.values()), out
    return out


def build_twin(scans, **kw):
    """The oracle volume after the scans."""
    o = ora(**kw)
    for pts, org in scans:
        o.integrate(pts, org)
    return o


def build(scans, **kw):
    """(GPU volume, oracle twin) after the same scans; the fields are equal before any change."""
    g, o = hip(**kw), build_twin(scans, **kw)
    for pts, org in scans:
        g.integrate(pts, org)
    assert bitwise(g, o)
    return g, o


# The changes as the oracle twin sees them.  The tests below apply the same boxes, thresholds and
# parts to the GPU volume; tests/test_pastcap_inputs.py builds the twins alone, on the CPU.

def evicted_twin(o, **kw):
    """(twin, (lo, hi)): o without the bricks outside cut_box."""
    lo, hi = cut_box(o.export_bricks()[0])
    return reference(o, lambda c: inside(c, lo, hi), **kw), (lo, hi)


def import_part(second, cut):
    """The bricks of the export `second` inside the brick box `cut`."""
    return rows(second, inside(second[0], *cut))


def second_evict_box(c0):
    """The other box of evict-integrate-evict: everything from the median brick y on goes."""
    c0 = np.asarray(c0, np.int64)
    lo2, hi2 = c0.min(0), c0.max(0) + 1
    hi2[1] = int(np.median(c0[:, 1]))
    return lo2, hi2


def evict_integrate_evict_twins(o, again, **kw):
    """(twin after evict and the scans `again`, twin after the second evict, first box, second
    box)."""
    c0 = o.export_bricks()[0]
    lo, hi = cut_box(c0)
    o2 = reference(o, lambda c: inside(c, lo, hi), again, **kw)
    lo2, hi2 = second_evict_box(c0)
    return o2, reference(o2, lambda c: inside(c, lo2, hi2), **kw), (lo, hi), (lo2, hi2)


PRUNE_WEIGHT = 2.0


def twins(scans):
    """name -> (oracle twin, cut) of every map the tests below query."""
    out = {}
    for sem in ("vdbfusion_f64", "voxblox"):
        kw = kw_of(sem)
        out["evict " + sem] = evicted_twin(build_twin(scans[:4], **kw), **kw)
    kw = kw_of()
    o = build_twin(scans[:4], **kw)
    cut = cut_box(o.export_bricks()[0])
    out["growth"] = (o, cut)
    out["prune"] = (pruned_twin(o, PRUNE_WEIGHT, **kw)[0], cut)
    o6 = build_twin(scans, **kw)
    out["pipelined"] = (o6, cut_box(o6.export_bricks()[0]))
    a, b = build_twin(scans[:2], **kw), build_twin(scans[2:4], **kw)
    cut = cut_box(a.export_bricks()[0].astype(np.int64))
    a.import_bricks(*import_part(b.export_bricks(), cut))
    out["import"] = (a, cut)
    _, twin, first, _ = evict_integrate_evict_twins(o, scans[4:6], **kw)
    out["evict, integrate, evict"] = (twin, first)
    return out


def pruned_twin(o, m, **kw):
    """VDBVolume.prune on the oracle's export: voxels below m back to the background, bricks left
    without an observed voxel dropped, the rest imported into a fresh oracle volume."""
    c, s, w = o.export_bricks()
    bg = F(0.0 if kw.get("semantics") == "voxblox" else kw["sdf_trunc"])
    s, w = s.copy(), w.copy()
    s[w < F(m)] = bg
    w[w < F(m)] = 0
    keep = (w > 0).reshape(len(c), -1).any(1)
    assert 0 < keep.sum() < len(c)
    o2 = ora(**kw)
    o2.import_bricks(c[keep], s[keep], w[keep])
    return o2, int(len(c) - keep.sum())


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "voxblox"])
def test_after_evict(scans, probes, semantics):
    kw = kw_of(semantics)
    g, o = build(scans[:4], **kw)
    twin, (lo, hi) = evicted_twin(o, **kw)
    n0 = g.num_bricks()
    n_ev = g.evict_outside(lo, hi, copy_out=False)
    assert 0 < n_ev < n0 and g.num_bricks() == n0 - n_ev
    assert bitwise(g, twin)
    after = Refs(g, (lo, hi), probes)
    shows = assert_change_shows(Refs(o, (lo, hi), probes), after)
    c = counts(after)
    print("evict %s: %d of %d bricks removed, %s, %s" % (semantics, n_ev, n0, shows, c))
    assert_not_vacuous(c)
    check(g, after, twin)
    g.close()


def test_after_prune(scans, probes):
    kw = kw_of()
    g, o = build(scans[:4], **kw)
    cut = cut_box(o.export_bricks()[0])
    twin, n_gone = pruned_twin(o, PRUNE_WEIGHT, **kw)
    assert g.prune(PRUNE_WEIGHT) == n_gone
    assert bitwise(g, twin)
    after = Refs(g, cut, probes)
    shows = assert_change_shows(Refs(o, cut, probes), after)
    c = counts(after)
    print("prune(2): %d bricks removed, %s, %s" % (n_gone, shows, c))
    assert_not_vacuous(c)
    check(g, after, twin)
    g.close()


def test_after_growth(scans, probes):
    """max_bricks = 128: pool and table are reallocated several times while the map is built."""
    kw = kw_of()
    g, o = build(scans[:4], max_bricks=128, **kw)
    st = g.stats()
    print("growth: %d grows to %d bricks" % (st["n_grows"], st["n_bricks"]))
    assert st["n_grows"] >= 3 and st["n_bricks"] == o.num_bricks() > 16 * 128
    refs = Refs(g, cut_box(o.export_bricks()[0]), probes)
    assert_not_vacuous(counts(refs))
    check(g, refs, o)
    g.close()


def test_after_import_merge(scans, probes):
    """Scans 2-3 of a second volume imported into a map of scans 0-1: a merge into held bricks,
    new bricks beside them.  Consecutive scans share nearly every brick, so the half of the
    second volume's export below the median brick x is imported: about half the held bricks are
    merged into, and the probes lie across the face between the merged half and the other."""
    kw = kw_of()
    g, o = build(scans[:2], **kw)
    g2, o2 = build(scans[2:4], **kw)
    held = o.export_bricks()[0].astype(np.int64)
    cut = cut_box(held)
    part = import_part(g2.export_bricks(), cut)
    new = part[0].astype(np.int64)
    key = lambda c: (c[:, 0] + (1 << 20)) | ((c[:, 1] + (1 << 20)) << 21) | ((c[:, 2] + (1 << 20)) << 42)  # noqa: E731
    share, fresh = np.isin(key(held), key(new)).mean(), int((~np.isin(key(new), key(held))).sum())
    print("import: %.0f %% of the %d held bricks are merged into, %d new" %
          (100 * share, len(held), fresh))
    assert 0.3 <= share <= 0.7 and fresh >= 10
    before = o.export_voxels()
    g.import_bricks(*part)
    o.import_bricks(*import_part(o2.export_bricks(), cut))
    assert bitwise(g, o) and not same_voxels(before, o.export_voxels())
    refs = Refs(g, cut, probes)
    assert_not_vacuous(counts(refs))
    check(g, refs, o)
    g.close()
    g2.close()


def test_after_evict_integrate_evict(scans, probes):
    """Evict, integrate two more scans back into the removed region, evict with another box."""
    kw = kw_of()
    g, o = build(scans[:4], **kw)
    again = scans[4:6]
    o2, twin, (lo, hi), (lo2, hi2) = evict_integrate_evict_twins(o, again, **kw)
    assert g.evict_outside(lo, hi, copy_out=False) > 0
    for pts, org in again:
        g.integrate(pts, org)
    assert bitwise(g, o2) and not inside(o2.export_bricks()[0], lo, hi).all()
    n0 = g.num_bricks()
    n_ev = g.evict_outside(lo2, hi2, copy_out=False)
    assert 0 < n_ev < n0
    assert bitwise(g, twin)
    refs = Refs(g, (lo, hi), probes)
    print("evict, integrate, evict: %d of %d bricks removed, %s" % (n_ev, n0, counts(refs)))
    assert_not_vacuous(counts(refs))
    check(g, refs, twin)
    g.close()


def test_pipelined_unsynced(scans, probes):
    """pipeline = 2, max_batch = 4: six scans integrated and not synced -- one batch in flight,
    two scans queued -- then a query at once.  Every kind of query meets that state on a volume
    of its own; the references run on the oracle twin's export, which each volume's export must
    equal afterwards."""
    kw = kw_of()
    o = build_twin(scans, **kw)
    refs = Refs(o, cut_box(o.export_bricks()[0]), probes)
    assert_not_vacuous(counts(refs))
    for kind in KINDS:
        g = hip(pipeline=2, max_batch=4, **kw)
        for pts, org in scans:
            g.integrate(pts, org)
        check(g, refs, o, kinds=(kind,))
        assert bitwise(g, o), kind
        g.close()
