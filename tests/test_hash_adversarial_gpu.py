"""Inputs aimed at the hashed tables (tests/hashref.py): the Merged pre-pass's
buckets and LDS table, OVF_MG, the global brick table's probe chains, and the front end's LDS brick
hash with its fallback pairs.  Ordinary clouds spread evenly over all of them, so these branches
run only on constructed keys.  Every comparison is bitwise against the oracle (which does not use
mix64) or an exact count; every test first asserts, through hashref, the property that makes its
input adversarial."""
import json

import numpy as np
import pytest

import hashref as H
import oracle
import rayref as rr
import sampleref as sr
import statsref as S
from conftest import decimate
from test_prune_gpu import bits, inside, rows, same_bricks, same_voxels

pytestmark = pytest.mark.gpu

VS, TAU = H.VS, 0.15
F = np.float32
O = np.array(H.O)
QUAT = np.array([np.sin(0.05), 0.0, 0.1, np.cos(0.05)])  # test_voxblox_merged._posed's, j = 1
OVF_MG = 128


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    kw.setdefault("max_bricks", 1 << 14)
    kw.setdefault("max_points", 1 << 13)
    return HipTSDFVolume(kw.pop("voxel_size", VS), kw.pop("sdf_trunc", TAU), **kw)


def ora(**kw):
    return S.oracle_volume(VS, TAU, **kw)


def assert_bitwise(g, o, least=1):
    a, b = g.export_voxels(), o if isinstance(o, tuple) else o.export_voxels()
    assert a[0].shape[0] >= least
    assert same_voxels(a, b)


def device_batch(g, scans):
    """One integrate_batch_device call of (points, origin or pose) scans."""
    import torch
    x = torch.from_numpy(np.concatenate([p for p, _ in scans]).astype(F)).to(g.tensor_device)
    torch.cuda.synchronize()
    offs = np.cumsum([0] + [p.shape[0] for p, _ in scans]).astype(np.uint64)
    g.integrate_batch_device(x.data_ptr(), offs, np.stack([e for _, e in scans]))
    g.sync()
    del x


# ---- 3. the Merged pre-pass ----------------------------------------------------------------------

def ext(const):
    """The sensor: a bare origin under constant weights, a posed one under 1 / z^2 weights."""
    return O if const else np.concatenate([O, QUAT])


def merged_kw(name, const):
    kw = {k: v for k, v in H.SPECS[name].items() if k in ("max_range", "allow_clear")}
    return dict(semantics="voxblox", method="merged", use_const_weight=const, **kw)


_oracle_fields = {}


def oracle_merged(name, const):
    """(export_voxels, n_rays_total) of the oracle on a case's cloud, once per (case, weights)."""
    if (name, const) not in _oracle_fields:
        o = ora(**merged_kw(name, const))
        o.integrate(H.spec_cloud(name)[0], ext(const))
        _oracle_fields[name, const] = (o.export_voxels(), o.stats()["n_rays_total"])
        o.close()
    return _oracle_fields[name, const]


def assert_case(name, f):
    """The property that makes the case's bucket adversarial (tests/test_hashref.py recomputes
    each fact independently on the CPU)."""
    assert f["P"] == 4
    if name == "full-table":
        assert f["keys"] == f["entries"] == H.MG_TAB > H.MG_REG and f["members"] == 0
        assert f["placed"] == H.MG_TAB
    elif name == "wrap":
        assert f["keys"] == 1800 > H.MG_REG and f["wraps"] and f["longest_probe"] >= 1790
    elif name in ("rank-512", "rank-513"):
        assert f["members"] == int(name[5:]) and f["entries"] <= H.MG_REG
        assert (name == "rank-512") == (f["members"] <= H.MG_GTHREADS)
        assert f["sizes"].min() == 2 and f["sizes"].max() == 5 and f["bundles"] > 100
    elif name == "bitonic-many":
        assert f["members"] == H.MG_GM and f["entries"] > H.MG_REG and f["keys"] <= H.MG_TAB
        assert f["bundles"] > 500 and f["sizes"].min() == 2 and f["sizes"].max() == 9
    elif name.startswith("walk"):
        assert f["members"] == int(name[5:]) > H.MG_GM and f["keys"] <= H.MG_TAB
        assert f["bundles"] > 500
    elif name == "clearing":
        assert f["members"] == H.MG_GM and 250 < f["clearing_keys"] < 350
        assert f["straddled"] == 8  # voxels that form a key and a clearing key
    elif name == "clearing-dropped":
        assert f["clearing_keys"] == 0 and f["valid"] < H.N_SCAN and f["bundles"] > 300
        assert f["members"] > H.MG_GTHREADS


MERGED = ["full-table", "wrap", "rank-512", "rank-513", "bitonic-many", "walk-2049", "walk-2600",
          "clearing", "clearing-dropped"]


@pytest.mark.parametrize("const", [True, False], ids=["const", "z2-posed"])
@pytest.mark.parametrize("name", MERGED)
def test_merged_bucket(name, const):
    """One 4096-point scan whose bucket 0 holds the case's keys: the field and the ray count are
    the oracle's, bit for bit."""
    pts, f = H.spec_cloud(name)
    assert_case(name, f)
    field, n_rays = oracle_merged(name, const)
    g = hip(**merged_kw(name, const))
    g.integrate(pts, ext(const))
    g.sync()
    assert_bitwise(g, field, least=1000)
    assert g.stats()["n_rays_total"] == n_rays
    if const:
        assert n_rays == f["keys_total"]  # one ray per distinct valid key
    g.close()


@pytest.mark.parametrize("const", [True, False], ids=["const", "z2-posed"])
@pytest.mark.parametrize("layout", ["scan-1-of-3", "after-an-empty-scan"])
def test_merged_bucket_in_a_device_batch(sim, layout, const):
    """The bitonic-many scan inside a 3-scan device batch (700, 4096 and 1025 points: bucket bases
    off / 1024 + t with scans that end inside a bucket), and as scan 2 behind an empty scan."""
    pts, f = H.spec_cloud("bitonic-many")
    assert_case("bitonic-many", f)
    q = [0.0, 0.0, 0.0, 1.0]

    def other(k, n):
        p, org = sim.scan(k)
        return decimate(p, 16)[:n], org if const else np.concatenate([org, q])

    mine = (np.asarray(pts), ext(const))
    if layout == "scan-1-of-3":
        scans = [other(2, 700), mine, other(5, 1025)]
    else:
        scans = [other(2, 1025), (np.zeros((0, 3), F), other(3, 1)[1]), mine]
    kw = merged_kw("bitonic-many", const)
    g, o = hip(max_batch=3, **kw), ora(**kw)
    device_batch(g, scans)
    for p, e in scans:
        o.integrate(p, e)
    assert_bitwise(g, o, least=1000)
    assert g.stats()["n_rays_total"] == o.stats()["n_rays_total"]
    assert g.stats()["n_batches"] == 1
    g.close()


# ---- 4. OVF_MG -----------------------------------------------------------------------------------

def read_log(path):
    return [json.loads(x) for x in path.read_text().splitlines()]


def test_ovf_mg_boundary_and_message(tmp_path):
    """2048 distinct keys in one bucket fit its table (test_merged_bucket[full-table]); 2049 raise
    OVF_MG: sync() fails with TSDF_ENOMEM, the text names the cause, and the batch's metrics record
    carries the flag.  This pair pins hashref.mix64 and the bucket rule on the GPU: keys hashed any
    other way spread over the four buckets and nothing overflows."""
    from tsdf_map import TsdfError, _abi
    pts, f = H.spec_cloud("overflow")
    assert f["P"] == 4 and f["keys"] == H.MG_TAB + 1 and f["placed"] == H.MG_TAB
    fits, ff = H.spec_cloud("full-table")
    assert ff["keys"] == H.MG_TAB
    g = hip(**merged_kw("overflow", True))
    g.set_metrics_log(str(tmp_path / "fits.jsonl"))
    g.integrate(fits, O)
    g.sync()
    assert all(r["overflow"] == 0 for r in read_log(tmp_path / "fits.jsonl"))
    g.close()
    g = hip(**merged_kw("overflow", True))
    g.set_metrics_log(str(tmp_path / "m.jsonl"))
    g.integrate(pts, O)
    with pytest.raises(TsdfError) as err:
        g.sync()
    assert err.value.code == _abi.TSDF_ENOMEM
    text = str(err.value)
    assert "capacity overflow (merged integrator" in text and "bucket" in text, text
    lines = read_log(tmp_path / "m.jsonl")
    assert lines and all(r["overflow"] & OVF_MG for r in lines if r["points"] == H.N_SCAN)
    assert any(r["overflow"] & OVF_MG and r["committed"] for r in lines)  # what fits is committed
    g.sync()  # reported once
    g.close()


def test_ovf_mg_leaves_the_context_usable_and_growable(sim):
    """After the refused batch the context still grows: an ordinary scan 200 m away, into the same
    context (created at 64 bricks), grows the pool, syncs, and its region is bit for bit an oracle
    that integrated only that scan.  (What the map holds of the refused batch is not held.)"""
    from tsdf_map import TsdfError
    pts, f = H.spec_cloud("overflow")
    assert f["keys"] == H.MG_TAB + 1
    kw = merged_kw("overflow", True)
    g = hip(max_bricks=64, max_bricks_hard=1 << 20, max_points=1 << 15, **kw)
    g.integrate(pts, O)
    with pytest.raises(TsdfError):
        g.sync()
    grows = g.stats()["n_grows"]
    held = g.num_bricks()
    p, org = sim.scan(0)
    shift = np.array([0.0, 200.0, 0.0])
    p, org = (decimate(p, 4) + shift.astype(F)).astype(F), org + shift
    o = ora(**kw)
    o.integrate(p, org)
    want = o.export_bricks()
    assert want[0].shape[0] > 3 * held  # past any capacity the first batch grew to (< 2.5 x held)
    g.integrate(p, org)
    g.sync()
    assert g.stats()["n_grows"] > grows
    got = g.export_bricks()
    far = got[0][:, 1] > int(100.0 / (8 * VS))
    assert not np.any(want[0][:, 1] <= int(100.0 / (8 * VS)))
    assert same_bricks(rows(got, far), want)
    g.close()


# ---- 5. the global brick table -------------------------------------------------------------------

def sem_kw(semantics):
    return S.sem_kw(semantics)


def random_bricks(coords, semantics, seed):
    """sdf / weight [z][y][x] of every brick for import_bricks: one voxel in sixteen unobserved
    (background, weight 0), so a trilinear sample inside a brick is valid more often than not."""
    rng = np.random.default_rng(seed)
    n = len(coords)
    bg = F(0.0 if semantics == "voxblox" else TAU)
    w = rng.integers(1, 6, (n, 512)).astype(F)
    w[rng.random((n, 512)) < 1 / 16] = 0
    s = rng.uniform(-TAU, TAU, (n, 512)).astype(F)
    s[w == 0] = bg
    return np.ascontiguousarray(coords, np.int32), s.reshape(n, 8, 8, 8), w.reshape(n, 8, 8, 8)


def dense_of(field, lo, hi):
    ax = [np.arange(lo[a], hi[a], dtype=np.int64) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return field.lookup(np.stack([x, y, z], -1))


def assert_reads(g, coords, seed=5):
    """query_dense over every brick's box and sample at jittered points inside the bricks, against
    sampleref on the export."""
    field = sr.field_of(g)
    for b in np.asarray(coords, np.int64):
        gs, gw = g.query_dense(8 * b, 8 * b + 8)
        rs, rw = dense_of(field, 8 * b, 8 * b + 8)
        assert np.array_equal(bits(gs), bits(rs)) and np.array_equal(bits(gw), bits(rw))
    rng = np.random.default_rng(seed)
    b = np.asarray(coords, np.int64)[rng.integers(0, len(coords), 2048)]
    q = ((8 * b + rng.uniform(0.0, 8.0, b.shape)) * VS).astype(F)
    for mode, code in (("nearest", sr.NEAREST), ("trilinear", sr.TRILINEAR)):
        rs, rw, rg, rv = sr.sample(field, q, code)
        gs, gw, gg, gv = g.sample(q, mode=mode)
        assert rv.sum() > 100, mode
        assert np.array_equal(np.asarray(gv).astype(np.uint8), rv), mode
        assert np.array_equal(bits(gs), bits(rs)) and np.array_equal(bits(gw), bits(rw)), mode
        assert np.array_equal(bits(gg), bits(rg)), mode


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "voxblox"])
def test_import_down_one_chain(semantics):
    """60 bricks whose homes are the last 8 slots of a 128-slot table, imported in one call: the
    CAS inserts share one chain that wraps to slot 0."""
    coords, f = H.chain_bricks(60, 7)
    assert H.table_mask(64) == 127
    assert f["in_tail"] == 60 and f["wraps"] and f["longest_probe"] >= 53
    c, s, w = random_bricks(coords, semantics, 1)
    kw = sem_kw(semantics)
    g, o = hip(max_bricks=64, max_bricks_hard=64, **kw), ora(**kw)
    g.import_bricks(c, s, w)
    o.import_bricks(c, s, w)
    order = np.argsort(H.brick_key(c))  # the export's (z, y, x) order
    assert same_bricks(g.export_bricks(), (c[order], s[order], w[order]))
    assert same_bricks(g.export_bricks(), o.export_bricks())
    assert_reads(g, c)
    _, s2, w2 = random_bricks(coords, semantics, 2)
    g.import_bricks(c, s2, w2)
    o.import_bricks(c, s2, w2)
    got = g.export_bricks()
    assert same_bricks(got, o.export_bricks()) and g.num_bricks() == 60
    assert not np.array_equal(bits(got[1]), bits(s[order]))  # the second import merged
    assert_reads(g, c)
    g.close()


def chain_scans(sim):
    """(scans, end bricks): points at the voxel (4, 4, 4) of 300 bricks that stay at the end of
    a 2048-slot table, seen from the simulator's origin; and two small scans into the same bricks
    (voxels (3, 3, 3) and (5, 5, 5) of a hundred of them) for the device batch."""
    coords, f = H.chain_bricks(300, 11)
    assert H.table_mask(1024) == 2047
    assert f["in_tail"] == 300 and f["wraps"] and f["longest_probe"] >= 290
    org = sim.scan(0)[1]
    c0 = np.floor(org / (8 * VS)).astype(np.int64)
    c = coords[np.abs(coords - c0).max(axis=1) >= 2].astype(np.int64)
    assert len(c) >= 295

    def at(b, v):
        return ((8 * b + v + 0.5) * VS).astype(F)

    return [(at(c[:100], 3), org), (at(c, 4), org), (at(c[-100:], 5), org)], c


@pytest.mark.parametrize("batch", ["alone", "device-batch"])
@pytest.mark.parametrize("walk", ["two", "single"])
@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "voxblox"])
def test_integrate_down_one_chain(sim, semantics, walk, batch):
    """k_place's / k_walk's table_insert with 300 new bricks on one wrapping chain, into an empty
    2048-slot table."""
    scans, c = chain_scans(sim)
    kw = sem_kw(semantics)
    g, o = hip(max_bricks=1024, walk=walk, max_batch=1 if batch == "alone" else 3, **kw), ora(**kw)
    if batch == "alone":
        scans = scans[1:2]
        g.integrate(*scans[0])
        g.sync()
    else:
        device_batch(g, scans)
    for p, e in scans:
        o.integrate(p, e)
    assert_bitwise(g, o, least=1500)
    st = g.stats()
    assert st["n_grows"] == 0 and st["n_bricks"] <= 1024  # the table stayed at 2048 slots
    held = g.export_bricks()[0].astype(np.int64)
    assert np.isin(H.brick_key(c), H.brick_key(held)).all()
    assert H.chain_facts(held, 2047)["longest_probe"] >= 280
    g.close()


def chain_rays(coords, seed):
    """256 rays through bricks of the set: from 1 m in front of a point inside a brick."""
    rng = np.random.default_rng(seed)
    b = np.asarray(coords, np.int64)[rng.integers(0, len(coords), 256)]
    p = (8 * b + rng.uniform(1.0, 7.0, b.shape)) * VS
    d = rng.normal(size=b.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(p - d, F), np.ascontiguousarray(d, F)


def assert_step(g, o, seed):
    got = g.export_bricks()
    assert same_bricks(got, o.export_bricks())
    org, d = chain_rays(got[0], seed)
    field = sr.field_of(g)
    rd, rn, rh = rr.raycast(field, org, d, None, 0.0, 2.0, VS / 2, rr.NEAREST)
    gd, gn, gh = g.raycast(org, d, None, 0.0, 2.0, VS / 2, "nearest")
    assert np.array_equal(np.asarray(gh).astype(np.uint8), rh)
    assert np.array_equal(bits(gd), bits(rd)) and np.array_equal(bits(gn), bits(rn))
    return int(rh.sum())


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "voxblox"])
def test_chain_through_growth_evict_and_prune(semantics):
    """250 bricks at the table's end under every mask up to 1024 slots, imported in three calls
    from 64 bricks (k_rehash into 256 and 512 slots), then evict_outside and prune (the table is
    rebuilt): after each step the export is the oracle twin's and rays through the kept bricks are
    rayref's."""
    coords, f = H.chain_bricks(250, 10)
    assert f["in_tail"] == 250 and f["wraps"]
    for bits_ in (8, 9, 10):
        ff = H.chain_facts(coords, (1 << bits_) - 1)
        assert ff["in_tail"] == 250 and ff["wraps"] and ff["longest_probe"] >= 240, bits_
    c, s, w = random_bricks(coords, semantics, 3)
    # a surface across every brick (negative below local x = 4), so rays find zero crossings
    s = (s * F(0.25) + F(0.5 * TAU) * np.sign(np.arange(8) - 3.5).astype(F)).astype(F)
    s[w == 0] = F(0.0 if semantics == "voxblox" else TAU)
    w[c[:, 1] % 2 == 1] = np.minimum(w[c[:, 1] % 2 == 1], F(4))  # bricks the prune below drops
    kw = sem_kw(semantics)
    g, o = hip(max_bricks=64, **kw), ora(**kw)
    hits = 0
    for k, part in enumerate((slice(0, 83), slice(83, 166), slice(166, 250))):
        g.import_bricks(c[part], s[part], w[part])
        o.import_bricks(c[part], s[part], w[part])
        hits += assert_step(g, o, 10 + k)
    assert g.stats()["n_grows"] >= 2
    lo, hi = [-81, -81, -81], [0, 81, 81]
    keep = inside(c, lo, hi)
    assert 90 < keep.sum() < 160
    pre = o.export_bricks()
    o2 = ora(**kw)
    o2.import_bricks(*rows(pre, inside(pre[0], lo, hi)))
    g.evict_outside(lo, hi)
    assert g.num_bricks() == int(keep.sum())
    hits += assert_step(g, o2, 20)
    # prune: voxels below weight 5 back to the background, bricks left without a voxel dropped
    pc, ps, pw = o2.export_bricks()
    ps, pw = ps.copy(), pw.copy()
    ps[pw < F(5.0)] = F(0.0 if semantics == "voxblox" else TAU)
    pw[pw < F(5.0)] = 0
    left = (pw > 0).reshape(len(pc), -1).any(1)
    o3 = ora(**kw)
    o3.import_bricks(pc[left], ps[left], pw[left])
    assert 20 < left.sum() < len(pc) - 20
    g.prune(5.0)
    assert g.num_bricks() == int(left.sum())
    hits += assert_step(g, o3, 30)
    assert H.chain_facts(g.export_bricks()[0], 1023)["in_tail"] == g.num_bricks() > 50
    assert hits > 20  # the rays found surfaces to compare
    g.close()


# ---- 6. the workgroup's LDS brick hash -----------------------------------------------------------

LDS_CLOUDS = {"window": dict(window=16, anchor=700), "wrap": dict(window=8, anchor=H.HCAP - 8)}
_lds = {}


def lds_case(sim, name):
    """(points, origin, facts, statsref's record of the scan alone, the oracle's field of it)."""
    if name not in _lds:
        org = sim.scan(0)[1]
        kw = LDS_CLOUDS[name]
        pts, f = H.lds_chain_cloud(200, centre=org, **kw)
        assert pts.shape[0] == H.RPB and f["bricks"] == f["in_window"] == 200
        assert f["must_fall"] >= 100 and f["fell"] >= f["must_fall"]  # fallback pairs
        assert f["wraps"] == f["wraps_full"] == (name == "wrap") and f["longest_full"] > 180
        ref = S.scan_ref_numpy(pts, org, "vdbfusion_f64")
        o = ora()
        o.integrate(pts, org)
        _lds[name] = (pts, org, f, ref, o.export_voxels())
        o.close()
    return _lds[name]


def assert_last_batch(g, refs):
    rec = S.batch_refs(refs, [len(refs)])[0][0]
    st = g.stats()
    assert st["n_pairs_last"] == rec["pairs"] > rec["rays"]
    assert st["n_voxels_last"] == rec["voxel_updates"]
    assert st["n_active_last"] == rec["active_bricks"] >= 200


@pytest.mark.parametrize("walk", ["two", "single"])
@pytest.mark.parametrize("name", sorted(LDS_CLOUDS))
def test_lds_hash_wide_and_single_walk(sim, name, walk):
    """The scan alone: one 1024-lane k_count workgroup whose LDS hash takes 200 bricks in one
    neighbourhood (over LDS_PROBES: fallback pairs), and the single walk's unbounded lds_insert_full
    on the same cloud; the field and the last batch's counters."""
    pts, org, f, ref, field = lds_case(sim, name)
    g = hip(walk=walk)
    g.integrate(pts, org)
    g.sync()
    assert_bitwise(g, field, least=3000)
    if walk == "two":
        assert_last_batch(g, [ref])
    else:
        assert g.stats()["n_voxels_last"] == ref.u_vox
    g.close()


@pytest.mark.parametrize("name", sorted(LDS_CLOUDS))
def test_lds_hash_large_batch_count(sim, name):
    """The scan as the last of a device batch of more than count_wide (512, tsdf_capi.cpp) k_count
    blocks: eight half scans of the simulator fill 512, so launch_count takes the form for large
    batches.  The filler's field is the oracle's export, imported into the twin."""
    import torch
    pts, org, f, ref, _ = lds_case(sim, name)
    filler = [(decimate(sim.scan(k)[0], 2), sim.scan(k)[1]) for k in range(8)]
    blocks = sum(-(-p.shape[0] // H.RPB) for p, _ in filler) + 1
    assert blocks > 512
    if "filler" not in _lds:
        o = oracle.OracleTSDFVolume(VS, TAU, threads=8)
        for p, e in filler:
            o.integrate(p, e)
        _lds["filler"] = o.export_bricks()
        o.close()
    o = ora()
    o.import_bricks(*_lds["filler"])
    o.integrate(pts, org)
    g = hip(max_bricks=1 << 17, max_points=1 << 16, max_batch=9)
    device_batch(g, filler + [(pts, org)])
    assert g.stats()["n_batches"] == 1
    assert_bitwise(g, o, least=100000)
    g.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("env", [{"TSDF_COUNT_WIDE": "0"},
                                 {"TSDF_COUNT_WIDE": "0", "TSDF_COUNT_PAIRED": "1"}],
                         ids=["narrow", "paired"])
@pytest.mark.parametrize("name", sorted(LDS_CLOUDS))
def test_lds_hash_count_shapes(sim, monkeypatch, name, env):
    """The same scan through the 256-lane k_count and through the paired one (two blocks per
    512-lane workgroup), by the switches tests/test_stats_gpu.py uses."""
    for k in ("TSDF_COUNT_PAIRED", "TSDF_COUNT_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pts, org, f, ref, field = lds_case(sim, name)
    g = hip()
    g.integrate(pts, org)
    g.sync()
    assert_bitwise(g, field, least=3000)
    assert_last_batch(g, [ref])
    g.close()


@pytest.mark.parametrize("name", sorted(LDS_CLOUDS))
def test_lds_hash_sector_contexts(sim, name):
    """A 2-sector context (sector_rule="world"): k_count's plain form behind k_sector_flags, each
    sector against its oracle twin."""
    pts, org, f, ref, _ = lds_case(sim, name)
    n = 0
    for k in range(2):
        kw = dict(n_sectors=2, sector=k, sector_rule="world")
        g, o = hip(**kw), ora(**kw)
        g.integrate(pts, org)
        o.integrate(pts, org)
        g.sync()
        assert_bitwise(g, o, least=500)
        assert g.stats()["n_rays_total"] == o.stats()["n_rays_total"]
        n += g.stats()["n_rays_total"]
        g.close()
    assert n == ref.rays


@pytest.mark.parametrize("name", sorted(LDS_CLOUDS))
def test_lds_hash_three_scans_one_batch(sim, name):
    """The same scan three times in one batch: the fallback pairs carry three scans' ranks into
    k_integrate."""
    pts, org, f, ref, _ = lds_case(sim, name)
    g, o = hip(max_batch=3), ora()
    for _ in range(3):
        g.integrate(pts, org)
        o.integrate(pts, org)
    g.sync()
    assert g.stats()["n_batches"] == 1
    assert_bitwise(g, o, least=3000)
    assert_last_batch(g, [ref] * 3)
    g.close()
