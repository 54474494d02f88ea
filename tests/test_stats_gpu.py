"""The batch counters of tsdf_get_stats and the metrics log against tests/statsref.py (DESIGN.md
§18): every comparison is exact integer equality with a reference that shares no code with the
kernels, and in every case the field is also bitwise the oracle's, so no counter passes on a wrong
map.  One code path per test: k_integrate_small and k_integrate batches under the three pipelines,
the single walk, the per-sample-weight kernels, carving, sector shards, a dense brick, growth and
replay, reset_stats, a map changed underneath, and the metrics ring."""
import json

import numpy as np
import pytest

import statsref as S

pytestmark = pytest.mark.gpu

VS, TAU = S.VS, S.TAU
REC_KEYS = ("scans", "points", "rays", "pairs", "voxel_updates", "dirty_voxels", "active_bricks",
            "new_bricks", "bricks", "algorithmic_bytes")
_fields = {}


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    kw.setdefault("max_bricks", 1 << 15)
    kw.setdefault("max_points", 1 << 14)
    return HipTSDFVolume(kw.pop("voxel_size", VS), kw.pop("sdf_trunc", TAU), **kw)


def oracle_field(key, scans, **kw):
    """The oracle's field after `scans` (one export, cached per key)."""
    if key not in _fields:
        o = S.oracle_volume(**kw)
        for p, e in scans:
            o.integrate(p, e)
        _fields[key] = o.export_voxels()
        o.close()
    return _fields[key]


def assert_field(g, ref):
    gi, gs, gw = g.export_voxels()
    ri, rs, rw = ref
    assert gi.shape == ri.shape and np.array_equal(gi, ri)
    assert np.array_equal(gw.view(np.uint32), rw.view(np.uint32))
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32))


def read_log(path):
    return [json.loads(x) for x in path.read_text().splitlines()]


def assert_record_invariants(r):
    """What holds for every record, committed or not, by the definitions alone: a voxel is dirty
    when at least one and at most `scans` of the batch's scans updated it."""
    assert r["dirty_voxels"] <= r["voxel_updates"] <= r["scans"] * r["dirty_voxels"], r
    if r["scans"] == 1:
        assert r["dirty_voxels"] == r["voxel_updates"], r
    assert r["algorithmic_bytes"] == 12 * r["rays"] + 16 * r["voxel_updates"], r
    assert r["new_bricks"] <= r["active_bricks"] <= r["pairs"], r


def assert_new_chain(lines, cap0):
    """new_bricks along the whole log of a context that grew from cap0 bricks, committed lines or
    not.  A line's `bricks - new_bricks` is the pool its run found.  After a committed line that is
    the committed line's `bricks` (so new_bricks is exact there).  After uncommitted lines it is
    what a growth kept of their bricks: at least the pool the first of them found, at most the
    pool the largest of them reached -- and exactly cap0 the first time, where the log's first run
    overflowed the initial pool, since grow_capacity keeps min(pool_count, capacity) bricks (the
    later capacities follow grow_capacity's own sizing rule and are not restated here)."""
    prev, run, first_cut = None, [], True
    for i, r in enumerate(lines):
        found = r["bricks"] - r["new_bricks"]
        if prev is None:
            assert found == 0, r
        elif not run:
            assert found == prev["bricks"], (prev, r)
        else:
            lo, hi = run[0]["bricks"] - run[0]["new_bricks"], max(x["bricks"] for x in run)
            assert lo <= found <= hi, (run, r)
            if found != prev["bricks"] and first_cut:  # a growth cut the pool at its capacity
                first_cut = False
                if len(run) == i and run[0]["bricks"] > cap0:
                    assert found == cap0, (run, r)
        run = [] if r["committed"] else run + [r]
        prev = r


def assert_counters(g, log, refs, held=None, before=(), vacuity=True, shards=True, skip=(),
                    new_exact=True, cap0=None):
    """Stats and the committed log records of `g` against the reference of `refs` in the batches
    the log reports; `before`: reference records of committed batches that ran before `refs`
    (they precede in the log and in the totals).  Returns (reference records, held bricks)."""
    g.sync()
    st = g.stats()
    lines = read_log(log)
    for r in lines:
        assert_record_invariants(r)
    ok = [r for r in lines if r["committed"]]
    ids = [r["batch"] for r in lines]
    assert ids == sorted(set(ids))
    if not new_exact:
        assert_new_chain(lines, cap0)
    part = [r["scans"] for r in ok[len(before):]]
    want, held = S.batch_refs(refs, part, held)
    if vacuity:
        S.assert_nonvacuous(refs, part, want, shards=shards)
    allw = list(before) + want
    assert len(ok) == len(allw)
    for got, w in zip(ok, allw):
        for k in REC_KEYS:
            if w[k] is None or k in skip:
                continue
            if k == "new_bricks" and not new_exact:
                assert got[k] <= w[k], (k, got, w)
                continue
            assert got[k] == w[k], (k, got, w)
    tot = S.totals(allw)
    for k, v in tot.items():
        if k in skip:
            continue
        assert st[k] == v, (k, st[k], v)
    return want, held


def run_host(scans, log, **kw):
    g = hip(**kw)
    g.set_metrics_log(log)
    for p, e in scans:
        g.integrate(p, e)
    return g


def run_device(scans, log, **kw):
    """The same scans through integrate_batch_device (one call; max_batch scans per batch)."""
    import torch
    g = hip(**kw)
    g.set_metrics_log(log)
    allp = np.concatenate([p for p, _ in scans])
    offs = np.cumsum([0] + [p.shape[0] for p, _ in scans]).astype(np.uint64)
    org = np.stack([o for _, o in scans])
    d = torch.from_numpy(allp).to(g.tensor_device)
    torch.cuda.synchronize()
    g.integrate_batch_device(d.data_ptr(), offs, org)
    g.sync()
    del d
    return g


# ---- 1. batch shapes, two walks -----------------------------------------------------------------

@pytest.mark.parametrize("pipeline", [0, 1, 2])
@pytest.mark.parametrize("max_batch", [1, 3, 9, 64])
@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_batch_shapes_two_walks(sim, tmp_path, semantics, max_batch, pipeline):
    """max_batch 1 and 3: k_integrate_small; 9 and 64: k_integrate (64: the widest window), each
    with a short last batch (11 = 3+3+3+2 = 9+2 scans; 70 = 64+6), so *_last must be the last
    batch's numbers, not the largest batch's.  Host queue and integrate_batch_device alike."""
    name = "seq70" if max_batch == 64 else "seq11"
    scans, refs = S.scans_of(sim, name), S.refs_numpy(sim, name, semantics)
    kw = dict(max_batch=max_batch, pipeline=pipeline, **S.sem_kw(semantics))
    field = oracle_field((name, semantics), scans, **kw)
    want = None
    for k, run in enumerate((run_host, run_device)):
        g = run(scans, tmp_path / ("m%d.jsonl" % k), **kw)
        w, _ = assert_counters(g, tmp_path / ("m%d.jsonl" % k), refs)
        assert [r["scans"] for r in w] == S.partition_of(len(scans), max_batch)
        assert want is None or w == want
        want = w
        st = g.stats()
        assert st["n_grows"] == 0 and st["n_replayed"] == 0
        assert_field(g, field)
        g.close()
    if len(want) > 1 and max_batch > 1:
        assert want[-1]["voxel_updates"] < want[0]["voxel_updates"]


# ---- 2. single walk, k_count's other shapes, ray tiles -----------------------------------------

@pytest.mark.parametrize("max_batch,pipeline", [(1, 0), (3, 2), (9, 0), (9, 1), (64, 2)])
@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_single_walk(sim, tmp_path, semantics, max_batch, pipeline):
    """walk="single": k_walk counts rays and pairs, k_spans feeds k_integrate (no small kernel)."""
    name = "seq70" if max_batch == 64 else "seq11"
    scans, refs = S.scans_of(sim, name), S.refs_numpy(sim, name, semantics)
    kw = dict(max_batch=max_batch, pipeline=pipeline, walk="single", **S.sem_kw(semantics))
    g = run_host(scans, tmp_path / "m.jsonl", **kw)
    assert_counters(g, tmp_path / "m.jsonl", refs)
    assert_field(g, oracle_field((name, semantics), scans, **kw))
    g.close()
    g = hip(**kw)  # the front end that ran is the single walk
    g.set_profiling(True)
    g.integrate(*scans[0])
    g.sync()
    launches = g.stats()["kernel_launches"]
    assert launches["walk"] == 1 and launches["count"] == 0
    g.close()


@pytest.mark.parametrize("env", [
    {"TSDF_COUNT_PAIRED": "1", "TSDF_COUNT_WIDE": "0"},   # two blocks per 512-lane workgroup
    {"TSDF_COUNT_WIDE": "0"},                             # the 256-lane k_count of large batches
    {"TSDF_RAY_TILES": "64"},                             # ray tiles, 1024-lane k_count
    {"TSDF_RAY_TILES": "64", "TSDF_COUNT_WIDE": "0"},
], ids=["paired", "narrow", "tiles", "tiles-narrow"])
@pytest.mark.parametrize("semantics", S.SEMANTICS)
def test_count_shapes_and_ray_tiles(sim, tmp_path, monkeypatch, semantics, env):
    """k_count's workgroup shapes (tests/test_gpu_parity.py::test_paired_count_workgroups_bitwise's
    switches) and the ray-tile front end (tests/test_ray_tiles_gpu.py's): the same counters.  With
    tiles, tiled_scans is the number of scans walked as tiles; nothing else moves."""
    for k in ("TSDF_COUNT_PAIRED", "TSDF_COUNT_WIDE", "TSDF_RAY_TILES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scans, refs = S.scans_of(sim, "seq11"), S.refs_numpy(sim, "seq11", semantics)
    kw = dict(max_batch=9, **S.sem_kw(semantics))
    g = run_host(scans, tmp_path / "m.jsonl", **kw)
    assert_counters(g, tmp_path / "m.jsonl", refs)
    assert_field(g, oracle_field(("seq11", semantics), scans, **kw))
    g.close()
    for r in read_log(tmp_path / "m.jsonl"):
        if "TSDF_RAY_TILES" in env:
            assert 0 < r["tiled_scans"] <= r["scans"]
        else:
            assert r["tiled_scans"] == 0


# ---- 3. Voxblox variants ------------------------------------------------------------------------

def with_pose(scans):
    return [(p, np.concatenate([o, [0.0, 0.0, 0.0, 1.0]])) for p, o in scans]


@pytest.mark.parametrize("max_batch", [3, 9])
@pytest.mark.parametrize("variant", ["depth", "merged"])
def test_voxblox_per_sample_weights(sim, tmp_path, variant, max_batch):
    """1 / z^2 weights and method="merged" run the per-sample-weight kernels (semantics 3); merged
    rays are bundles.  Rays and vox are the oracle's, dirty / active / new route A's (pairs: no
    route covers them here)."""
    scans = with_pose(S.scans_of(sim, "seq3"))
    kw = dict(semantics="voxblox", max_batch=max_batch,
              **({"method": "merged"} if variant == "merged" else {}))
    refs = [S.scan_ref_oracle(p, e, **kw) for p, e in scans]
    assert all(r.u_vox == r.oracle_vox for r in refs)  # vox as the oracle's stats count it
    if variant == "merged":
        assert all(r.rays < r.points for r in refs)
    g = run_host(scans, tmp_path / "m.jsonl", **kw)
    assert_counters(g, tmp_path / "m.jsonl", refs)
    assert_field(g, oracle_field(("seq3", variant), scans, **kw))
    g.close()


def test_voxblox_clearing_rays(sim, tmp_path):
    """Constant weights, allow_clear and max_range 12 m: the rays beyond 12 m (three in four of
    this scene's) become clearing rays, the others hit.  Route A for the scans; pairs from the
    oracle one ray at a time on a hundred rays per scan."""
    kw = dict(max_batch=3, **S.CLEAR_KW)
    scans = S.scans_of(sim, "seq3")
    refs = [S.scan_ref_oracle(p, o, **kw) for p, o in scans]
    assert all(r.u_vox == r.oracle_vox for r in refs)
    g = run_host(scans, tmp_path / "m.jsonl", **kw)
    assert_counters(g, tmp_path / "m.jsonl", refs)
    assert_field(g, oracle_field(("seq3", "clear"), scans, **kw))
    g.close()
    few, refs = S.refs_few_rays(sim, *S.CLEAR_FEW, **S.CLEAR_KW)
    S.assert_few_rays_nonvacuous(few, refs, S.CLEAR_KW)
    g = run_host(few, tmp_path / "f.jsonl", **kw)
    assert_counters(g, tmp_path / "f.jsonl", refs, shards=False)
    assert_field(g, oracle_field(("seq3", "clear-few"), few, **kw))
    g.close()


# ---- 4. space carving ---------------------------------------------------------------------------

@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "vdbfusion"])
def test_space_carving(sim, tmp_path, semantics):
    """Carving to 20 m (k_count's maxp != 4 branch: pairs emitted one by one, fallback pairs).
    The range limit keeps a third of this scene's rays, so the batch is 16 scans decimated by 64:
    10 515 valid rays in 32 blocks.  Pairs: the oracle one ray at a time, on under 300 rays."""
    ckw = S.carve_kw(semantics)
    kw = dict(max_batch=16, max_bricks=1 << 16, **ckw)
    scans = S.scans_of(sim, "carve16")
    refs = S.refs_oracle(sim, "carve16", **ckw)
    g = run_host(scans, tmp_path / "m.jsonl", **kw)
    assert_counters(g, tmp_path / "m.jsonl", refs)
    assert_field(g, oracle_field(("carve16", semantics), scans, **kw))
    g.close()
    few, refs = S.refs_few_rays(sim, *S.CARVE_FEW, **ckw)
    S.assert_few_rays_nonvacuous(few, refs, ckw)
    kw["max_batch"] = 3
    g = run_host(few, tmp_path / "f.jsonl", **kw)
    assert_counters(g, tmp_path / "f.jsonl", refs, shards=False)
    assert_field(g, oracle_field(("carve16-few", semantics), few, **kw))
    g.close()


# ---- 5. a sector shard --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["seq3", "seq6"])
@pytest.mark.parametrize("rule", ["index", "world"])
def test_sector_shards(sim, tmp_path, rule, name):
    """Each of four sector contexts against the oracle's shard; rays and pairs of the shards add up
    to the unsharded context's, dirty and active do not (border voxels count twice).  vox adds up
    too as long as no voxel is sampled by two shards' rays of one scan: so it is on seq3 (3 x 4 096
    points; tests/test_stats_ref.py asserts it on the reference), and there the sum is asserted.
    seq6 (6 x 8 192 points, 12 288 rays per shard: every counter shard filled) has such voxels at
    the sector borders, and the shards' vox adds up to more, by the reference's count of them."""
    n = len(S.INPUTS[name][0])
    scans = S.scans_of(sim, name)
    whole = S.batch_refs(S.refs_numpy(sim, name, "vdbfusion_f64"), [n])[0][0]
    got, want_vox = [], 0
    for k in range(4):
        kw = dict(n_sectors=4, sector=k, sector_rule=rule, max_batch=n)
        refs = S.refs_oracle(sim, name, semantics="vdbfusion_f64", **kw)
        want_vox += sum(r.u_vox for r in refs)
        log = tmp_path / ("s%d.jsonl" % k)
        g = run_host(scans, log, **kw)
        assert_counters(g, log, refs, shards=name == "seq6")
        assert_field(g, oracle_field((name, rule, k), scans, **kw))
        g.close()
        got.append(read_log(log)[0])
    for k in ("rays", "pairs"):
        assert sum(r[k] for r in got) == whole[k], k
    assert sum(r["voxel_updates"] for r in got) == want_vox
    assert want_vox == whole["voxel_updates"] if name == "seq3" else want_vox > whole["voxel_updates"]
    assert sum(r["dirty_voxels"] for r in got) > whole["dirty_voxels"]
    assert sum(r["active_bricks"] for r in got) > whole["active_bricks"]


# ---- 6. a dense brick ---------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch,n", [(64, 64), (512, 130)])
@pytest.mark.parametrize("semantics", ["vdbfusion", "voxblox"])
def test_dense_brick(tmp_path, semantics, max_batch, n):
    """512 points at the voxel centres of one brick, n identical scans in ONE batch: every voxel of
    the brick has a cell in every scan, 512 n (voxel, scan) cells of one brick (32 768 at 64
    scans), which k_integrate counts window by window in the low half of a packed 32-bit scan
    word.  With 130 scans (max_batch 512) the windows split at 64 scans."""
    pts, org, want = S.dense_brick_scan()
    kw = dict(max_batch=max_batch, **S.sem_kw(semantics))
    r = S.scan_ref_oracle(pts, org, **kw)
    assert np.isin(want, r.vox).all() and np.unique(S.brick_of(want)).shape[0] == 1
    in_brick = int(np.count_nonzero(S.brick_of(r.vox) == S.brick_of(want)[0]))
    assert in_brick == 512
    scans = [(pts, org)] * n
    log = tmp_path / "m.jsonl"
    g = run_device(scans, log, **kw)
    w, _ = assert_counters(g, log, [r] * n, vacuity=False)
    assert len(w) == 1 and w[0]["voxel_updates"] == n * r.u_vox >= 512 * n
    assert w[0]["dirty_voxels"] == r.u_vox
    assert_field(g, oracle_field(("dense", semantics, n), scans, **kw))
    g.close()


# ---- 7. growth and replay -----------------------------------------------------------------------

@pytest.mark.parametrize("pipeline", [0, 2])
@pytest.mark.parametrize("max_batch", [1, 4])
def test_growth_and_replay(sim, tmp_path, max_batch, pipeline):
    """max_bricks = 64: batches fail, the pool grows, they are replayed.  A replayed batch counts
    once and a failed batch's partial counters do not leak: the committed records alone are the
    reference's and add up to the totals.  new_bricks of a replayed batch leaves out the bricks its
    failed run had already put in the pool (they stay there), so it is at most the reference's;
    `bricks` after a committed batch is exact, and assert_new_chain ties every line's new_bricks
    to the pool its run found."""
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    kw = dict(max_batch=max_batch, pipeline=pipeline, max_bricks=64)
    log = tmp_path / "m.jsonl"
    g = run_host(scans, log, **kw)
    want, _ = assert_counters(g, log, refs, new_exact=False, cap0=64)
    st = g.stats()
    assert st["n_grows"] >= 1 and st["n_replayed"] >= 1
    lines = read_log(log)
    bad = [r for r in lines if not r["committed"]]
    ok = [r for r in lines if r["committed"]]
    assert bad and all(r["committed"] is False for r in bad)
    assert sum(r["new_bricks"] for r in ok) <= st["n_bricks"] == want[-1]["bricks"]
    for k, t in (("rays", "n_rays_total"), ("voxel_updates", "n_voxels_total"),
                 ("dirty_voxels", "n_dirty_total")):
        assert sum(r[k] for r in ok) == st[t]
    # a failed run walks all its rays before it is given up: its record counts them, the totals
    # do not
    assert all(r["rays"] > 0 for r in bad) and sum(r["rays"] for r in lines) > st["n_rays_total"]
    assert_field(g, oracle_field(("seq6", "vdbfusion_f64"), scans, **kw))
    g.close()


def test_fixed_capacity_enomem(sim, tmp_path):
    """max_bricks_hard == max_bricks: the library's ordinary refusal.  Rays are counted in full,
    the pool is full, and the context goes on answering.  (vox and dirty there: DESIGN.md §18.)"""
    from tsdf_map import TsdfError, _abi
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    g = hip(max_bricks=64, max_bricks_hard=64, max_batch=4)
    g.set_metrics_log(tmp_path / "m.jsonl")
    for p, o in scans:
        g.integrate(p, o)
    with pytest.raises(TsdfError) as e:
        g.sync()
    assert e.value.code == _abi.TSDF_ENOMEM
    st = g.stats()  # the call after the error still returns stats
    want = S.totals(S.batch_refs(refs, [4, 2])[0])
    assert st["n_bricks"] == st["max_bricks"] == 64
    for k in ("n_rays_total", "n_scans", "n_batches", "n_points_in"):
        assert st[k] == want[k], k
    assert 0 < st["n_dirty_total"] <= st["n_voxels_total"] <= want["n_voxels_total"]
    ok = [r for r in read_log(tmp_path / "m.jsonl") if r["committed"]]
    assert [r["scans"] for r in ok] == [4, 2]
    for r in ok:
        assert_record_invariants(r)
        assert r["overflow"] != 0 and r["bricks"] == 64
    g.close()


# ---- 8. reset_stats -----------------------------------------------------------------------------

ZEROED = ("n_voxels_total", "n_rays_total", "n_dirty_total", "n_scans", "n_batches", "n_points_in")


@pytest.mark.parametrize("max_bricks", [1 << 15, 64])
def test_reset_stats(sim, tmp_path, max_bricks):
    """After two batches: the totals and the host's scan / batch / point counts are zero; growths,
    replays, the pool and its capacity stay; *_last stays the last batch's (tsdf_hip.h says so).
    One more batch then stands alone in the totals.  max_bricks 64: the same after growths."""
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    log = tmp_path / "m.jsonl"
    g = run_host(scans[:4], log, max_batch=2, max_bricks=max_bricks)
    exact = max_bricks > 64
    first, held = assert_counters(g, log, refs[:4], new_exact=exact, cap0=max_bricks)
    a = g.stats()
    assert (a["n_grows"] >= 1) == (not exact)
    g.reset_stats()
    b = g.stats()
    assert all(b[k] == 0 for k in ZEROED)
    for k in ("n_grows", "n_replayed", "n_bricks", "max_bricks", "n_voxels_last", "n_pairs_last",
              "n_active_last"):
        assert b[k] == a[k], k
    assert b["n_voxels_last"] == first[-1]["voxel_updates"] > 0
    for p, o in scans[4:]:
        g.integrate(p, o)
    g.sync()
    alone, _ = S.batch_refs(refs[4:], [2], held)
    c = g.stats()
    for k, v in S.totals(alone).items():
        assert c[k] == v, k
    assert 0 < alone[0]["new_bricks"] < alone[0]["active_bricks"]
    g.close()


def test_reset_stats_drains_the_queue_first(sim, tmp_path):
    """Two scans still queued (max_batch 3): reset_stats launches them, waits, then clears, so the
    totals are zero and *_last is that batch's."""
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    g = hip(max_batch=3)
    g.set_metrics_log(tmp_path / "m.jsonl")
    for p, o in scans[:2]:
        g.integrate(p, o)
    g.reset_stats()
    st = g.stats()
    want = S.batch_refs(refs[:2], [2])[0][0]
    assert all(st[k] == 0 for k in ZEROED)
    assert (st["n_voxels_last"], st["n_pairs_last"], st["n_active_last"], st["n_bricks"]) == \
        (want["voxel_updates"], want["pairs"], want["active_bricks"], want["bricks"])
    recs = read_log(tmp_path / "m.jsonl")
    assert len(recs) == 1 and recs[0]["dirty_voxels"] == want["dirty_voxels"]
    g.integrate(*scans[2])
    g.sync()
    alone, _ = S.batch_refs(refs[2:3], [1], np.unique(S.brick_of(np.concatenate(
        [r.vox for r in refs[:2]]))))
    st = g.stats()
    for k, v in S.totals(alone).items():
        assert st[k] == v, k
    g.close()


# ---- 9. after the map changed underneath --------------------------------------------------------

def twin_of(c, s, w, **kw):
    """A fresh oracle volume holding exactly these bricks."""
    o = S.oracle_volume(**kw)
    o.import_bricks(c, s, w)
    return o


def next_batch_after_change(g, twin, log, scans, refs, before):
    """The batch after a change: new_bricks and bricks against the map the twin holds."""
    held = S.bkey(twin.brick_coords())
    assert g.num_bricks() == held.shape[0]
    for p, o in scans:
        g.integrate(p, o)
        twin.integrate(p, o)
    want, _ = assert_counters(g, log, refs, held=held, before=before)
    assert 0 < want[0]["new_bricks"] < want[0]["active_bricks"]
    assert_field(g, twin.export_voxels())
    return want


@pytest.mark.parametrize("change", ["evict", "prune", "import", "merge"])
def test_after_the_map_changed(sim, tmp_path, change):
    """evict_outside and prune take bricks away, so the next batch finds them new again;
    import_bricks and merge_from (its own slot claims, k_merge_apply) add bricks, which are not new
    to a later batch."""
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    log = tmp_path / "m.jsonl"
    kw = dict(max_batch=2)
    g = run_host(scans[:4], log, **kw)
    before, held = assert_counters(g, log, refs[:4])
    o = S.oracle_volume()
    for p, org in scans[:4]:
        o.integrate(p, org)
    c, s, w = o.export_bricks()
    nxt, nref = scans[4:6], refs[4:6]
    plain = S.batch_refs(nref, [2], held)[0][0]  # the next batch had the map not changed
    if change == "evict":
        lo, hi = c.min(0).astype(np.int64), c.max(0).astype(np.int64) + 1
        hi[0] = int(np.median(c[:, 0]))
        keep = np.all((c >= lo) & (c < hi), axis=1)
        assert g.evict_outside(lo, hi, copy_out=False) == int((~keep).sum()) > 0
        twin = twin_of(c[keep], s[keep], w[keep])
    elif change == "prune":
        s, w = s.copy(), w.copy()
        s[w < 2.0] = np.float32(TAU)
        w[w < 2.0] = 0
        keep = (w > 0).reshape(len(c), -1).any(1)
        assert g.prune(2.0) == int((~keep).sum()) > 0
        twin = twin_of(c[keep], s[keep], w[keep])
    elif change == "import":
        o2 = S.oracle_volume()
        o2.integrate(*scans[5])
        c2, s2, w2 = o2.export_bricks()
        g.import_bricks(c2, s2, w2)
        twin = twin_of(c, s, w)
        twin.import_bricks(c2, s2, w2)
    else:  # an identity-pose merge of a second volume holding scan 5 alone
        src = hip()
        src.integrate(*scans[5])
        src.sync()
        st = g.merge_from(src, np.eye(4), mode="nearest")
        src.close()
        # every observed voxel of the source lands on itself: the map holds the union of the bricks
        union = np.union1d(S.bkey(c), refs[5].bricks)
        assert np.array_equal(np.sort(S.bkey(g.brick_coords())), union)
        assert st["new_bricks"] == union.shape[0] - len(c) > 0
        twin = twin_of(*g.export_bricks())  # (the merged field itself: tests/test_merge_gpu.py)
    want = next_batch_after_change(g, twin, log, nxt, nref, before)
    if change in ("import", "merge"):
        assert want[0]["new_bricks"] < plain["new_bricks"]
    else:
        assert want[0]["new_bricks"] > plain["new_bricks"]
    g.close()


# ---- an all-empty batch ---------------------------------------------------------------------------

@pytest.mark.parametrize("pipeline", [0, 1, 2])
@pytest.mark.parametrize("max_batch", [1, 2])
def test_empty_batches_between_real_ones(sim, tmp_path, max_batch, pipeline):
    """Scans without a point make batches without a block: no front end, no compaction.  Their
    lines count nothing, report the pool as it stands and no new brick; the batches around them
    are unmoved."""
    scans, refs = S.scans_of(sim, "seq6"), S.refs_numpy(sim, "seq6", "vdbfusion_f64")
    none = (np.zeros((0, 3), np.float32), scans[0][1])
    seq = scans[:max_batch] + [none] * max_batch + scans[max_batch:2 * max_batch] + [none] * max_batch
    sref = refs[:max_batch] + [S.empty_ref()] * max_batch + refs[max_batch:2 * max_batch] + \
        [S.empty_ref()] * max_batch
    log = tmp_path / "m.jsonl"
    g = run_host(seq, log, max_batch=max_batch, pipeline=pipeline)
    want, _ = assert_counters(g, log, sref, vacuity=False)
    assert [r["scans"] for r in want] == [max_batch] * 4
    for e, real in ((want[1], want[0]), (want[3], want[2])):
        assert e["bricks"] == real["bricks"] > 0 and e["new_bricks"] == e["active_bricks"] == 0
    assert 0 < want[2]["new_bricks"] < want[2]["active_bricks"]
    st = g.stats()
    assert st["n_voxels_last"] == st["n_pairs_last"] == st["n_active_last"] == 0
    assert_field(g, oracle_field(("seq6-empties", max_batch), seq))
    g.close()


# ---- 10. the metrics ring -----------------------------------------------------------------------

def test_metrics_ring_wrap(sim, tmp_path):
    """300 one-scan batches of 64 points with the log on and nothing that drains in between, then
    one sync.  emit_metrics writes the ids from max(metrics_next, end - METRIC_RING) to end, so a
    ring that wrapped before a drain would drop the ids below end - 256; launch() drains once
    METRIC_RING - 8 = 248 records are pending, so outside a replay none is ever dropped: all 300
    ids are there, in order, and every line is the reference's."""
    scans = []
    for k in range(300):
        p, o = sim.scan(k % 100)
        scans.append((np.ascontiguousarray(p[(k * 7) % 2048::2048]), o))
    assert all(p.shape[0] == 64 for p, _ in scans)
    refs = [S.scan_ref_numpy(p, o, "vdbfusion_f64") for p, o in scans]
    log = tmp_path / "m.jsonl"
    g = run_host(scans, log, max_batch=1)
    want, _ = assert_counters(g, log, refs, vacuity=False)
    ids = [r["batch"] for r in read_log(log)]
    assert ids == list(range(300)) and len(want) == 300
    assert S.METRIC_RING == 256 < len(ids)
    assert sum(1 for r in want if r["new_bricks"] == 0) > 0 < sum(r["new_bricks"] for r in want)
    o = S.oracle_volume()
    for p, org in scans:
        o.integrate(p, org)
    assert_field(g, o.export_voxels())
    g.close()
