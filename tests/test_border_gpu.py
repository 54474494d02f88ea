"""The multi-context read-out on the GPU (csrc/tsdf_border.hip and its transaction in
csrc/tsdf_capi.cpp) against tests/borderref.py, bit for bit: the border reduce by steps and through
tsdf_border_reduce_local on every built case and on integrated maps, abort, repeat, maps whose
layout has just changed, and the mesh halo.  All contexts are on device 0.

The reference runs on the library's own exports, which list held bricks without an observed voxel
too; the oracle twin lists a brick only while it is observed, so twins are compared as voxels."""
import ctypes as C

import numpy as np
import pytest
import torch

import borderref as B
from test_borderref import (CASE_SEM, SEM, TILE, check_tiles, make_scans, mc_tab, ora,
                            same_export)
from test_distributed import tri_set
from test_multigpu import emulated_reduce_host, voxels_equal_bitwise
from test_prune_gpu import cut_box
from tsdf_map import _abi

pytestmark = pytest.mark.gpu

VS, TAU = B.VS, B.TAU
SMALL = dict(max_bricks=256, max_points=4096, max_batch=2)
MAPS = dict(max_bricks=1 << 12, max_points=1 << 16, max_batch=2)
DEV = "cuda:0"


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume(VS, TAU, **kw)


def sharded(world, **kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume.sharded(world, VS, TAU, device_ids=[0] * world, **kw)


def close(vols):
    for v in vols:
        v.close()


def pack_all(vols, world):
    """keys -> pack for the live contexts `vols` (rank -> volume) of a world of `world` ranks:
    (sends per rank, splits (world, world))."""
    counts, keys = [0] * world, {}
    for r, v in vols.items():
        k = torch.empty(max(v.num_bricks(), 1), dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        counts[r] = v.brick_keys_into(k.data_ptr(), k.numel())
        keys[r] = k
    stride = max(max(counts), 1)
    allk = torch.full((world, stride), -1, dtype=torch.int64, device=DEV)
    for r in vols:
        allk[r, :counts[r]] = keys[r][:counts[r]]
    sends, splits = {}, np.zeros((world, world), np.int64)
    for r, v in vols.items():
        s = torch.empty((max(counts[r], 1), TILE), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        splits[r] = v.border_pack(allk.data_ptr(), counts, stride, world, r, s.data_ptr(),
                                  s.shape[0])
        sends[r] = s
    return sends, splits


def merge_all(vols, world, sends, splits, groups=None):
    """The exchange in torch and one border_merge per owner and group of source ranks (default:
    one call with every source, ascending)."""
    for d, v in vols.items():
        for group in groups or [range(world)]:
            parts, rc = [], [0] * world
            for r in group:
                if r not in vols or not splits[r, d]:
                    continue
                off = int(splits[r, :d].sum())
                parts.append(sends[r][off:off + int(splits[r, d])])
                rc[r] = int(splits[r, d])
            recv = torch.cat(parts).contiguous() if parts else \
                torch.empty((1, TILE), dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            v.border_merge(recv.data_ptr(), rc)


def reduce_steps(vols, world):
    sends, splits = pack_all(vols, world)
    merge_all(vols, world, sends, splits)
    for v in vols.values():
        v.border_commit(True)
    return splits


def assert_exports(vols, want, what=""):
    for r, v in vols.items():
        assert same_export(v.export_bricks(), want[r]), (what, r)


def filled(name, sem, make):
    """(live contexts {rank: volume}, exports, facts, cap, bg) of a case imported into contexts
    that `make(world, rank)` creates (only the ranks that hold a brick when world is 64)."""
    _, bg, cap = SEM[sem]
    exports, facts = B.case(name, bg)
    world = len(exports)
    live = [r for r in range(world) if world < 64 or len(exports[r][0])]
    vols = {r: make(world, r) for r in live}
    for r, v in vols.items():
        v.import_bricks(*exports[r])
        assert same_export(v.export_bricks(), exports[r])  # the case survives the import
    return vols, exports, facts, cap, bg


@pytest.mark.parametrize("name,sem", CASE_SEM)
def test_case_by_steps(name, sem):
    vols, exports, facts, cap, bg = filled(
        name, sem, lambda w, r: hip(n_sectors=w, sector=r, **SEM[sem][0], **SMALL))
    world = len(exports)
    if name == "one_chain":
        assert all(v.stats()["n_grows"] == 0 and v.stats()["max_bricks"] == facts["max_bricks"]
                   for v in vols.values())
    want, moved = B.reduce(exports, cap, bg)
    got = reduce_steps(vols, world)
    assert np.array_equal(got, B.splits(exports))
    assert got.sum() == moved
    assert_exports(vols, want)
    close(vols.values())


@pytest.mark.parametrize("name,sem", [c for c in CASE_SEM if c[0] != "high_ranks"])
def test_case_reduce_local(name, sem):
    from tsdf_map import border_reduce_local
    _, bg, cap = SEM[sem]
    world = len(B.case(name, bg)[0])
    g = sharded(world, **SEM[sem][0], **SMALL)
    vols, exports, facts, cap, bg = filled(name, sem, lambda w, r: g[r])
    want, moved = B.reduce(exports, cap, bg)
    assert border_reduce_local(g) == moved
    assert_exports(vols, want)
    close(g)


@pytest.mark.parametrize("name,sem,groups", [("fan_in", "vdbfusion_f64", [[1, 2, 3], [4, 5, 6, 7]]),
                                             ("capped", "voxblox_cap3", [[1], [2]]),
                                             ("one_chain", "vdbfusion_f64", [[1], [2]])])
def test_abort_after_two_merges(name, sem, groups):
    """Pack, two border_merge calls per owner (a brick held by every rank receives tiles in both:
    the second snapshot holds the first call's result), abort: every export is back to its bits.
    Then a full reduce gives the reference."""
    vols, exports, facts, cap, bg = filled(
        name, sem, lambda w, r: hip(n_sectors=w, sector=r, **SEM[sem][0], **SMALL))
    world = len(exports)
    sends, splits = pack_all(vols, world)
    assert all(sum(int(splits[r, 0]) for r in grp) > 0 for grp in groups)
    own = B.owners(exports)
    both = [{k for r in grp for k in B.keys_of(exports[r][0])[own[r] == 0].tolist()}
            for grp in groups]
    assert both[0] & both[1]  # a brick of rank 0 receives tiles in both calls
    merge_all(vols, world, sends, splits, groups)
    assert not same_export(vols[0].export_bricks(), exports[0])  # the owner merged
    for v in vols.values():
        v.border_commit(False)
    assert_exports(vols, exports, "abort")
    want, moved = B.reduce(exports, cap, bg)
    assert reduce_steps(vols, world).sum() == moved
    assert_exports(vols, want, "reduce after abort")
    close(vols.values())


@pytest.mark.parametrize("name,sem", [("fan_in", "voxblox"), ("capped", "voxblox_cap3"),
                                      ("one_chain", "vdbfusion_f64")])
def test_reduce_twice(name, sem):
    """The second reduce changes no bit; its splits are the first's, because the sent bricks are
    still held and travel again at W = 0."""
    vols, exports, facts, cap, bg = filled(
        name, sem, lambda w, r: hip(n_sectors=w, sector=r, **SEM[sem][0], **SMALL))
    world = len(exports)
    want, moved = B.reduce(exports, cap, bg)
    first = reduce_steps(vols, world)
    assert_exports(vols, want)
    again, moved2 = B.reduce(want, cap, bg)
    assert moved2 == moved and all(same_export(a, b) for a, b in zip(again, want))
    second = reduce_steps(vols, world)
    assert np.array_equal(second, first) and np.array_equal(second, B.splits(want))
    assert_exports(vols, want, "second")
    close(vols.values())


# ---- integrated maps ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scans(sim):
    return make_scans(sim, 8)


def integrate_both(g, o, scans):
    from tsdf_map import integrate_sectors
    for pts, pose in scans:
        integrate_sectors(g, pts, pose)
        for v in o:
            v.integrate(pts, pose)


def assert_twins(g, o, what=""):
    for r, (a, b) in enumerate(zip(g, o)):
        assert voxels_equal_bitwise(a.export_voxels(), b.export_voxels()), (what, r)


def reduce_and_check(g, o, sem, what=""):
    """border_reduce_local on g against the reference run on g's exports, and against the oracle
    twins' reduce; returns (the exports before, tiles moved)."""
    from tsdf_map import border_reduce_local
    _, bg, cap = SEM[sem]
    before = [v.export_bricks() for v in g]
    want, moved = B.reduce(before, cap, bg)
    assert border_reduce_local(g) == moved
    assert_exports(dict(enumerate(g)), want, what)
    emulated_reduce_host(o)
    assert_twins(g, o, what)
    return before, moved


@pytest.mark.parametrize("world", [3, 4])
@pytest.mark.parametrize("rule", ["world", "index"])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox", "voxblox_merged"])
def test_integrated_maps(scans, sem, rule, world):
    kw = dict(sector_yaw0=0.3, sector_rule=rule)
    g = sharded(world, **SEM[sem][0], **kw, **MAPS)
    o = [ora(sem, world, r, **kw) for r in range(world)]
    integrate_both(g, o, scans)
    _, moved = reduce_and_check(g, o, sem)
    assert moved > 50
    close(g)


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_reduce_after_prune(scans, sem):
    """Reduce, prune(0) everywhere (the sent bricks are empty and go: the pool compacts), a third
    scan, reduce again."""
    world = 3
    g = sharded(world, **SEM[sem][0], sector_yaw0=0.3, **MAPS)
    o = [ora(sem, world, r, sector_yaw0=0.3) for r in range(world)]
    integrate_both(g, o, scans[:2])
    reduce_and_check(g, o, sem, "first")
    held = [v.export_bricks() for v in g]
    empty = [B.as_export(e)[0][~B.observed(e)] for e in held]
    assert sum(map(len, empty)) > 50
    for v, e, gone in zip(g, held, empty):
        assert v.prune(0.0) == len(gone) and v.num_bricks() == len(e[0]) - len(gone)
    assert_twins(g, o, "prune")
    integrate_both(g, o, scans[2:])
    assert_twins(g, o, "third scan")
    before, moved = reduce_and_check(g, o, sem, "second")
    # had the emptied bricks stayed, they would have travelled again
    kept = []
    for e, gone in zip(before, empty):
        c, s, w = B.as_export(e)
        have = set(B.keys_of(c).tolist())
        extra = np.array([b for b in gone.tolist() if int(B.keys_of([b])[0]) not in have],
                         np.int32).reshape(-1, 3)
        zeros = np.zeros((len(extra), 512), np.float32)
        kept.append((np.concatenate([c, extra]), np.concatenate([s, zeros]),
                     np.concatenate([w, zeros])))
    assert moved < B.splits(kept).sum()
    close(g)


def evicted_twin(o, sem, world, rank, lo, hi, **kw):
    c, s, w = o.export_bricks()
    keep = np.all((c >= lo) & (c < hi), axis=1)
    t = ora(sem, world, rank, **kw)
    t.import_bricks(c[keep], s[keep], w[keep])
    return t


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_reduce_after_evict(scans, sem):
    """evict_outside on ranks 1 and 2 (the box cuts through their bricks: the pool compacts with
    moves and the table is rebuilt), then the reduce."""
    world = 3
    g = sharded(world, **SEM[sem][0], sector_yaw0=0.3, **MAPS)
    o = [ora(sem, world, r, sector_yaw0=0.3) for r in range(world)]
    integrate_both(g, o, scans[:2])
    for r in (1, 2):
        lo, hi = cut_box(g[r].export_bricks()[0])
        n0 = g[r].num_bricks()
        n_ev = g[r].evict_outside(lo, hi, copy_out=False)
        assert 0 < n_ev < n0 and g[r].num_bricks() == n0 - n_ev
        o[r] = evicted_twin(o[r], sem, world, r, lo, hi, sector_yaw0=0.3)
    assert_twins(g, o, "evict")
    _, moved = reduce_and_check(g, o, sem)
    assert moved > 20
    close(g)


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_reduce_after_growth(scans, sem):
    world = 3
    g = sharded(world, **SEM[sem][0], sector_yaw0=0.3, **dict(MAPS, max_bricks=128))
    o = [ora(sem, world, r, sector_yaw0=0.3) for r in range(world)]
    integrate_both(g, o, scans[:2])
    assert all(v.stats()["n_grows"] >= 2 for v in g)
    reduce_and_check(g, o, sem)
    close(g)


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_reduce_unsynced_pipeline(scans, sem):
    """pipeline = 2: a scan integrated and not synced, then tsdf_border_reduce_local at once.  The
    exports before the reduce come from contexts built alike and synced."""
    from tsdf_map import border_reduce_local, integrate_sectors
    world = 3
    _, bg, cap = SEM[sem]
    g = sharded(world, **SEM[sem][0], sector_yaw0=0.3, pipeline=2, **dict(MAPS, max_batch=4))
    h = sharded(world, **SEM[sem][0], sector_yaw0=0.3, **MAPS)
    o = [ora(sem, world, r, sector_yaw0=0.3) for r in range(world)]
    integrate_both(h, o, scans[:2])
    for pts, pose in scans[:2]:
        integrate_sectors(g, pts, pose)
    want, moved = B.reduce([v.export_bricks() for v in h], cap, bg)
    assert border_reduce_local(g) == moved
    assert_exports(dict(enumerate(g)), want)
    emulated_reduce_host(o)
    assert_twins(g, o)
    close(g + h)


# ---- halo and mesh -----------------------------------------------------------------------------

def halo_of(g, r, exports):
    """Context r's halo keys and the other contexts' answers, each checked against the reference;
    returns the halo tiles (device)."""
    world = len(g)
    need = B.halo_needed(exports[r])
    assert g[r].halo_keys_into(0, 0) == len(need) > 0
    keys = torch.empty(len(need), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert g[r].halo_keys_into(keys.data_ptr(), keys.numel()) == len(need)
    hk = keys.cpu().numpy()
    assert np.array_equal(hk.view(np.uint64), B.keys_of(need))
    tiles = []
    for j in range(world):
        if j == r:
            continue
        ak, as_, aw = B.halo_answer(exports[j], hk)
        send = torch.zeros((len(need), TILE), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        if len(ak):  # one row short: TSDF_EOVERFLOW with the count, and the context goes on
            n = C.c_uint64()
            rc = g[j]._lib.tsdf_halo_pack_device(g[j]._ctx, C.c_void_p(keys.data_ptr()), len(need),
                                                 C.c_void_p(send.data_ptr()), len(ak) - 1,
                                                 C.byref(n))
            assert rc == _abi.TSDF_EOVERFLOW and n.value == len(ak)
        n = g[j].halo_pack(keys.data_ptr(), len(need), send.data_ptr(), len(need))
        assert n == len(ak)
        if n:
            check_tiles(send[:n].cpu().numpy(), ak, as_, aw)
        tiles.append(send[:n])
    return torch.cat(tiles).contiguous()


@pytest.mark.parametrize("table", ["generated", "lorensen"])
def test_halo_and_mesh_on_corner_case(table):
    from tsdf_map import extract_mesh_local
    g = sharded(3, **SEM["vdbfusion_f64"][0], **SMALL)
    vols, exports, facts, cap, bg = filled("halo_corner", "vdbfusion_f64", lambda w, r: g[r])
    tab = mc_tab(table)
    field = B.union_field(exports)
    soups = []
    for r, v in enumerate(g):
        halo = halo_of(g, r, exports)
        torch.cuda.synchronize()
        got = v.extract_triangle_mesh(table=table, halo=(halo.data_ptr(), halo.shape[0]))[0]
        own = B.as_export(exports[r])[0][B.observed(exports[r])]
        want = B.rank_soup(field, own, VS, tab)
        assert want.shape[0] > 0 and np.array_equal(tri_set(got), tri_set(want)), r
        soups.append(got)
    rows = np.concatenate([tri_set(s) for s in soups])
    assert len(np.unique(rows, axis=0)) == len(rows)  # pairwise disjoint
    whole = extract_mesh_local(g, table=table)[0]
    assert whole.shape[0] == sum(s.shape[0] for s in soups)
    at = 0
    for r, s in enumerate(soups):
        assert np.array_equal(tri_set(whole[at:at + s.shape[0]]), tri_set(s)), r
        at += s.shape[0]
    assert_exports(vols, exports)  # the reduce inside moved nothing
    close(g)


@pytest.mark.parametrize("table", ["generated", "lorensen"])
def test_halo_and_mesh_on_integrated_map(sim, table):
    """Two scans (every 16th point), reduced, so that contexts hold sent bricks at (background, 0)
    beside the halo tiles of the same bricks: requests and answers against the reference, every
    context's soup against rank_soup of the union field, the soups disjoint, and
    extract_mesh_local their concatenation in context order."""
    from tsdf_map import extract_mesh_local
    world, sem = 3, "vdbfusion_f64"
    g = sharded(world, **SEM[sem][0], sector_yaw0=0.3, **MAPS)
    o = [ora(sem, world, r, sector_yaw0=0.3) for r in range(world)]
    integrate_both(g, o, make_scans(sim, 16)[:2])
    reduce_and_check(g, o, sem)
    exports = [v.export_bricks() for v in g]
    held_empty = [set(B.keys_of(B.as_export(e)[0][~B.observed(e)]).tolist()) for e in exports]
    field, tab, soups, shadowed = B.union_field(exports), mc_tab(table), [], 0
    for r, v in enumerate(g):
        halo = halo_of(g, r, exports)
        tiles = halo.cpu().numpy().view(np.uint32)
        keys = tiles[:, 1024].astype(np.uint64) | \
            (tiles[:, 1025].astype(np.uint64) << np.uint64(32))
        shadowed += len(held_empty[r] & set(keys.tolist()))
        torch.cuda.synchronize()
        got = v.extract_triangle_mesh(table=table, halo=(halo.data_ptr(), halo.shape[0]))[0]
        own = B.as_export(exports[r])[0][B.observed(exports[r])]
        want = B.rank_soup(field, own, VS, tab)
        assert want.shape[0] > 300 and np.array_equal(tri_set(got), tri_set(want)), r
        soups.append(got)
    assert shadowed >= 10  # halo tiles of bricks the context itself holds empty
    rows = np.concatenate([tri_set(s) for s in soups])
    assert len(np.unique(rows, axis=0)) == len(rows)
    whole = extract_mesh_local(g, table=table)[0]
    assert whole.shape[0] == sum(s.shape[0] for s in soups)
    at = 0
    for r, s in enumerate(soups):
        assert np.array_equal(tri_set(whole[at:at + s.shape[0]]), tri_set(s)), r
        at += s.shape[0]
    close(g)


def test_halo_pack_on_one_chain():
    """k_halo_pack's table_find down the wrapping chain: every context is asked for all 120 keys of
    the case's pool and for as many keys it does not hold, and answers with what it observes."""
    g = sharded(3, **SEM["vdbfusion_f64"][0], **SMALL)
    vols, exports, facts, cap, bg = filled("one_chain", "vdbfusion_f64", lambda w, r: g[r])
    pool = np.unique(np.concatenate([B.keys_of(e[0]) for e in exports]))
    absent = B.keys_of(B.coords_of(pool) + [0, 0, 200])
    ask = np.concatenate([pool, absent]).view(np.int64)
    keys = torch.from_numpy(ask).to(DEV)
    for r, v in enumerate(g):
        ak, as_, aw = B.halo_answer(exports[r], ask)
        assert len(ak) == 80
        send = torch.zeros((len(ask), TILE), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        assert v.halo_pack(keys.data_ptr(), len(ask), send.data_ptr(), len(ask)) == 80
        check_tiles(send[:80].cpu().numpy(), ak, as_, aw)
    close(g)
