"""tests/borderref.py (the border reduce and the mesh halo in numpy) against the CPU oracle twin,
the builders' conditions on the reference alone, and a reduced map against the one-context map
(DESIGN.md §22).  tests/test_border_gpu.py holds the GPU library to the same reference.

The oracle keeps voxels, not bricks: it lists a brick only while one of its voxels is observed
(oracle/tsdf_oracle.c, "border-brick reduce"), so a brick it sent drops out of its export where
the library goes on holding it at (background, 0).  The comparisons below are therefore on the
observed bricks of the reference's result, and the reference runs on the oracle's own exports."""
import numpy as np
import pytest

import borderref as B
import meshref
import oracle
from test_distributed import tri_set
from test_multigpu import emulated_reduce_host
from tsdf_map import _abi, bricks_to_voxels

VS, TAU = B.VS, B.TAU
TILE = 1028

# semantics name -> (volume keywords, background, merge cap)
SEM = {
    "vdbfusion_f64": (dict(semantics="vdbfusion_f64"), TAU, np.inf),
    "vdbfusion": (dict(semantics="vdbfusion"), TAU, np.inf),
    "voxblox": (dict(semantics="voxblox"), 0.0, 10000.0),
    "voxblox_cap3": (dict(semantics="voxblox", max_weight=3.0), 0.0, 3.0),
    "voxblox_const": (dict(semantics="voxblox", use_const_weight=True), 0.0, 10000.0),
    "voxblox_merged": (dict(semantics="voxblox", method="merged"), 0.0, 10000.0),
}
# case -> the semantics it runs under
CASE_SEM = [("fan_in", "vdbfusion_f64"), ("fan_in", "voxblox"), ("paths", "vdbfusion_f64"),
            ("paths", "voxblox"), ("capped", "voxblox_cap3"), ("empty_ranks", "vdbfusion_f64"),
            ("all_empty", "vdbfusion_f64"), ("high_ranks", "vdbfusion_f64"),
            ("one_chain", "vdbfusion_f64"), ("halo_corner", "vdbfusion_f64")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_export(a, b):
    a, b = B.as_export(a), B.as_export(b)
    return (np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
            and np.array_equal(bits(a[2]), bits(b[2])))


def observed_only(e):
    c, s, w = B.as_export(e)
    k = B.observed(e)
    return c[k], s[k], w[k]


def ora(sem, world, rank, **kw):
    return oracle.OracleTSDFVolume(VS, TAU, n_sectors=world, sector=rank, **SEM[sem][0], **kw)


def check_reduce_on_oracle(vols, sem):
    """Reduce oracle contexts by steps; splits, tiles moved and exports against the reference."""
    _, bg, cap = SEM[sem]
    before = [v.export_bricks() for v in vols]
    want, moved = B.reduce(before, cap, bg)
    got = emulated_reduce_host(vols)
    assert np.array_equal(np.array(got, np.int64), B.splits(before))
    assert sum(map(sum, got)) == moved
    for r, v in enumerate(vols):
        assert same_export(v.export_bricks(), observed_only(want[r])), r
    return before, want, moved


@pytest.mark.parametrize("name,sem", CASE_SEM)
def test_reference_equals_oracle_on_cases(name, sem):
    exports, facts = B.case(name, SEM[sem][1])
    world = len(exports)
    vols = [ora(sem, world, r) for r in range(world)]
    for v, e in zip(vols, exports):
        v.import_bricks(*e)
        assert same_export(v.export_bricks(), e)  # the case survives the import bit for bit
    _, _, moved = check_reduce_on_oracle(vols, sem)
    assert moved == B.splits(exports).sum()
    check_reduce_on_oracle(vols, sem)  # again: nothing observed is left to move


def make_scans(sim, every):
    """Scans 0, 3 and 6 of the simulator with poses, every `every`-th point."""
    out = []
    for k in (0, 3, 6):
        pts, org = sim.scan(k)
        pose = np.concatenate([org, [0.0, 0.0, np.sin(0.05 * k), np.cos(0.05 * k)]])
        out.append((np.ascontiguousarray(pts[::every]), pose))
    return out


@pytest.fixture(scope="module")
def scans(sim):
    return make_scans(sim, 4)


def mc_tab(table):
    return meshref.mc_table(oracle.load(), _abi.MC_TABLES[table])


@pytest.mark.parametrize("rule", ["world", "index"])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox", "voxblox_merged"])
def test_reference_equals_oracle_on_scans(scans, sem, rule):
    world = 3
    vols = [ora(sem, world, r, sector_yaw0=0.3, sector_rule=rule) for r in range(world)]
    for pts, pose in scans[:2]:
        for v in vols:
            v.integrate(pts, pose)
    _, want, moved = check_reduce_on_oracle(vols, sem)
    assert moved > 50
    # the halo requests and answers of the reduced contexts
    post = [v.export_bricks() for v in vols]
    for r, v in enumerate(vols):
        need = B.halo_needed(post[r])
        keys = np.empty(max(len(need), 1), np.int64)
        assert v.halo_keys_into(keys.ctypes.data, keys.size) == len(need)
        assert np.array_equal(keys[:len(need)].view(np.uint64), B.keys_of(need))
        j = (r + 1) % world
        hk, hs, hw = B.halo_answer(post[j], keys[:len(need)])
        send = np.empty((max(len(need), 1), TILE), np.int32)
        n = vols[j].halo_pack(keys.ctypes.data, len(need), send.ctypes.data, send.shape[0])
        assert n == len(hk) and n > 0
        check_tiles(send[:n], hk, hs, hw)


@pytest.mark.parametrize("table", ["generated", "lorensen"])
def test_rank_soups_on_scans(sim, table):
    """Two scans (every 16th point), reduced: every context's soup against rank_soup of the
    union field, and the soups disjoint."""
    world = 3
    vols = [ora("vdbfusion_f64", world, r, sector_yaw0=0.3) for r in range(world)]
    for pts, pose in make_scans(sim, 16)[:2]:
        for v in vols:
            v.integrate(pts, pose)
    assert sum(map(sum, emulated_reduce_host(vols))) > 50
    post = [v.export_bricks() for v in vols]
    field, tab, soups, n_halo = B.union_field(post), mc_tab(table), [], 0
    for r, v in enumerate(vols):
        need = B.halo_needed(post[r])
        keys = B.keys_of(need).view(np.int64)
        halo = []
        for j in range(world):
            if j != r:
                send = np.empty((len(need), TILE), np.int32)
                n = vols[j].halo_pack(keys.ctypes.data, len(need), send.ctypes.data, len(need))
                halo.append(send[:n])
        halo = np.ascontiguousarray(np.concatenate(halo))
        n_halo += halo.shape[0]
        got = v.extract_triangle_mesh(table=table, halo=(halo.ctypes.data, halo.shape[0]))[0]
        want = B.rank_soup(field, post[r][0], VS, tab)
        assert want.shape[0] > 300 and np.array_equal(tri_set(got), tri_set(want)), r
        soups.append(tri_set(got))
    rows = np.concatenate(soups)
    assert len(np.unique(rows, axis=0)) == len(rows)
    print("halo tiles", n_halo, "triangles", len(rows))
    assert n_halo >= 20  # cubes that read another rank's brick exist


def check_tiles(tiles, keys, s, w):
    """Tiles (n, 1028) int32 in any row order against the reference's answer sorted by key."""
    t = np.ascontiguousarray(tiles).view(np.uint32)
    k = t[:, 1024].astype(np.uint64) | (t[:, 1025].astype(np.uint64) << np.uint64(32))
    o = np.argsort(k)
    assert np.array_equal(k[o], keys)
    assert np.array_equal(t[o, :512], bits(s)) and np.array_equal(t[o, 512:1024], bits(w))
    assert not t[:, 1026:].any()


@pytest.mark.parametrize("table", ["generated", "lorensen"])
def test_halo_and_rank_soups_on_oracle(table):
    """halo_corner on the oracle: requests, answers and every context's soup."""
    exports, facts = B.case("halo_corner", TAU)
    world = len(exports)
    vols = [ora("vdbfusion_f64", world, r) for r in range(world)]
    for v, e in zip(vols, exports):
        v.import_bricks(*e)
    tab = mc_tab(table)
    field = B.union_field(exports)
    soups = []
    for r, v in enumerate(vols):
        need = B.halo_needed(exports[r])
        assert all(max(b) <= B.TOP for b in need.tolist()) and len(need) > 0
        keys = np.empty(len(need), np.int64)
        assert v.halo_keys_into(keys.ctypes.data, keys.size) == len(need)
        assert np.array_equal(keys.view(np.uint64), B.keys_of(need))
        halo = []
        for j in range(world):
            if j == r:
                continue
            hk, hs, hw = B.halo_answer(exports[j], keys)
            send = np.empty((len(need), TILE), np.int32)
            n = vols[j].halo_pack(keys.ctypes.data, len(need), send.ctypes.data, len(need))
            assert n == len(hk)
            check_tiles(send[:n], hk, hs, hw)
            halo.append(send[:n])
        halo = np.ascontiguousarray(np.concatenate(halo))
        got = v.extract_triangle_mesh(table=table, halo=(halo.ctypes.data, halo.shape[0]))[0]
        own = B.as_export(exports[r])[0][B.observed(exports[r])]
        want = B.rank_soup(field, own, VS, tab)
        assert want.shape[0] > 0
        assert np.array_equal(tri_set(got), tri_set(want)), r
        soups.append(tri_set(got))
    rows = np.concatenate(soups)
    assert len(np.unique(rows, axis=0)) == len(rows)  # no triangle twice: the soups are disjoint


# ---- the cases are what they are meant to be (on the reference alone) ----------------------------

def test_fan_in_depends_on_the_merge_order():
    exports, facts = B.case("fan_in")
    assert len(exports) == 8 and facts["bricks"] == 24
    held = {}
    for r, e in enumerate(exports):
        for b in e[0].tolist():
            held.setdefault(tuple(b), []).append(r)
    assert sum(h == list(range(8)) for h in held.values()) == 6
    assert sum(h == [1, 4, 7] for h in held.values()) == 6 and len(held) == 24
    a, moved = B.reduce(exports)
    b, _ = B.reduce_in_order(exports, range(7, -1, -1))
    diff = sum(int((bits(x[1]) != bits(y[1])).sum()) for x, y in zip(a, b))
    assert diff >= 50
    assert all(np.array_equal(x[2] > 0, y[2] > 0) for x, y in zip(a, b))
    own = B.owners(exports)
    assert set(own[4].tolist()) >= {0, 1} and 3 not in own[4].tolist()  # 4 never sends to 3


def test_paths_holds_every_combination():
    exports, facts = B.case("paths")
    combo = facts["combo"]
    for k in range(1, 8):
        assert (combo == k).sum() >= 200, k
    assert all(np.array_equal(e[2] > 0, (combo >> r) & 1 == 1) for r, e in enumerate(exports))
    # voxels the owner copies (first observed at source 1: combinations 2 and 6; at source 2: 4):
    # a mean run over them, (s w) / w, would not return s
    wrong = 0
    for src, at in ((1, (combo == 2) | (combo == 6)), (2, combo == 4)):
        _, s, w = exports[src]
        with np.errstate(invalid="ignore", divide="ignore"):
            back = (s * w) / w
        wrong += int((at & (bits(back) != bits(s))).sum())
    assert wrong >= 100
    copied, s1 = combo == 2, exports[1][1]
    out, _ = B.reduce(exports)
    assert np.array_equal(bits(out[0][1])[copied], bits(s1)[copied])


def test_capped_reaches_the_cap_on_both_sides():
    exports, facts = B.case("capped")
    cap = np.float32(facts["max_weight"])
    w0, w1, w2 = (e[2] for e in exports)
    assert max(w.max() for w in (w0, w1, w2)) <= cap
    both = (w0 > 0) & (w1 > 0)
    first = w0 + w1
    assert (both & (first > cap) & (w2 > 0)).sum() >= 20  # capped before the second source
    out, _ = B.reduce(exports, cap, 0.0)
    W = out[0][2]
    n_src = (w0 > 0).astype(int) + (w1 > 0) + (w2 > 0)
    total = w0.astype(np.float64) + w1 + w2
    assert ((n_src >= 2) & (W == cap) & (total > cap)).sum() >= 100
    assert ((n_src >= 2) & (W < cap)).sum() >= 100
    assert W.max() == cap
    free, _ = B.reduce(exports, np.inf, 0.0)
    assert free[0][2].max() > cap  # the cap is what holds the weights down


def test_empty_and_high_ranks_are_what_they_say():
    exports, facts = B.case("empty_ranks")
    assert [len(e[0]) for e in exports] == [0, 7, 0, 7]
    sp = B.splits(exports)
    assert sp[3, 1] == 4 and sp.sum() == 4 and not sp[0].any()
    exports, _ = B.case("all_empty")
    assert not B.splits(exports).any() and B.reduce(exports)[1] == 0
    exports, facts = B.case("high_ranks")
    assert [r for r, e in enumerate(exports) if len(e[0])] == [0, 31, 63]
    sp = B.splits(exports)
    assert sp[31, 0] == 3 and sp[63, 0] == 2 and sp[63, 31] == 2 and sp.sum() == 7


def test_one_chain_is_one_wrapping_chain():
    import hashref
    from test_hashref import naive_probe
    exports, facts = B.case("one_chain")
    assert facts["max_bricks"] == 256 and facts["mask"] == 511
    for e, f in zip(exports, facts["facts"]):
        home = hashref.table_home(B.keys_of(e[0]), facts["mask"])
        assert np.all(home >= 512 - 8)
        longest, wrapped, dropped = naive_probe(home, 512)
        assert wrapped and dropped == 0 and longest >= 70
        assert f["wraps"] and f["in_tail"] == 80
    sp = B.splits(exports)
    assert sp.sum() >= 80 and sp[2, 1] > 0 and sp[2, 0] > 0 and sp[1, 0] > 0


def test_halo_corner_spans_three_ranks():
    exports, facts = B.case("halo_corner")
    assert B.corner_cube_ranks(exports, facts["corner"] - 1) == {0, 1, 2}
    own = {tuple(b): r for r, e in enumerate(exports) for b in e[0].tolist()}
    assert {own[tuple(b)] for b in facts["around"].tolist()} == {0, 1, 2}
    top = tuple(facts["top"].tolist())
    assert top[0] == B.TOP and own[top] == 1
    need = B.halo_needed(exports[1])  # the top brick asks for no neighbour past the key range
    assert need[:, 0].max() == B.TOP and (need[:, 0] == B.TOP).sum() == 3
    # near the origin fp32 resolves a vertex's place inside its voxel (at x = TOP it would not)
    assert np.spacing(np.float32(8 * 3 * VS)) < 1e-4 * VS < np.spacing(np.float32(8 * B.TOP * VS))


# ---- a reduced map against the one-context map (measured on the oracle) ----------

ROWS = ["vdbfusion_f64", "vdbfusion", "voxblox_const", "voxblox", "voxblox_merged"]


@pytest.mark.parametrize("rule", ["world", "index"])
@pytest.mark.parametrize("sem", ROWS)
def test_reduced_map_against_single_context(scans, sem, rule, capsys):
    world = 3
    vols = [ora(sem, world, r, sector_yaw0=0.3, sector_rule=rule) for r in range(world)]
    ref = oracle.OracleTSDFVolume(VS, TAU, **SEM[sem][0])
    for pts, pose in scans:
        for v in vols + [ref]:
            v.integrate(pts, pose)
    emulated_reduce_host(vols)
    parts = [v.export_bricks() for v in vols]
    coords = np.concatenate([p[0] for p in parts])
    assert len({tuple(b) for b in coords.tolist()}) == len(coords)  # each brick on one rank
    mi, ms, mw = bricks_to_voxels(coords, np.concatenate([p[1] for p in parts]),
                                  np.concatenate([p[2] for p in parts]))
    ri, rs, rw = ref.export_voxels()
    same_set = np.array_equal(mi, ri)
    if same_set:
        share, dw, ds = float(np.mean(mw != rw)), float(np.abs(mw - rw).max()), \
            float(np.abs(ms - rs).max())
    else:
        a = {tuple(v): n for n, v in enumerate(mi.tolist())}
        both = [(a[tuple(v)], n) for n, v in enumerate(ri.tolist()) if tuple(v) in a]
        ia, ib = np.array(both).T
        share, dw, ds = float(np.mean(mw[ia] != rw[ib])), float(np.abs(mw[ia] - rw[ib]).max()), \
            float(np.abs(ms[ia] - rs[ib]).max())
    with capsys.disabled():
        print("\nreduced-vs-single %-15s %-5s voxels %s (%d / %d)  W differs %.3g  max|dW| %.3g  "
              "max|dS| %.3g" % (sem, rule, "equal" if same_set else "DIFFER", len(mi), len(ri),
                                share, dw, ds))
    if sem.startswith("vdbfusion"):
        assert same_set and share == 0.0 and ds <= 1e-5
    if sem == "voxblox_merged" and rule == "index":
        # every context bundles its own share: a voxel with points on both sides of a share
        # boundary casts two rays.  share > 0 alone would not tell (sums in another order differ
        # in W too, by a few ulps: W stays below 2^7 here, an ulp is at most 7.7e-6); a split
        # bundle moves whole ray weights between voxels, or observes another voxel
        assert share > 0.0 and (not same_set or dw > 1e-4)
