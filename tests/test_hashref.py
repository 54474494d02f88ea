"""tests/hashref.py on the CPU: its constants against the sources, each builder's
stated facts recomputed another way, and the restated bundle key against the oracle's bundling
rule (the oracle does not use mix64).  No GPU."""
import os
import re

import numpy as np
import pytest

import hashref as H
import oracle
from conftest import REPO
from test_voxblox_merged import running_mean

CSRC = os.path.join(REPO, "noetic-slam_amd", "csrc")
F = np.float32
TAU = 0.15


def _source(name):
    txt = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", txt)


def _constant(txt, name):
    """The integer a source gives `name`: `constexpr <type> NAME = <int>;`, `1 << n`, or a
    `#define TSDF_NAME <int>` default behind `constexpr int NAME = TSDF_NAME;`."""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, txt)
    assert m, name
    v = m.group(1).strip()
    if re.fullmatch(r"TSDF_\w+", v):
        m = re.search(r"#define\s+%s\s+(\d+)" % v, txt)
        assert m, v
        v = m.group(1)
    m = re.fullmatch(r"(\d+)u?(?:\s*<<\s*(\d+))?", v)
    assert m, (name, v)
    return int(m.group(1)) << int(m.group(2) or 0)


def test_constants_are_the_sources():
    merged, device = _source("tsdf_merged.hip"), _source("tsdf_device.h")
    for name in ("MG_BSHIFT", "MG_PMAX", "MG_TAB", "MG_GM", "MG_GTHREADS", "MG_EPT", "MG_VOX_LIM"):
        assert getattr(H, name) == _constant(merged, name), name
    for name in ("RPB", "HCAP", "LDS_PROBES"):
        assert getattr(H, name) == _constant(device, name), name
    assert H.BRICK_KEY_BIAS == _constant(_source("brick_key.h"), "BRICK_KEY_BIAS")
    # the home rules' shifts and masks, as the sources write them
    ray = _source("tsdf_ray.h")
    assert "0xff51afd7ed558ccdull" in ray and "0xc4ceb9fe1a85ec53ull" in ray
    assert ray.count("k ^= k >> 33;") == 3
    assert "mix64(key) & T.mask" in ray
    assert "(mix64(key) >> 32) * (uint64_t)P) >> 32" in merged
    assert "(uint32_t)mix64(key) & (MG_TAB - 1u)" in merged
    for f in ("tsdf_kernels.hip", "tsdf_walk.hip"):
        assert "(uint32_t)(mix64(key) >> 40) & (HCAP - 1)" in _source(f), f
    assert "K.cap = next_pow2(2 * max_bricks);" in _source("tsdf_capi.cpp")


def test_mix64_known_answers():
    """MurmurHash3's 64-bit finaliser (public test values) in Python integers."""
    def ref(k):
        m = (1 << 64) - 1
        k ^= k >> 33
        k = k * 0xff51afd7ed558ccd & m
        k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 & m
        return k ^ k >> 33
    ks = [0, 1, 2, (1 << 63) | 12345, (1 << 64) - 1, H.brick_key([[-3, 7, 80]])[0]]
    got = H.mix64(np.array(ks, np.uint64))
    assert [int(x) for x in got] == [ref(int(k)) for k in ks]
    assert int(got[0]) == 0 and int(got[1]) == 0xb456bcfc34c2cb2c


def test_brick_key_is_the_codec():
    b = np.array([[0, 0, 0], [-1, 2, -3], [-(1 << 20), (1 << 20) - 1, 5]])
    k = H.brick_key(b)
    for ax in range(3):
        assert np.array_equal(((k >> np.uint64(21 * ax)) & np.uint64(0x1FFFFF)).astype(np.int64)
                              - (1 << 20), b[:, ax])


def naive_probe(homes, slots, limit=None):
    """Open addressing written out: (longest probe count, wrapped, dropped keys)."""
    tab = [False] * slots
    longest, wrapped, dropped = 0, False, 0
    for h in homes:
        q, n = int(h), 0
        while n < (limit or slots) and tab[q]:
            if q == slots - 1:
                wrapped = True
            q, n = (q + 1) % slots, n + 1
        if n == (limit or slots):
            dropped += 1
            longest = max(longest, n)
            continue
        tab[q] = True
        longest = max(longest, n + 1)
    return longest, wrapped, dropped


def test_probe_runs_is_plain_open_addressing():
    rng = np.random.default_rng(3)
    for slots, n, lim in ((16, 16, None), (16, 20, None), (64, 40, 8), (2048, 1500, 64)):
        homes = (rng.integers(0, 6, n) + slots - 3) % slots
        got = H.probe_runs(homes, slots, lim)
        longest, wrapped, dropped = naive_probe(homes, slots, lim)
        assert got[1] == longest and int((got[0] < 0).sum()) == dropped
        assert got[2] or not wrapped
        placed = got[0][got[0] >= 0]
        assert np.unique(placed).shape[0] == placed.shape[0]


def independent_bucket(pts, name):
    """The target bucket of a case, from float64 voxel indices and Python-int hashing of a sample
    plus np.unique on the restated keys."""
    kw = H.SPECS[name]
    mr = kw.get("max_range", np.inf)
    ok, key = H.merged_keys(pts, H.O, H.VS, max_range=mr, allow_clear=kw.get("allow_clear", True))
    ijk = np.floor(pts.astype(np.float64) / H.VS).astype(np.int64)
    depth = np.linalg.norm(pts.astype(np.float64) - np.array(H.O), axis=1)
    far = depth > mr
    assert np.array_equal(ok, ~far | kw.get("allow_clear", True))
    k2 = H.voxel_key(ijk, far)
    assert np.array_equal(key[ok], k2[ok])
    b = H.mg_bucket(k2, 4)
    return k2[ok & (b == 0)], k2[ok]


@pytest.mark.parametrize("name", sorted(H.SPECS))
def test_bucket_cloud_has_what_it_is_meant_to_test(name):
    pts, f = H.spec_cloud(name)
    kw = H.SPECS[name]
    assert pts.shape == (H.N_SCAN, 3) and pts.dtype == F and f["P"] == 4
    d = H.depth_of(pts, H.O)
    assert pts[:, 0].min() >= H.X_LO - 0.01 and pts[:, 0].max() <= H.X_HI + 0.01
    # no point within a millimetre of the range limit (fp32 depths are good to a micrometre)
    assert np.all(np.abs(d - F(kw.get("max_range", 1e9))) > 1e-3)
    assert f["straddled"] == kw.get("straddle", 0) * (kw.get("allow_clear", True) is True)
    mine, allk = independent_bucket(pts, name)
    uniq, cnt = np.unique(mine, return_counts=True)
    assert f["entries"] == mine.shape[0] and f["keys"] == uniq.shape[0]
    assert f["members"] == int(cnt[cnt > 1].sum()) and f["bundles"] == int((cnt > 1).sum())
    assert f["keys_total"] == np.unique(allk).shape[0]
    spec = kw["spec"]
    dropped = kw.get("allow_clear", True) is False
    if not dropped:  # the bucket holds exactly the prescribed multiset; the rest are singletons
        assert f["entries"] == sum(k * m for k, m in spec) and f["valid"] == H.N_SCAN
        assert f["keys"] == sum(k for k, _ in spec)
        want = np.sort(np.concatenate([np.full(k, m) for k, m in spec if m > 1] + [[]]))
        assert np.array_equal(f["sizes"], want)
        # (a voxel cut by max_range: four points in two keys of the other buckets)
        assert f["keys_total"] == H.N_SCAN - f["members"] + f["bundles"] - 2 * kw.get("straddle", 0)
    else:
        assert f["clearing_keys"] == 0 and f["valid"] < H.N_SCAN
    assert f["keys"] <= H.MG_TAB or name == "overflow"
    assert f["placed"] == min(f["keys"], H.MG_TAB)
    # members are interleaved with other bundles' members in cloud order
    if f["bundles"] > 1:
        _, key = H.merged_keys(pts, H.O, H.VS, max_range=kw.get("max_range", np.inf))
        k = uniq[cnt > 1][0]
        at = np.flatnonzero(key == k)
        assert at[-1] - at[0] > len(at)
    # the naive simulation of the table, in the same order
    _, first = np.unique(mine, return_index=True)
    homes = H.mg_home(mine[np.sort(first)])
    longest, wrapped, drop = naive_probe(homes, H.MG_TAB)
    assert f["longest_probe"] == longest and f["wraps"] == wrapped
    assert drop == max(0, f["keys"] - H.MG_TAB)
    if name == "wrap":
        assert np.all((homes >= H.MG_TAB - 8)) and f["wraps"] and f["longest_probe"] >= 1790
    if name in ("clearing",):
        assert f["clearing_keys"] == round(sum(k for k, _ in spec) / 3)
    if name == "full-table":
        assert f["keys"] == H.MG_TAB and f["members"] == 0 and f["entries"] > H.MG_REG
    if name == "overflow":
        assert f["keys"] == H.MG_TAB + 1
    if name.startswith("rank"):
        assert f["members"] == int(name[5:]) and f["entries"] <= H.MG_REG
    if name == "bitonic-many":
        assert f["members"] == H.MG_GM and f["bundles"] > 500 and f["entries"] > H.MG_REG
    if name.startswith("walk"):
        assert f["members"] == int(name[5:]) > H.MG_GM and f["bundles"] > 500


def ora(**kw):
    return oracle.OracleTSDFVolume(H.VS, TAU, semantics="voxblox", **kw)


@pytest.mark.parametrize("name", sorted(H.SPECS))
def test_oracle_bundles_by_the_restated_key(name):
    """The oracle's ray count on the case's cloud is the restatement's count of distinct valid
    keys; and (constant weights) a multi-point bundle alone is one ray of weight m whose voxels are
    those of the Simple ray to running_mean of its members in cloud order."""
    pts, f = H.spec_cloud(name)
    kw = {k: v for k, v in H.SPECS[name].items() if k in ("max_range", "allow_clear")}
    o = ora(method="merged", use_const_weight=True, **kw)
    o.integrate(pts, np.array(H.O))
    assert o.stats()["n_rays_total"] == f["keys_total"]
    assert o.stats()["n_points_in"] == H.N_SCAN
    o.close()
    if not f["bundles"]:
        return
    ok, key = H.merged_keys(pts, H.O, H.VS, **kw)
    near = ok & ((key >> np.uint64(63)) == 0) & (H.mg_bucket(key, 4) == 0)
    uniq, cnt = np.unique(key[near], return_counts=True)
    o32 = np.array(H.O).astype(F)
    for m in sorted(set(cnt[cnt > 1].tolist()))[:4]:
        k = uniq[cnt == m][0]
        grp = pts[key == k]
        a = ora(method="merged", use_const_weight=True, use_weight_dropoff=False, **kw)
        a.integrate(grp, np.array(H.O))
        assert a.stats()["n_rays_total"] == 1
        ai, _, aw = a.export_voxels()
        mean, mw = running_mean(grp - o32, [1] * m)
        assert mw == m and np.all(aw == F(m)) and ai.shape[0] > 3
        s = ora(use_const_weight=True, use_weight_dropoff=False, **kw)
        s.integrate((o32 + mean).astype(F)[None], np.array(H.O))
        si, _, sw = s.export_voxels()
        assert np.array_equal(ai, si) and np.all(sw == 1)
        a.close()
        s.close()


@pytest.mark.parametrize("bits,n", [(7, 60), (10, 250), (11, 300)])
def test_chain_bricks_stay_at_the_tables_end(bits, n):
    c, f = H.chain_bricks(n, bits)
    assert c.shape == (n, 3) and np.abs(c).max() <= 80
    assert np.unique(c, axis=0).shape[0] == n
    key = H.brick_key(c)
    for m in range(3, bits + 1):  # every table the set can meet on its way up
        slots = 1 << m
        home = [int(x) % slots for x in H.mix64(key)]
        assert min(home) >= slots - 8, m
        longest, wrapped, dropped = naive_probe(home, slots)
        assert wrapped and dropped == max(0, n - slots)
        if n <= slots:
            assert longest >= n // 8
    assert f["in_tail"] == n and f["wraps"] and f["longest_probe"] >= n // 8
    assert H.table_mask(64) == 127 and H.table_mask(1024) == 2047 and H.table_mask(65) == 255


@pytest.mark.parametrize("anchor", [0, 700, H.HCAP - 8], ids=["low", "mid", "end"])
def test_lds_chain_cloud_crowds_one_window(anchor):
    window = 8 if anchor == H.HCAP - 8 else 16
    pts, f = H.lds_chain_cloud(200, window, anchor=anchor)
    assert pts.shape == (H.RPB, 3) and pts.dtype == F
    b = np.floor(pts.astype(np.float64) / H.VS).astype(np.int64) >> 3
    ub = np.unique(b, axis=0)
    assert ub.shape[0] == 200 == f["bricks"] == f["in_window"]
    assert np.abs(ub).max() <= 80 and np.abs(ub).max(axis=1).min() >= 6
    home = np.array([(int(x) >> 40) % H.HCAP for x in H.mix64(H.brick_key(ub))])
    assert np.all((home - anchor) % H.HCAP < window)
    # bounded probing: at most window + LDS_PROBES - 1 keys find a slot, whatever the order
    assert f["must_fall"] == 200 - (window + H.LDS_PROBES - 1) >= 100
    for order in (np.arange(200), np.random.default_rng(1).permutation(200)):
        longest, wrapped, dropped = naive_probe(home[order], H.HCAP, H.LDS_PROBES)
        assert dropped >= f["must_fall"] and longest == H.LDS_PROBES
        assert wrapped == (anchor == H.HCAP - 8)
        longest, wrapped, dropped = naive_probe(home[order], H.HCAP)
        assert dropped == 0 and longest > 180 and wrapped == (anchor == H.HCAP - 8)
    assert f["fell"] >= f["must_fall"] and f["wraps"] == (anchor == H.HCAP - 8)
    assert f["wraps_full"] == (anchor == H.HCAP - 8) and f["longest_full"] > 180
