"""The integrate path (k_count / k_place, k_walk / k_spans, k_integrate / k_integrate_small, the
Merged pre-pass) against the CPU oracle, bit for bit, across band widths, voxel sizes and worst-case
rays.  The band, 2 * sdf_trunc / voxel_size, decides the pair and sample slots of a ray, which
body k_count and k_place take, whether the single walk runs and on how many register slots
(noetic-slam_amd/csrc/ctx_plan.h); tests/bandref.py holds the grid of bands at which each of these
changes and the adversarial rays, tests/test_band_inputs.py proves on the CPU that the rays are
what they claim and stay inside the plan's bounds.

Equality is the voxel set, the weight bits and the sdf bits of export_voxels(); in every case
sync() succeeds (an exceeded per-ray bound, OVF_PAIRS, would fail it) and nothing grows that
fits.  Contexts are small (2^14 points, 2^14 bricks); an oracle field is computed once per
parameter set."""
import numpy as np
import pytest

import bandref as B
from conftest import decimate

pytestmark = pytest.mark.gpu

F = np.float32
CTX = dict(max_points=1 << 14, max_bricks=1 << 14)
ENTRIES = [pytest.param(g, id="%g-%.11g" % g) for g in B.GRID]

# name -> (parameters, whether its scans carry a tilted pose)
VARIANTS = {
    "vdbfusion": (dict(semantics="vdbfusion"), False),
    "vdbfusion_f64": (dict(semantics="vdbfusion_f64"), False),
    "voxblox_const": (dict(semantics="voxblox", use_const_weight=True), False),
    "voxblox_z2": (dict(semantics="voxblox", use_const_weight=False), True),
    "voxblox_merged": (dict(semantics="voxblox", method="merged"), True),
}


def hip(entry, **kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume(entry[0], entry[1], **{**CTX, **kw})


def scans_of(entry, scan0, posed, seeds=(0,), reach=6.0):
    """The adversarial scans of the entry and every 16th point of the simulated scene's scan."""
    scans = [s for seed in seeds for s in B.adversarial_rays(*entry, seed=seed, reach=reach)]
    scans.append((decimate(scan0[0], 16), scan0[1]))
    return B.tilted(scans) if posed else scans


_ref = {}


def oracle_ref(key, entry, scans, last=1, **kw):
    """The oracle after `scans`: its field, rays kept, bricks, and the pairs of the last `last`
    scans (the sum of their rays' brick runs) -- once per key."""
    if key not in _ref:
        o = B.oracle_volume(*entry, **kw)
        for p, e in scans:
            o.integrate(p, e)
        field = o.export_voxels()
        for a in field:
            a.setflags(write=False)
        facts = [B.ray_facts(o, s) for s in scans]
        assert o.stats()["n_rays_total"] == sum(f.kept for f in facts)
        _ref[key] = dict(field=field, rays=sum(f.kept for f in facts), bricks=o.num_bricks(),
                         pairs_last=int(sum(f.runs.sum() for f in facts[-last:])))
        o.close()
    return _ref[key]


def assert_bitwise(g, ref):
    gi, gs, gw = g.export_voxels()
    oi, os_, ow = ref
    assert gi.shape == oi.shape, (gi.shape, oi.shape)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gw.view(np.uint32), ow.view(np.uint32))
    bad = np.flatnonzero(gs.view(np.uint32) != os_.view(np.uint32))
    assert bad.size == 0, "sdf differs at %d voxels, e.g. %s: gpu %r oracle %r" % (
        bad.size, gi[bad[:3]].tolist(), gs[bad[:3]].tolist(), os_[bad[:3]].tolist())
    return gi.shape[0]


def assert_quiet(g, ref=None):
    """sync() succeeded (the caller ran it) and no capacity had to grow -- unless the oracle's map
    holds more bricks than the context's initial pool (the 2 cm entries): then the context grew, by
    the library's own path, and the field still has to be the oracle's."""
    st = g.stats()
    if ref is not None and ref["bricks"] > CTX["max_bricks"]:
        assert st["n_grows"] > 0, st
    else:
        assert st["n_grows"] == 0 and st["n_replayed"] == 0, st
    return st


def run(g, scans):
    for p, e in scans:
        g.integrate(p, e)
    g.sync()
    return g


# ---- a. the grid --------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_grid(scan0, entry, variant):
    """Every band of the grid under every semantics, max_batch 2: a batch of two scans, then --
    through a sync() -- two batches of one, so that the last batch's pairs are one scan's.  The
    field, the rays, the bricks and the last batch's pairs are the oracle's."""
    kw, posed = VARIANTS[variant]
    adv = scans_of(entry, scan0, posed)
    scans = [adv[0], adv[3], adv[1], adv[2]]  # the scene's scan second
    ref = oracle_ref(("grid", entry, variant), entry, scans, **kw)
    g = hip(entry, max_batch=2, **kw)
    run(g, scans[:3])
    run(g, scans[3:])
    n = assert_bitwise(g, ref["field"])
    assert n > 10000
    st = assert_quiet(g, ref)
    assert st["n_batches"] == 3 and st["n_scans"] == 4
    assert st["n_rays_total"] == ref["rays"]
    assert st["n_bricks"] == ref["bricks"]
    assert st["n_pairs_last"] == ref["pairs_last"]
    g.close()


# ---- b. the single walk -------------------------------------------------------------------------

def front_end(vol):
    launches = vol.stats()["kernel_launches"]
    assert (launches["walk"] > 0) != (launches["count"] > 0)
    return "walk" if launches["walk"] else "count"


@pytest.mark.parametrize("variant", ["vdbfusion", "vdbfusion_f64", "voxblox_const"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_single_walk(scan0, entry, variant):
    """walk="single" over the grid: k_walk + k_spans run exactly where ctx_plan.h says the band is
    eligible (16 register slots up to band 6.92, 32 from 6.932; on the pair whose floats put the
    band at 7 while the plan sees less), and give the two-walk field and the oracle's."""
    kw, _ = VARIANTS[variant]
    scans = scans_of(entry, scan0, False)
    plan = B.plan_of(voxel_size=entry[0], sdf_trunc=entry[1], walk="single", max_batch=2, **CTX,
                     **kw)
    ref = oracle_ref(("single", entry, variant), entry, scans, last=2, **kw)  # batches of two
    g = hip(entry, max_batch=2, walk="single", **kw)
    g.set_profiling(True)
    run(g, scans)
    assert front_end(g) == ("walk" if plan.fused else "count")
    assert_bitwise(g, ref["field"])
    st = assert_quiet(g, ref)
    assert st["n_rays_total"] == ref["rays"] and st["n_pairs_last"] == ref["pairs_last"]
    if plan.fused:
        t = run(hip(entry, max_batch=2, **kw), scans)
        for x, y in zip(g.export_voxels(), t.export_voxels()):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y)
        t.close()
    g.close()


# ---- c. kernel variants away from six voxels ----------------------------------------------------

C_ENTRIES = [pytest.param((0.05, 0.05), id="band2"), pytest.param((0.07, 0.37), id="band10.57")]
C_VARIANTS = ["vdbfusion_f64", "voxblox_z2"]


@pytest.mark.parametrize("env", [
    {"TSDF_SMALL_NS": "8", "TSDF_COUNT_WIDE": "256"},   # k_integrate_small, 1024-lane k_count
    {"TSDF_SMALL_NS": "0", "TSDF_COUNT_WIDE": "0"},     # k_integrate, 256-lane k_count
    {"TSDF_COUNT_PAIRED": "1", "TSDF_COUNT_WIDE": "0"},  # two blocks per 512-lane workgroup
], ids=["small", "large", "paired"])
@pytest.mark.parametrize("variant", C_VARIANTS)
@pytest.mark.parametrize("entry", C_ENTRIES)
def test_kernel_variants(scan0, monkeypatch, entry, variant, env):
    """The run-time kernel choices (tests/test_gpu_parity.py::test_small_batch_kernel_bitwise's and
    ::test_paired_count_workgroups_bitwise's switches) at a band of 2 voxels (register path of
    k_count / k_place) and of 10.57 (their per-pair emit path)."""
    for k in ("TSDF_SMALL_NS", "TSDF_COUNT_WIDE", "TSDF_COUNT_PAIRED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw, posed = VARIANTS[variant]
    scans = scans_of(entry, scan0, posed)
    ref = oracle_ref(("variants", entry, variant), entry, scans, **kw)
    g = run(hip(entry, max_batch=2, **kw), scans)
    assert_bitwise(g, ref["field"])
    st = assert_quiet(g)
    assert st["n_rays_total"] == ref["rays"] and st["n_bricks"] == ref["bricks"]
    g.close()


@pytest.mark.parametrize("pipeline", [0, 1, 2])
@pytest.mark.parametrize("variant", C_VARIANTS)
def test_pipelines_at_band_10(scan0, variant, pipeline):
    """Six scans, two per batch, under the three batch pipelines at band 10.57."""
    entry = (0.07, 0.37)
    kw, posed = VARIANTS[variant]
    scans = scans_of(entry, scan0, posed, seeds=(0, 1))[1:]  # five adversarial scans + the scene's
    assert len(scans) == 6
    ref = oracle_ref(("pipe", entry, variant), entry, scans, last=2, **kw)
    g = run(hip(entry, max_batch=2, pipeline=pipeline, **kw), scans)
    assert_bitwise(g, ref["field"])
    st = assert_quiet(g)
    assert st["n_batches"] == 3 and st["n_rays_total"] == ref["rays"]
    assert st["n_pairs_last"] == ref["pairs_last"]
    g.close()


# ---- d. the 512-scan instantiation --------------------------------------------------------------

@pytest.mark.parametrize("variant", ["vdbfusion", "voxblox_z2"])
def test_130_scans_one_batch(variant):
    """130 scans of 188 adversarial rays each (every eighth ray of an adversarial scan: each family
    in each) as ONE device batch of a max_batch = 512 context (k_integrate<MAXS = 512>, windows of
    up to 128 scans) at band 10.57; Voxblox through integrate_batch_device_pose."""
    import torch
    entry = (0.07, 0.37)
    kw, posed = VARIANTS[variant]
    scans = [(np.ascontiguousarray(p[j::8]), o) for seed in range(6)
             for p, o in B.adversarial_rays(*entry, seed=seed) for j in range(8)][:130]
    assert len(scans) == 130 and all(p.shape[0] == 188 for p, _ in scans)
    if posed:
        scans = B.tilted(scans)
    ref = oracle_ref(("b512", entry, variant), entry, scans, last=130, **kw)
    g = hip(entry, max_batch=512, **kw)
    g.set_profiling(True)
    d = torch.from_numpy(np.concatenate([p for p, _ in scans])).to(g.tensor_device)
    torch.cuda.synchronize()
    offs = np.cumsum([0] + [p.shape[0] for p, _ in scans]).astype(np.uint64)
    ext = np.stack([e for _, e in scans])
    if posed:
        g.integrate_batch_device_pose(d.data_ptr(), offs, ext)
    else:
        g.integrate_batch_device(d.data_ptr(), offs, ext)
    g.sync()
    assert_bitwise(g, ref["field"])
    st = assert_quiet(g)
    assert st["n_batches"] == 1 and st["n_scans"] == 130 and st["kernel_launches"]["count"] == 1
    assert st["n_rays_total"] == ref["rays"] and st["n_pairs_last"] == ref["pairs_last"]
    g.close()
    del d


# ---- e. Voxblox at and below one voxel of truncation, dropoff on ---------------------------------

@pytest.mark.parametrize("variant", ["voxblox_const", "voxblox_z2", "voxblox_merged"])
@pytest.mark.parametrize("entry", [(0.05, 0.05), (0.05, 0.04), (0.05, 0.025)],
                         ids=["tau=vs", "tau=0.8vs", "tau=0.5vs"])
def test_voxblox_dropoff_at_and_below_one_voxel(scan0, entry, variant):
    """The dropoff's divisor tau - vs is zero at tau == vs (a quotient is +-inf, or NaN where
    tau + sdf == 0, and the w > 0 select turns both into a dropped sample or an infinite weight
    the gate sees) and negative below (the quotient then grows behind the surface: weights above
    the ray's).  The formula is upstream's; the oracle's field is finite, and the GPU's equals it."""
    kw, posed = VARIANTS[variant]
    assert F(entry[1]) - F(entry[0]) <= 0
    scans = scans_of(entry, scan0, posed)
    ref = oracle_ref(("dropoff", entry, variant), entry, scans, **kw)
    _, s, w = ref["field"]
    assert s.size > 10000 and np.isfinite(s).all() and np.isfinite(w).all()
    if entry[1] < entry[0] and variant == "voxblox_const":
        # a single ray of weight 1 leaves weights above 1: the quotient of the negative divisor
        top = 0.0
        for q in scans[0][0][:200:4]:
            one = B.oracle_volume(*entry, **kw)
            one.integrate(q[None], scans[0][1])
            top = max(top, float(one.export_voxels()[2].max(initial=0.0)))
            one.close()
        assert top > 1.0, top
    g = run(hip(entry, max_batch=2, **kw), scans)
    assert_bitwise(g, ref["field"])
    st = assert_quiet(g)
    assert st["n_rays_total"] == ref["rays"] and st["n_bricks"] == ref["bricks"]
    g.close()


# ---- f. carving with a short range --------------------------------------------------------------

@pytest.mark.parametrize("variant", ["vdbfusion_f64", "voxblox_z2"])
@pytest.mark.parametrize("entry", [(0.03, 0.1), (0.07, 0.37)], ids=["band6.67", "band10.57"])
def test_carving_short_range(scan0, entry, variant):
    """space_carving with max_range 3 m: a walk of up to 103 voxels at 3 cm (about 40 pair slots
    per ray) and 49 at 7 cm (19), between the six-voxel band and the 400-voxel carving cases.  The
    adversarial hits lie within 2.5 m; the scene's points beyond 3 m are dropped (VDBFusion) or
    become clearing rays (Voxblox)."""
    kw, posed = VARIANTS[variant]
    kw = dict(kw, space_carving=True, max_range=3.0)
    plan = B.plan_of(voxel_size=entry[0], sdf_trunc=entry[1], max_batch=2, **CTX, **kw)
    assert plan.maxp > 10
    scans = scans_of(entry, scan0, posed, reach=2.5)
    ref = oracle_ref(("carve", entry, variant), entry, scans, last=2, **kw)  # batches of two
    g = run(hip(entry, max_batch=2, **kw), scans)
    assert assert_bitwise(g, ref["field"]) > 20000
    st = assert_quiet(g)
    assert st["n_rays_total"] == ref["rays"] and st["n_bricks"] == ref["bricks"]
    assert st["n_pairs_last"] == ref["pairs_last"]
    g.close()


# ---- g. exact sums inside their headroom --------------------------------------------------------

@pytest.mark.parametrize("tau", [0.15, 2.0])
def test_capped_weights_sum_exactly_inside_the_headroom(tau):
    """n identical points of one scan, Voxblox with 1 / z^2 weights, z = 1e-3 (1 / z^2 = 1e6: the
    per-sample cap min(max_weight, 2^16) = 2^16 binds), max_weight 1e9, no dropoff.

    The cells (read from tsdf_integrate.hip, k_integrate and k_integrate_small alike): a voxel's
    weight cell is an unsigned 64-bit LDS word that takes atomicAdd(trunc(w 2^32)) per sample and
    is READ BACK AS SIGNED ((double)(long long)cB * 2^-32), its value cell likewise a signed sum of
    trunc((s w) 2^32); the oracle's A and B are int64.  Both sums are exact while they stay below
    2^63: n w_cap < 2^31 and n |s| w_cap < 2^31, |s| the largest sample of the ray (Voxblox's
    projective distance is not truncated before the sum: up to tau plus a voxel's half diagonal).
    With w_cap = 2^16 that is n < 2^15 = 32768 at tau = 0.15 (the weight sum binds) and
    n < 2^15 / |s|max, about 16000, at tau = 2 (the value sum binds).  n is 0.9 of the tighter bound;
    nothing beyond the bound is sent.

    Closed form: every voxel of the ray holds W = min(max_weight, n 2^16) and S = the ray's
    sample, summed in fixed point and divided, clamped to +-tau."""
    vs, cap, mw = 0.05, 65536.0, 1e9
    kw = dict(semantics="voxblox", use_const_weight=False, use_weight_dropoff=False, max_weight=mw)
    o = np.array([0.012, 0.013, 0.011])
    p = (o + [3.0, 0.4, 1e-3]).astype(F)
    pose = np.concatenate([o, [0.0, 0.0, 0.0, 1.0]])
    one = B.oracle_volume(vs, tau, **kw)
    ijk, s = one.ray_voxels(p, o)
    one.close()
    smax = float(np.abs(s).max())
    assert ijk.shape[0] > 5 and 0.5 * tau < smax < tau + vs
    bound = min(2.0 ** 31 / cap, 2.0 ** 31 / (smax * cap))
    n = int(0.9 * bound)
    assert n * cap < 2 ** 31 and n * smax * cap < 2 ** 31
    print("tau %g: |s|max %.4f, bound %d, n %d" % (tau, smax, int(bound), n))
    pts = np.repeat(p[None], n, 0)
    ora = B.oracle_volume(vs, tau, **kw)
    ora.integrate(pts, pose)
    oi, os_, ow = ora.export_voxels()
    # the oracle against the closed form
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
    assert np.array_equal(oi, ijk[order])
    want_w = F(min(mw, n * cap))
    assert np.all(ow == want_w), (np.unique(ow), want_w)
    b = F(n * int(F(cap) * F(4294967296.0)) / 2.0 ** 32)
    for k, sd in zip(order, os_):
        a = F(n * int(F(s[k]) * F(cap) * F(4294967296.0)) / 2.0 ** 32)
        ns = F(a) / F(b)
        assert sd == (min(ns, F(tau)) if ns > 0 else max(ns, -F(tau))), (s[k], sd)
        assert abs(float(sd) - max(-tau, min(tau, float(s[k])))) < 1e-6
    # the GPU against the oracle
    g = hip((vs, tau), max_points=1 << 15, max_bricks=1 << 14, **kw)
    g.integrate(pts, pose)
    g.sync()
    assert_bitwise(g, (oi, os_, ow))
    assert_quiet(g)
    g.close()
    ora.close()
