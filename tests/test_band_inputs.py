"""The per-ray bounds of the sizing plan (noetic-slam_amd/csrc/ctx_plan.h: pair slots maxp, sample
slots spr, the single walk's register slots nstep) held against real walks, on the CPU: the oracle
walks tests/bandref.py's adversarial rays at every band of its grid, under each semantics, and every
ray must stay inside what the header itself (tests/cpp/ctx_plan_print.cpp) sizes for it.  The plan
computes the band from the double parameters, the walks run on their floats: two grid entries lie
below an integer in double and at or above it in float.

The second half checks the inputs: the grid covers every class of the plan, every family of rays is
present, kept by the oracle and does what it is there for.  tests/test_band_sweep_gpu.py runs the
same grid and rays on the GPU."""
import numpy as np
import pytest

import bandref as B

F = np.float32
ENTRIES = [pytest.param(g, id="%g-%.11g" % g) for g in B.GRID]


def sem_kw(semantics):
    # constant weights and no range limit: the Voxblox variant the single walk takes
    return dict(semantics=semantics, **({"use_const_weight": True} if semantics == "voxblox" else {}))


@pytest.fixture(scope="module")
def plans():
    """ctx_plan.h's plan of every (grid entry, semantics) with the single walk asked for, so that
    `fused` says whether the band is eligible for it."""
    keys = [(g, s) for g in B.GRID for s in B.SEMANTICS]
    sets = [dict(voxel_size=g[0], sdf_trunc=g[1], walk="single", max_points=1 << 14, max_batch=2,
                 **sem_kw(s)) for g, s in keys]
    return dict(zip(keys, B.plans_of(sets)))


_facts = {}


def facts_of(entry, semantics):
    """ray_facts of the entry's three adversarial scans, concatenated (cached)."""
    key = (entry, semantics)
    if key not in _facts:
        o = B.oracle_volume(*entry, **sem_kw(semantics))
        parts = [B.ray_facts(o, (p, org)) for p, org in B.adversarial_rays(*entry)]
        o.close()
        _facts[key] = B.RayFacts(*[np.concatenate([getattr(f, k) for f in parts])
                                   for k in ("visited", "gated", "runs")],
                                 sum(f.kept for f in parts))
    return _facts[key]


# ---- the bounds ---------------------------------------------------------------------------------

@pytest.mark.parametrize("semantics", B.SEMANTICS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_bounds_hold_on_real_walks(plans, entry, semantics):
    """A ray's brick runs stay within maxp and its gated voxels within spr; where the band is
    eligible for the single walk, the voxels its DDA visits (gated or not: k_walk spends one
    register slot per step) stay within nstep."""
    P, f = plans[(entry, semantics)], facts_of(entry, semantics)
    print("band %-10.7g %-13s pairs %2d / maxp %2d   samples %2d / spr %2d   steps %2d / nstep %s"
          % (B.band_float(*entry), semantics, f.runs.max(), P.maxp, f.gated.max(), P.spr,
             f.visited.max(), P.nstep if P.fused else "-"))
    assert f.kept > 4000
    assert f.runs.max() <= P.maxp
    assert f.gated.max() <= P.spr
    if P.fused:
        assert P.maxp <= 4
        assert f.gated.max() <= P.nstep
        assert f.visited.max() <= P.nstep


@pytest.mark.parametrize("entry", sorted(B.STRADDLE), ids=lambda g: "%g-%.11g" % g)
def test_straddling_pairs_straddle(plans, entry):
    """The double band lies below the integer (the plan sizes for it), the floats' band at or above
    it (the kernels walk it), in float and in double arithmetic on the floats alike."""
    vs, tau = entry
    k = B.STRADDLE[entry]
    assert entry in B.GRID
    assert B.band_double(vs, tau) < k
    assert B.band_float(vs, tau) >= k
    assert F(2.0) * F(tau) / F(vs) >= F(k)
    assert F(2.0) * F(tau) * (F(1.0) / F(vs)) >= F(k)
    # the plan is the lower integer's: that of the band a hair below, not that of the integer
    lo, at = B.plans_of([dict(voxel_size=vs, sdf_trunc=tau, walk="single", semantics="vdbfusion"),
                         dict(voxel_size=vs, sdf_trunc=k * vs / 2 * (1 + 1e-9), walk="single",
                              semantics="vdbfusion")])
    assert plans[(entry, "vdbfusion")][:4] == lo[:4]
    assert (lo.maxp, lo.spr) != (at.maxp, at.spr) or lo.fused != at.fused


# ---- the inputs ---------------------------------------------------------------------------------

def test_grid_covers_every_class(plans):
    P = [plans[(g, "vdbfusion")] for g in B.GRID]
    assert {p.maxp for p in P} >= {4, 7, 10}
    assert {p.nstep for p in P if p.fused} == {16, 32}
    assert {p.fused for p in P} == {True, False}
    assert sum(g in B.GRID for g in B.STRADDLE) == 2
    assert len({F(vs) for vs, _ in B.GRID} - {F(0.05)}) >= 3
    # eligibility is the band's alone: the same under the three semantics
    for g in B.GRID:
        assert len({plans[(g, s)][:4] for s in B.SEMANTICS}) == 1, g
    # the slot count changes between the two bands that bracket sqrt(3) band = 11
    by = dict(zip(B.GRID, P))
    assert by[(0.05, 0.173)].nstep == 16 and by[(0.05, 0.1733)].nstep == 32
    # 1/z^2 weights and a finite max_range (clearing rays) keep the two-walk path
    off = B.plans_of([dict(voxel_size=0.05, sdf_trunc=0.1, walk="single", semantics="voxblox"),
                      dict(voxel_size=0.05, sdf_trunc=0.1, walk="single", semantics="voxblox",
                           use_const_weight=True, max_range=30.0),
                      dict(voxel_size=0.05, sdf_trunc=0.1, semantics="vdbfusion")])
    assert not any(p.fused for p in off)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_family_is_present_and_kept(entry):
    """Every family at its size in every scan; the oracle keeps at least 90 % of each under each
    semantics -- all of them but family 6's zero-depth points, which every semantics drops."""
    scans = B.adversarial_scans(*entry)
    assert len(scans) == 3
    for p, org, fam, zero in scans:
        assert p.dtype == np.float32 and p.shape == (sum(B.FAMILY_SIZE.values()), 3)
        assert np.isfinite(p).all()
        for k, n in B.FAMILY_SIZE.items():
            assert np.count_nonzero(fam == k) == n, B.FAMILIES[k]
        assert np.count_nonzero(zero) == B.N_ZERO_DEPTH and np.all(fam[zero] == 6)
    fam = np.concatenate([s[2] for s in scans])
    zero = np.concatenate([s[3] for s in scans])
    for semantics in B.SEMANTICS:
        f = facts_of(entry, semantics)
        assert np.all(f.visited[zero] == -1)
        assert f.kept == fam.size - 3 * B.N_ZERO_DEPTH
        for k in B.FAMILIES:
            m = (fam == k) & ~zero
            kept = np.count_nonzero(f.visited[m] >= 0)
            assert kept >= 0.9 * m.sum(), (semantics, B.FAMILIES[k], kept)
            # and they reach the fuse: a family of rays without gated voxels would test nothing
            # (below one voxel of truncation a band can miss every centre -- a short ray's mostly
            # does --, and a hit on a voxel centre has that voxel alone in its band, the skipped
            # one: there only some of a family's rays can be asked for)
            need = 0.9 * m.sum() if B.band_double(*entry) >= 2 else 30
            assert np.count_nonzero(f.gated[m] > 0) >= need, (semantics, B.FAMILIES[k])


@pytest.mark.parametrize("entry", ENTRIES)
def test_families_do_what_they_are_for(entry):
    vs, tau = entry
    scans = B.adversarial_scans(vs, tau)
    fam = np.concatenate([s[2] for s in scans])
    v32, t32 = F(vs), F(tau)
    for semantics in B.SEMANTICS:
        f = facts_of(entry, semantics)
        # 1: some near-diagonal ray reaches 4 brick runs at every band of two voxels and more
        if B.band_double(vs, tau) >= 2:
            assert f.runs[fam == 1].max() >= 4, semantics
        # 7: identical points walk identically
        for k in ("visited", "gated", "runs"):
            a = getattr(f, k)[fam == 7].reshape(3, -1)
            assert np.all(a == a[:, :1])
    ties = 0
    for p, org, fm, zero in scans:
        o32 = org.astype(F)
        d = p - o32[None]
        # 2: on the grid (an exact multiple of float32(vs)) wherever the origin is, axis-parallel
        #    or diagonal, with equal initial t_next values among them
        g = fm == 2
        nz = np.count_nonzero(d[g] != 0, axis=1)
        assert np.count_nonzero(nz == 1) == 120 and np.count_nonzero(nz == 2) == 60
        q = np.round(p[g].astype(np.float64) / float(v32))
        on = np.array([k is not None for k in B.ORIGIN_GRID[[np.array_equal(org, x) for x in
                                                             B.origins_of(vs)].index(True)]])
        assert np.all((q.astype(F) * v32)[:, on] == p[g][:, on])
        ties += np.count_nonzero(B.finite_ties(B.initial_t_next(p[g], org, vs, tau)))
        # 3: one zero, two zeros, one tiny component
        z = d[fm == 3]
        nz = np.count_nonzero(z == 0, axis=1)
        assert np.count_nonzero(nz == 1) >= 66 and np.count_nonzero(nz == 2) >= 66
        u = np.abs(z) / np.linalg.norm(z.astype(np.float64), axis=1)[:, None]
        tiny = np.count_nonzero(((u > 0) & (u < 1e-6)).any(axis=1))
        assert tiny >= 60, tiny
        # 4: hits on voxel centres as the kernels form them; centres at tau behind the hit
        c = p[fm == 4][:100]
        assert np.all((np.floor(c / v32) + F(0.5)) * v32 == c)
        # 5: hits in the negative octants, some within tau of a plane of index 0
        n5 = p[fm == 5]
        assert np.count_nonzero((n5 < 0).all(axis=1)) >= 50
        assert np.count_nonzero((np.abs(n5) < t32).any(axis=1)) >= 50
        # 6: depths below tau, at tau and of a tenth of a voxel
        depth = np.linalg.norm(d[fm == 6].astype(np.float64), axis=1)
        assert np.count_nonzero((depth > 0) & (depth < 0.9 * tau)) >= 60
        assert np.count_nonzero(np.abs(depth / float(t32) - 1) < 1e-6) >= 30
        assert np.count_nonzero((depth > 0) & (depth < 0.2 * vs)) >= 30 or tau < 0.2 * vs
    print("band %-10.7g family 2 rays with two equal finite t_next: %d" % (B.band_float(vs, tau),
                                                                          ties))
    assert ties >= 20


@pytest.mark.parametrize("semantics", ["vdbfusion", "voxblox"])
@pytest.mark.parametrize("entry", [B.GRID[1], B.GRID[9], B.GRID[13]], ids=lambda g: "%g-%.11g" % g)
def test_ray_facts_agree_with_ray_voxels(entry, semantics):
    """ray_facts' counts against OracleTSDFVolume.ray_voxels one ray at a time (the fp32 walks,
    which both take): gated is the list's length, runs the changes of ijk >> 3 along it, and a run
    is a distinct brick (a line meets a brick once)."""
    o = B.oracle_volume(*entry, **sem_kw(semantics))
    f = facts_of(entry, semantics)
    pts = np.concatenate([p for p, _ in B.adversarial_rays(*entry)])
    org = np.repeat(np.stack([q for _, q in B.adversarial_rays(*entry)]), pts.shape[0] // 3, 0)
    for i in range(0, pts.shape[0], 7):
        got = o.ray_voxels(pts[i], org[i], cap=4096)
        if got is None:
            assert f.visited[i] == -1
            continue
        b = got[0] >> 3
        runs = 0 if b.shape[0] == 0 else 1 + np.count_nonzero(np.any(b[1:] != b[:-1], axis=1))
        assert (f.gated[i], f.runs[i]) == (b.shape[0], runs), i
        assert runs == np.unique(b, axis=0).shape[0], i
