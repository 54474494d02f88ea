"""Reference for the batch counters of tsdf_get_stats and the metrics log (test helper; DESIGN.md
§18).  Nothing here calls libtsdf_hip.so.

Definitions, read from k_count / k_walk, k_compact_scan, k_integrate / k_integrate_small and
k_finish (not measured on them):

  per scan
    ray      a point that passes the range filter (min_range / max_range, the far-ray rule, the
             sector filter) and walks; Voxblox "merged": a bundle.  A ray without one gated voxel
             is still a ray.
    samples  a ray's gated voxels (the voxels its walk hands to the fuse).
    pairs    the distinct bricks (ijk >> 3) among a ray's samples (k_count closes a pair when the
             next gated voxel's brick differs; a line meets a brick in one run).
    U_vox    the distinct voxels among the scan's samples.  Voxblox: a voxel whose fuse the
             nw < 1e-6 rule skips still counts, k_integrate counts the cell, not the update.
  per batch (consecutive scans launched together)
    rays, pairs, voxel_updates   sums over the batch's scans (voxel_updates = sum of U_vox)
    dirty    the distinct voxels over all the batch's scans
    active   the distinct bricks over all the batch's scans
    new      the active bricks the map did not hold before the batch
    bricks   the bricks the map holds after the batch

Two routes to these numbers:

  Route A (oracle): every scan goes into a FRESH OracleTSDFVolume; the voxels it exports (W > 0)
  are the scan's sampled set.  Why: the map was empty, so a voxel's W after the scan is the sum of
  its samples' weights.  VDBFusion samples weigh 1.  A Voxblox sample is gated at w >= 2^-16
  (VB_MIN_WEIGHT) and 2^-16 > 1e-6, so the first fuse of a sampled voxel is never skipped by the
  nw < 1e-6 rule and leaves W >= 2^-16 > 0; 1/z^2 weights and bundle weights only scale w by a
  positive factor that the gate sees too.  A clearing or carving sample weighs like any other.  So
  W > 0 exactly on the sampled voxels.  Rays are the oracle's n_rays_total.  The route holds for
  every semantics, carving, range limits, clearing rays and sector filters.

  Route B (numpy): tests/walkref.py's restated walks with each sample's ray index; gives the same
  numbers plus a ray's pairs, within walkref's scope (origin-only, no carving, no range limits,
  far from the domain's edge).

  Pairs outside route B's scope (carving, clearing rays, a range-filtered cloud): the oracle one
  ray at a time, each ray a one-point scan into a fresh volume, pairs = distinct ijk >> 3 of its
  export.  Slow: a few hundred rays at most.
"""
import numpy as np

import oracle
import walkref

VS, TAU = 0.05, 0.15
RPB = 1024          # TSDF_RPB: rays per k_count block; counters are sharded by block index & 7
METRIC_RING = 256   # tsdf_device.h
BIAS = 1 << 20
M21 = (1 << 21) - 1

ORACLE_DROPS = ("max_batch", "pipeline", "walk", "max_points", "max_bricks", "max_bricks_hard")


def vkey(ijk):
    """One int64 per voxel (21 bits per axis, biased by 2^20)."""
    v = np.asarray(ijk, np.int64).reshape(-1, 3) + BIAS
    assert v.size == 0 or (v.min() >= 0 and v.max() <= M21)
    return v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)


def brick_of(vk):
    """Brick keys of voxel keys (the bias is a multiple of 8, so each field shifts on its own)."""
    vk = np.asarray(vk, np.int64)
    return ((vk & M21) >> 3) | ((((vk >> 21) & M21) >> 3) << 21) | ((vk >> 45) << 42)


def bkey(bijk):
    """Brick keys of brick coordinates (voxel >> 3), comparable with brick_of()."""
    b = np.asarray(bijk, np.int64).reshape(-1, 3) + (BIAS >> 3)
    return b[:, 0] | (b[:, 1] << 21) | (b[:, 2] << 42)


def oracle_volume(vs=VS, tau=TAU, **kw):
    for k in ORACLE_DROPS:
        kw.pop(k, None)
    return oracle.OracleTSDFVolume(vs, tau, **kw)


class ScanRef:
    """One scan's counters: points, rays, vox (sorted distinct voxel keys), pairs (None where the
    route gives none), oracle_vox (the oracle's own n_voxels_last; route A only)."""

    def __init__(self, points, rays, vox, pairs=None, oracle_vox=None):
        self.points, self.rays, self.vox = int(points), int(rays), vox
        self.pairs = None if pairs is None else int(pairs)
        self.oracle_vox = oracle_vox

    @property
    def u_vox(self):
        return int(self.vox.shape[0])

    @property
    def bricks(self):
        return np.unique(brick_of(self.vox))


def scan_ref_oracle(pts, ext, vs=VS, tau=TAU, **kw):
    """Route A for one scan (ext: origin or pose, as HipTSDFVolume.integrate takes it)."""
    o = oracle_volume(vs, tau, **kw)
    o.integrate(pts, ext)
    st = o.stats()
    ijk, _, w = o.export_voxels()
    assert np.all(w > 0)
    o.close()
    return ScanRef(st["n_points_in"], st["n_rays_total"], np.unique(vkey(ijk)),
                   oracle_vox=st["n_voxels_last"])


def scan_ref_numpy(pts, org, semantics, vs=VS, tau=TAU):
    """Route B for one scan (walkref's scope), pairs included."""
    p = np.ascontiguousarray(pts, np.float32)
    with np.errstate(all="ignore"):
        parts = walkref._SAMPLES[semantics](p, org, np.float32(vs), np.float32(tau), rays=True)
    vk = vkey(np.concatenate([x[0] for x in parts]))
    ray = np.concatenate([x[3] for x in parts]).astype(np.int64)
    o32 = np.asarray(org, np.float64).astype(np.float32)
    rays = int(np.count_nonzero(np.any(p != o32, axis=1)))  # depth > 0 (no range limits in scope)
    rb = np.unique(np.stack([ray, brick_of(vk)], 1), axis=0)
    return ScanRef(p.shape[0], rays, np.unique(vk), pairs=rb.shape[0])


def pairs_per_ray_numpy(pts, org, semantics, vs=VS, tau=TAU):
    """Route B's pairs of every ray (n,)."""
    p = np.ascontiguousarray(pts, np.float32)
    with np.errstate(all="ignore"):
        parts = walkref._SAMPLES[semantics](p, org, np.float32(vs), np.float32(tau), rays=True)
    vk = vkey(np.concatenate([x[0] for x in parts]))
    ray = np.concatenate([x[3] for x in parts]).astype(np.int64)
    rb = np.unique(np.stack([ray, brick_of(vk)], 1), axis=0)
    return np.bincount(rb[:, 0], minlength=p.shape[0])


def pairs_per_ray_oracle(pts, ext, vs=VS, tau=TAU, **kw):
    """The oracle one ray at a time: pairs of every ray (n,), 0 for a ray the filter drops."""
    p = np.ascontiguousarray(pts, np.float32)
    assert p.shape[0] <= 400, "the per-ray oracle route is for a few hundred rays"
    out = np.zeros(p.shape[0], np.int64)
    for i in range(p.shape[0]):
        o = oracle_volume(vs, tau, **kw)
        o.integrate(p[i:i + 1], ext)
        ijk, _, _ = o.export_voxels()
        out[i] = np.unique(bkey(ijk.astype(np.int64) >> 3)).shape[0]
        o.close()
    return out


def batch_refs(refs, partition, held=None):
    """The metrics records of `refs` launched in batches of partition[b] scans, into a map holding
    the brick keys `held`.  Returns (records, held after)."""
    held = np.zeros(0, np.int64) if held is None else np.unique(np.asarray(held, np.int64))
    assert sum(partition) == len(refs)
    out, i = [], 0
    for n in partition:
        grp = refs[i:i + n]
        i += n
        dirty = np.unique(np.concatenate([r.vox for r in grp]))
        act = np.unique(brick_of(dirty))
        new = np.setdiff1d(act, held, assume_unique=True)
        held = np.union1d(held, act)
        rec = dict(scans=n, points=sum(r.points for r in grp), rays=sum(r.rays for r in grp),
                   pairs=None if any(r.pairs is None for r in grp) else sum(r.pairs for r in grp),
                   voxel_updates=sum(r.u_vox for r in grp), dirty_voxels=int(dirty.shape[0]),
                   active_bricks=int(act.shape[0]), new_bricks=int(new.shape[0]),
                   bricks=int(held.shape[0]))
        rec["algorithmic_bytes"] = 12 * rec["rays"] + 16 * rec["voxel_updates"]
        out.append(rec)
    return out, held


def totals(records):
    """tsdf_get_stats of a context that ran exactly these batches since create / reset_stats."""
    last = records[-1]
    st = dict(n_scans=sum(r["scans"] for r in records), n_batches=len(records),
              n_points_in=sum(r["points"] for r in records),
              n_rays_total=sum(r["rays"] for r in records),
              n_voxels_total=sum(r["voxel_updates"] for r in records),
              n_dirty_total=sum(r["dirty_voxels"] for r in records),
              n_voxels_last=last["voxel_updates"], n_active_last=last["active_bricks"],
              n_bricks=last["bricks"])
    if last["pairs"] is not None:
        st["n_pairs_last"] = last["pairs"]
    return st


def assert_nonvacuous(refs, partition, records, shards=True):
    """Every input of the GPU tests must make its counters tell each other apart: asserted on the
    reference (tests/test_stats_ref.py) and again before the GPU comparison."""
    i = 0
    for b, (n, rec) in enumerate(zip(partition, records)):
        grp = refs[i:i + n]
        i += n
        if n > 1:  # dirty is neither the largest scan nor the sum of the scans
            assert max(r.u_vox for r in grp) < rec["dirty_voxels"] < rec["voxel_updates"], (b, rec)
            common = grp[0].bricks
            for r in grp[1:]:
                common = np.intersect1d(common, r.bricks, assume_unique=True)
            assert common.shape[0] >= 1, b  # a brick sampled by every scan of the batch
        if rec["pairs"] is not None:
            assert rec["pairs"] > rec["rays"], (b, rec)
        if b > 0:
            assert 0 < rec["new_bricks"] < rec["active_bricks"], (b, rec)
        if shards:  # all eight counter shards (block index & 7) can receive something
            assert rec["rays"] >= 8 * RPB and rec["active_bricks"] >= 64, (b, rec)


# ---- the inputs of tests/test_stats_gpu.py ------------------------------------------------------
# name -> (scan ids, decimation).  Decimated scans of the session's OusterSim, 2 048 - 8 192 points.
INPUTS = {
    "seq11": (tuple(range(0, 33, 3)), 16),   # 11 scans: batches of 1, 3 (3+3+3+2) and 9 (9+2)
    "seq70": (tuple(range(70)), 64),          # 64-scan windows: 64 + 6
    "seq6": ((0, 4, 8, 12, 16, 20), 16),      # growth / reset / changed-map cases, sector shards
    "seq3": ((0, 5, 10), 32),                 # Voxblox variants
    # space carving to 20 m keeps a third of this scene's rays: 16 scans for 8 * RPB valid ones
    "carve16": (tuple(range(0, 48, 3)), 64),
}
SEMANTICS = ("vdbfusion_f64", "vdbfusion", "voxblox")

_scans, _refs = {}, {}


def scans_of(sim, name):
    if name not in _scans:
        ids, dec = INPUTS[name]
        _scans[name] = [(np.ascontiguousarray(p[::dec]), o) for p, o in (sim.scan(k) for k in ids)]
    return _scans[name]


def sem_kw(semantics):
    """Context keywords of a semantics within route B's scope (Voxblox: constant point weight)."""
    return dict(semantics=semantics, **({"use_const_weight": True} if semantics == "voxblox" else {}))


def refs_oracle(sim, name, **kw):
    """Route A's ScanRefs of an input, computed once per (input, context keywords)."""
    key = ("A", name, tuple(sorted((k, v) for k, v in kw.items() if k not in ORACLE_DROPS)))
    if key not in _refs:
        _refs[key] = [scan_ref_oracle(p, o, **kw) for p, o in scans_of(sim, name)]
    return _refs[key]


def refs_numpy(sim, name, semantics):
    """Route B's ScanRefs of an input (pairs included), computed once."""
    key = ("B", name, semantics)
    if key not in _refs:
        _refs[key] = [scan_ref_numpy(p, o, semantics) for p, o in scans_of(sim, name)]
    return _refs[key]


def few_rays(scans, step):
    """About a hundred rays of each scan: inputs of the one-ray-at-a-time pairs route."""
    return [(np.ascontiguousarray(p[3::step]), o) for p, o in scans]


def refs_few_rays(sim, name, step, **kw):
    """(scans, ScanRefs) of few_rays(first three scans of an input): route A, with pairs from the
    oracle one ray at a time.  Computed once per (input, step, context keywords)."""
    key = ("few", name, step, tuple(sorted((k, v) for k, v in kw.items() if k not in ORACLE_DROPS)))
    if key not in _refs:
        scans = few_rays(scans_of(sim, name)[:3], step)
        assert sum(p.shape[0] for p, _ in scans) <= 300
        out = []
        for p, e in scans:
            r = scan_ref_oracle(p, e, **kw)
            r.pairs = int(pairs_per_ray_oracle(p, e, **kw).sum())
            out.append(r)
        _refs[key] = (scans, out)
    return _refs[key]


CLEAR_KW = dict(semantics="voxblox", use_const_weight=True, allow_clear=True, max_range=12.0)
CLEAR_FEW = ("seq3", 41)
CARVE_FEW = ("carve16", 21)


def carve_kw(semantics):
    return dict(semantics=semantics, space_carving=True, max_range=20.0)


def assert_few_rays_nonvacuous(scans, refs, kw):
    """The few-ray inputs cannot fill eight shards (the per-ray route is for a few hundred rays);
    what they must show: the long-ray paths are taken, and pairs differ from rays."""
    rays, pairs = sum(r.rays for r in refs), sum(r.pairs for r in refs)
    if kw.get("space_carving"):  # long rays: many bricks each; some rays beyond max_range dropped
        assert 30 <= rays < sum(r.points for r in refs) and pairs > 8 * rays
    else:  # clearing rays and hits, no ray dropped
        far = sum(int(np.count_nonzero(np.linalg.norm(p - o.astype(np.float32), axis=1)
                                       > kw["max_range"])) for p, o in scans)
        assert 10 <= far <= rays - 10 and pairs > rays == sum(r.points for r in refs)
    recs, _ = batch_refs(refs, [len(refs)])
    assert_nonvacuous(refs, [len(refs)], recs, shards=False)


def empty_ref():
    """A scan without a point."""
    return ScanRef(0, 0, np.zeros(0, np.int64), pairs=0, oracle_vox=0)


def partition_of(n, max_batch):
    return [max_batch] * (n // max_batch) + ([n % max_batch] if n % max_batch else [])


def dense_brick_scan(brick=(100, 3, 2), vs=VS):
    """512 points at the voxel centres of one brick, seen from 5 m away along -x."""
    b = np.asarray(brick, np.int64) * 8
    g = np.arange(8)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    ijk = np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + b
    pts = ((ijk + 0.5) * vs).astype(np.float32)
    org = np.array([(b[0] + 4) * vs - 5.0, (b[1] + 4.3) * vs, (b[2] + 3.7) * vs])
    return pts, org, vkey(ijk)
