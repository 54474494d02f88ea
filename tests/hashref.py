"""The library's hash restated in numpy, and builders of inputs aimed at its tables (test helper;
DESIGN.md §20).  Nothing here calls libtsdf_hip.so.

Every hot structure is an open-addressing table keyed by mix64 (tsdf_ray.h):

  global brick table   home = mix64(brick key) & mask, mask = next_pow2(2 max_bricks) - 1
                       (table_insert / table_find, k_rehash)
  LDS brick hash       home = (mix64(brick key) >> 40) & (HCAP - 1)
                       (lds_insert: LDS_PROBES probes, then a fallback pair; lds_insert_full)
  Merged pre-pass      bucket = ((mix64(bundle key) >> 32) * P) >> 32 among P = mg_buckets(n),
                       LDS table home = mix64(bundle key) & (MG_TAB - 1)      (tsdf_merged.hip)

The hash is a fixed function, so the builders below search a box of candidate voxels or bricks for
keys with chosen buckets and homes, and return the cloud or brick set together with the facts a
test asserts about it.  The constants are restated here; tests/test_hashref.py reads the same names
out of the sources and asserts equality, so a retuned constant re-aims these tests."""
import functools

import numpy as np

F = np.float32
U = np.uint64

# tsdf_merged.hip
MG_BSHIFT = 10
MG_PMAX = 4096
MG_TAB = 2048
MG_GM = 2048
MG_GTHREADS = 512
MG_EPT = 3
MG_VOX_LIM = 1 << 20
# tsdf_device.h
RPB = 1024
HCAP = 2048
LDS_PROBES = 64
# brick_key.h
BRICK_KEY_BIAS = 1 << 20

MG_REG = MG_EPT * MG_GTHREADS  # a bucket's entries kept in registers; later ones are re-read


def mix64(k):
    """tsdf_ray.h mix64 on uint64 arrays (the products wrap, as the device's do)."""
    k = np.array(k, dtype=U, ndmin=1)
    k ^= k >> U(33)
    k *= U(0xff51afd7ed558ccd)
    k ^= k >> U(33)
    k *= U(0xc4ceb9fe1a85ec53)
    k ^= k >> U(33)
    return k


def brick_key(b):
    """brick_key.h brick_key_pack: biased coordinates in three 21-bit fields, x lowest."""
    b = np.asarray(b, np.int64).reshape(-1, 3)
    assert b.size == 0 or (b.min() >= -BRICK_KEY_BIAS and b.max() < BRICK_KEY_BIAS)
    v = (b + BRICK_KEY_BIAS).astype(U)
    return v[:, 0] | (v[:, 1] << U(21)) | (v[:, 2] << U(42))


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def table_mask(max_bricks):
    return next_pow2(2 * int(max_bricks)) - 1


def table_home(key, mask):
    return (mix64(key) & U(mask)).astype(np.int64)


def lds_home(key):
    return ((mix64(key) >> U(40)) & U(HCAP - 1)).astype(np.int64)


def mg_buckets(n):
    return min(max((int(n) + (1 << MG_BSHIFT) - 1) >> MG_BSHIFT, 1), MG_PMAX)


def mg_bucket(key, P):
    return (((mix64(key) >> U(32)) * U(P)) >> U(32)).astype(np.int64)


def mg_home(key):
    return (mix64(key) & U(MG_TAB - 1)).astype(np.int64)


def voxel_key(ijk, clearing=False):
    """The bundle key of voxel indices: clearing bit 63 | 21 biased bits per axis, x lowest."""
    v = (np.asarray(ijk, np.int64).reshape(-1, 3) + MG_VOX_LIM).astype(U)
    c = np.broadcast_to(np.asarray(clearing, bool), v.shape[:1]).astype(U)
    return (c << U(63)) | (v[:, 2] << U(42)) | (v[:, 1] << U(21)) | v[:, 0]


def voxel_of(points, vs):
    """The pre-pass's fp32 index rule: floor(fp32(p) * (fp32(1) / fp32(vs)) + fp32(1e-6))."""
    p = np.ascontiguousarray(points, F)
    inv = F(1) / F(vs)
    return np.floor(p * inv + F(1e-6)).astype(np.int64)


def depth_of(points, origin):
    """mg_point's fp32 depth: sqrt(dx dx + (dy dy + dz dz)) of p - fp32(origin)."""
    d = np.ascontiguousarray(points, F) - np.asarray(origin, np.float64)[:3].astype(F)
    return np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))


def merged_keys(points, origin, vs, max_range=np.inf, min_range=0.0, allow_clear=True):
    """(valid, key) of every point as mg_point forms them; an invalid point has no key (0)."""
    ijk = voxel_of(points, vs)
    depth = depth_of(points, origin)
    clearing = depth > F(max_range)
    ok = (depth > 0) & ~(depth < F(min_range)) & (~clearing | bool(allow_clear))
    ok &= np.all((ijk > -MG_VOX_LIM) & (ijk < MG_VOX_LIM), axis=1)
    key = np.where(ok, voxel_key(np.where(ok[:, None], ijk, 0), clearing), U(0))
    return ok, key


def probe_runs(homes, slots, limit=None):
    """Linear probing of `homes` (in this order) into an empty table of `slots`: (slot of every
    key or -1, longest probe count, whether a probe stepped from the last slot to slot 0).  A key
    probes at most `limit` slots (default: all); one that finds none is dropped.  Each slot keeps
    a pointer to the next free one, so a full cluster is skipped in one step."""
    limit = slots if limit is None else limit
    nxt = list(range(slots + 1))  # nxt[s]: the first free slot at or after s (slots: none, wrap)
    free = slots

    def first_free(s):
        r = s
        while nxt[r] != r:
            r = nxt[r]
        while nxt[s] != r:
            nxt[s], s = r, nxt[s]
        return r

    out, longest, wraps = [], 0, False
    for h in homes:
        h = int(h)
        if not free:
            out.append(-1)
            longest = max(longest, limit)
            wraps |= (h + limit - 1) >= slots
            continue
        s = first_free(h)
        wrapped = s == slots
        if wrapped:
            s = first_free(0)
        n = (s - h) % slots + 1
        if n > limit:
            out.append(-1)
            longest = max(longest, limit)
            wraps |= (h + limit - 1) >= slots
            continue
        out.append(s)
        nxt[s] = s + 1
        free -= 1
        longest = max(longest, n)
        wraps |= wrapped
    return np.array(out, np.int64), longest, wraps


# ---- candidates ----------------------------------------------------------------------------------

VS = 0.05
X_LO, X_HI = 3.0, 12.0  # the clouds lie this far in front of the sensor (along +x)


@functools.lru_cache(maxsize=None)
def _voxel_candidates(vs):
    """Voxels of a box 3 to 12 m in front of the sensor, +-6 m wide, +-1.5 m high (2.6 M)."""
    x = np.arange(int(round(X_LO / vs)), int(round(X_HI / vs)))
    y = np.arange(-int(round(6.0 / vs)), int(round(6.0 / vs)))
    z = np.arange(-int(round(1.5 / vs)), int(round(1.5 / vs)))
    g = np.stack(np.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _brick_candidates(r=80):
    """Bricks within +-r of the origin with their hashes (4.2 M for r = 80)."""
    a = np.arange(-r, r + 1)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    h = mix64(brick_key(g))
    g.setflags(write=False)
    h.setflags(write=False)
    return g, h


def bucket_facts(points, origin, bucket, vs=VS, **range_kw):
    """What a scan puts into one bucket of the pre-pass, by the restatement: entries (valid points),
    distinct keys, members (entries of keys met more than once), bundles (such keys), and the
    probing of its distinct keys (in order of first appearance) into the MG_TAB-slot table."""
    ok, key = merged_keys(points, origin, vs, **range_kw)
    P = mg_buckets(len(points))
    mine = ok & (mg_bucket(key, P) == bucket)
    k = key[mine]
    uniq, first, cnt = np.unique(k, return_index=True, return_counts=True)
    order = np.argsort(first)
    slots, longest, wraps = probe_runs(mg_home(uniq[order]), MG_TAB)
    return dict(P=P, valid=int(ok.sum()), keys_total=int(np.unique(key[ok]).shape[0]),
                entries=int(k.shape[0]), keys=int(uniq.shape[0]),
                members=int(cnt[cnt > 1].sum()), bundles=int((cnt > 1).sum()),
                sizes=np.sort(cnt[cnt > 1]), placed=int((slots >= 0).sum()),
                longest_probe=longest, wraps=bool(wraps),
                clearing_keys=int((uniq >> U(63)).sum()), straddled=_straddled(key[ok]))


def _straddled(keys):
    """Voxels that form both a key and a clearing key."""
    bit = U(1) << U(63)
    return int(np.intersect1d(np.unique(keys[(keys & bit) == 0]),
                              np.unique(keys[(keys & bit) != 0] ^ bit)).shape[0])


def bucket_cloud(n, spec, seed=0, bucket=0, vs=VS, origin=(0.0, 0.0, 0.0), max_range=np.inf,
                 far_frac=0.0, home=None, allow_clear=True, straddle=0):
    """One scan of n points whose bucket `bucket` (of mg_buckets(n)) receives the bundles of
    `spec`, a list of (k, m): k keys of m members each; the other points are singletons of the
    other buckets.  Points sit at voxel centres plus a jitter below 0.4 voxel, shuffled into cloud
    order.  far_frac of the target keys lie beyond max_range (clearing bundles: the key carries bit
    63); `home` = (first, count) takes the target keys' LDS table homes from that cyclic range.
    `straddle` voxels of the other buckets are cut by the max_range sphere and hold two points on
    either side of it: the same voxel then forms two keys, a bundle and a clearing bundle.
    Returns (points float32 (n, 3), facts); the facts are recomputed from the float32 points."""
    rng = np.random.default_rng(seed)
    P = mg_buckets(n)
    cand = _voxel_candidates(vs)
    o = np.asarray(origin, np.float64)
    centre = (cand + 0.5) * vs
    depth = np.linalg.norm(centre - o, axis=1)
    far = depth > max_range
    usable = np.abs(depth - max_range) > 3 * vs  # the jitter moves no point across max_range
    key = voxel_key(cand, far)
    bk = mg_bucket(key, P)
    in_t = (bk == bucket) & usable
    if home is not None:
        in_t &= ((mg_home(key) - home[0]) % MG_TAB) < home[1]
    n_keys = sum(k for k, _ in spec)
    n_far = int(round(far_frac * n_keys))
    near_i, far_i = np.flatnonzero(in_t & ~far), np.flatnonzero(in_t & far)
    assert near_i.size >= n_keys - n_far and far_i.size >= n_far, (near_i.size, far_i.size)
    pick = np.concatenate([rng.choice(near_i, n_keys - n_far, replace=False),
                           rng.choice(far_i, n_far, replace=False)])
    rng.shuffle(pick)
    sizes = np.concatenate([np.full(k, m) for k, m in spec]).astype(np.int64)
    rng.shuffle(sizes)
    target = np.repeat(pick, sizes)
    rest_n = n - target.size
    assert rest_n >= 0
    # the other buckets' singletons: valid keys (a point beyond max_range stays out unless clearing
    # rays are kept, so every one of the n points is an entry when allow_clear is on)
    other = np.flatnonzero((bk != bucket) & usable & (~far | (far_frac > 0)))
    rest = rng.choice(other, rest_n - 4 * straddle, replace=False)
    idx = np.concatenate([target, rest])
    pts = (centre[idx] + rng.uniform(-0.4, 0.4, (idx.size, 3)) * vs).astype(F)
    assert np.array_equal(voxel_of(pts, vs), cand[idx])  # the index rule on the fp32 points
    if straddle:
        cut = np.flatnonzero((np.abs(depth - max_range) < 0.1 * vs)
                             & (mg_bucket(voxel_key(cand, False), P) != bucket)
                             & (mg_bucket(voxel_key(cand, True), P) != bucket))
        sv = rng.choice(cut, straddle, replace=False)
        u = (centre[sv] - o) / depth[sv][:, None]  # along the ray: +-0.25 and +-0.35 voxel
        sp = np.concatenate([centre[sv] + t * vs * u for t in (-0.35, 0.25, -0.25, 0.35)]).astype(F)
        assert np.array_equal(voxel_of(sp, vs), np.tile(cand[sv], (4, 1)))
        pts = np.concatenate([pts, sp])
    pts = pts[rng.permutation(n)]
    facts = bucket_facts(pts, o, bucket, vs, max_range=max_range, allow_clear=allow_clear)
    return pts, facts


def chain_bricks(n, mask_bits, tail=8, seed=0, r=80):
    """n brick coordinates within +-r bricks of the origin whose home lies in the last `tail` slots
    of every table of 2^m slots, log2(tail) <= m <= mask_bits (the low hash bits are shared between
    the masks, so one set stays at the table's end across growth).  Returns (coords int32 (n, 3),
    facts of the set in a 2^mask_bits-slot table)."""
    assert tail & (tail - 1) == 0
    g, h = _brick_candidates(r)
    sel = np.flatnonzero((h & U((1 << mask_bits) - 1)) >= U((1 << mask_bits) - tail))
    assert sel.size >= n, sel.size
    sel = np.random.default_rng(seed).choice(sel, n, replace=False)
    coords = np.ascontiguousarray(g[sel], np.int32)
    return coords, chain_facts(coords, (1 << mask_bits) - 1, tail)


def chain_facts(coords, mask, tail=8):
    """A brick set in a (mask + 1)-slot table: how many homes lie in its last `tail` slots, and the
    probing of the set in the given order."""
    home = table_home(brick_key(coords), mask)
    _, longest, wraps = probe_runs(home, mask + 1)
    return dict(n=int(len(coords)), in_tail=int((home >= mask + 1 - tail).sum()),
                longest_probe=longest, wraps=bool(wraps))


def lds_chain_cloud(n_bricks, window, anchor=0, n_points=RPB, seed=0, vs=VS,
                    centre=(0.0, 0.0, 0.0), r=80, r_min=6):
    """At most RPB points (one front-end workgroup) whose end bricks are n_bricks distinct bricks
    with LDS brick-hash home in the cyclic range [anchor, anchor + window); anchor = HCAP - window
    puts the probe chain across the table's end.  The bricks lie within +-r bricks of the brick of
    `centre` and at least r_min bricks away from it.  Points are voxel centres plus a jitter below
    0.4 voxel, cycling over the bricks.  Returns (points float32, facts)."""
    assert n_points <= RPB
    rng = np.random.default_rng(seed)
    g, h = _brick_candidates(r)
    c0 = np.floor(np.asarray(centre, np.float64) / (8 * vs)).astype(np.int64)
    home = ((h >> U(40)) & U(HCAP - 1)).astype(np.int64)
    ok = (((home - anchor) % HCAP) < window) & (np.abs(g - c0).max(axis=1) >= r_min)
    sel = np.flatnonzero(ok)
    assert sel.size >= n_bricks, sel.size
    bricks = g[rng.choice(sel, n_bricks, replace=False)]
    b = bricks[np.arange(n_points) % n_bricks]
    vox = 8 * b + rng.integers(0, 8, (n_points, 3))
    order = rng.permutation(n_points)
    pts = ((vox[order] + 0.5 + rng.uniform(-0.4, 0.4, (n_points, 3))) * vs).astype(F)
    return pts, lds_facts(pts, anchor, window, vs)


def lds_facts(points, anchor, window, vs=VS):
    """The end bricks of a cloud in the workgroup's LDS brick hash: distinct bricks, how many have
    their home in the window, and the bounded probing (LDS_PROBES) of those in order of first
    appearance: the dropped ones take fallback pairs.  must_fall is the order-free lower bound: a
    key is placed within LDS_PROBES slots of its home, so the window's keys share
    window + LDS_PROBES - 1 slots."""
    b = np.floor(np.ascontiguousarray(points, F).astype(np.float64) / vs).astype(np.int64) >> 3
    uniq, first = np.unique(brick_key(b), return_index=True)
    uniq = uniq[np.argsort(first)]
    home = lds_home(uniq)
    inw = ((home - anchor) % HCAP) < window
    slots, longest, wraps = probe_runs(home[inw], HCAP, LDS_PROBES)
    _, longest_full, wraps_full = probe_runs(home[inw], HCAP)
    return dict(bricks=int(uniq.shape[0]), in_window=int(inw.sum()),
                fell=int((slots < 0).sum()), longest_probe=longest, wraps=bool(wraps),
                must_fall=max(0, int(inw.sum()) - (window + LDS_PROBES - 1)),
                longest_full=longest_full, wraps_full=bool(wraps_full))


# ---- the Merged pre-pass cases of tests/test_hash_adversarial_gpu.py -----------------------------
# name -> bucket_cloud keywords; every scan has 4096 points (P = 4), the target bucket is 0.
O = (0.012, 0.013, 0.011)  # the sensor's position in every case
MAX_RANGE = 8.0            # the clearing cases' range limit
_BITONIC = [(210, 2), (150, 3), (100, 4), (60, 5), (40, 6), (20, 7), (10, 8), (2, 9)]
SPECS = {
    # 2048 distinct keys: the table exactly full, 512 inserts on the re-read path, no member
    "full-table": dict(spec=[(MG_TAB, 1)]),
    # one key more than the table holds: OVF_MG
    "overflow": dict(spec=[(MG_TAB + 1, 1)]),
    # 1800 keys with their homes in the table's last 8 slots: chains across slot 2047 -> 0
    "wrap": dict(spec=[(1800, 1)], home=(MG_TAB - 8, 8)),
    # 512 and 513 members in bundles of 2..5: the rank sort's last size, the bitonic sort's first
    "rank-512": dict(spec=[(50, 2), (40, 3), (38, 4), (28, 5), (600, 1)]),
    "rank-513": dict(spec=[(49, 2), (41, 3), (38, 4), (28, 5), (600, 1)]),
    # 2048 members in 592 bundles of 2..9: the bitonic sort at N = MG_GM
    "bitonic-many": dict(spec=_BITONIC + [(300, 1)]),
    # one member more than the list holds, and 2600: the forward walk over many bundles
    "walk-2049": dict(spec=[(209, 2), (151, 3)] + _BITONIC[2:] + [(300, 1)]),
    "walk-2600": dict(spec=[(350, 3), (350, 4), (30, 5), (200, 1)]),
    # bitonic-many with a third of the target keys beyond max_range
    # and 8 voxels of the other buckets cut by max_range (a bundle and a clearing bundle each)
    "clearing": dict(spec=_BITONIC + [(300, 1)], far_frac=1 / 3, max_range=MAX_RANGE, straddle=8),
    "clearing-dropped": dict(spec=_BITONIC + [(300, 1)], far_frac=1 / 3, max_range=MAX_RANGE,
                             straddle=8, allow_clear=False),
}
N_SCAN = 4096


@functools.lru_cache(maxsize=None)
def spec_cloud(name):
    """(points, facts) of a case above; built once."""
    kw = dict(SPECS[name])
    seed = sorted(SPECS).index(name)
    pts, facts = bucket_cloud(N_SCAN, kw.pop("spec"), seed=seed, origin=O, **kw)
    pts.setflags(write=False)
    return pts, facts
