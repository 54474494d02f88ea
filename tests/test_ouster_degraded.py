"""The Ouster decoder on frames a sensor link really delivers: packets missing, reordered and
repeated, columns flagged invalid or carrying a measurement_id outside the frame, and pixel bytes
with every bit above every field mask set (tests/ousterpkt.py writes them).

On the CPU the writer is pinned as the inverse of oracle/ouster_ref.py on the five recorded
frames.  On the GPU tsdf_os_decode_device is called directly on images pre-filled with 0x6E6E6E6E
and followed by a guard row: every image must equal ouster_ref.decode_frames bit for bit (zero
where no valid column arrived), and the guard must come back untouched.  k_os_xyz runs past its
grid cap, and a degraded recorded frame is integrated end to end against the oracle.

Two different columns with the same measurement_id in one frame are not tested: separate
workgroups write them, so the result has no defined order (identical duplicates are included)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import ouster_ref as R
import ousterpkt as P
from test_ouster import FIXTURES, _frontend, load, pose

PROFILES = list(R.PROFILES)
FIELDS = ("RANGE", "SIGNAL", "REFLECTIVITY", "NEAR_IR")  # tsdf_os_decode_device's output order
FILL = 0x6E6E6E6E
MAIN = (40, 1024, 16)    # 64 packets; h = 40 leaves lanes of the 64-lane workgroup idle
ONE = (40, 1024, 128)    # the one-packet case: a packet of 128 columns, so that >= 100 are kept
SHAPES = [(16, 512, 16), (64, 2048, 16), (130, 1024, 8), (32, 1024, 16)]
CASES = ["clean", "third_missing", "one_packet", "empty", "status", "m_id", "reversed", "shuffled"]
# the cases that drop columns for a stated cause (>= 100 of them, asserted)
CAUSE = {"third_missing", "one_packet", "empty", "status", "m_id"}


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def build(case, profile, shape=None):
    """(packets as handed to the decoder, (h, w, cpp), columns dropped for the case's cause)."""
    h, w, cpp = shape or (ONE if case == "one_packet" else MAIN)
    seed = seed_of(case, profile, h, w, cpp)
    fid, m, st, ts, px = P.random_frame(profile, h, w, cpp, seed)
    rng = np.random.default_rng(seed + 1)
    top = 0xFFFFFFFF if profile == "LEGACY" else 0xFFFF  # every bit of the profile's status field
    dropped = 0
    if case == "status":
        bad = np.arange(w) % 4 == 2                       # a quarter: bit 0 clear
        st[:] = np.where(np.arange(w) % 2 == 0, 1, top)   # the kept ones alternate 1 / all bits
        st[bad] = np.where(np.arange(bad.sum()) % 2 == 0, top - 1, 0)  # 0xFFFE (legacy: 32 bits)
        dropped = int(bad.sum())
    if case == "m_id":
        bad = rng.choice(w, 120, replace=False)
        m[bad] = np.resize(np.array([w, w + 1, 0xFFFF], np.uint64), bad.size)
        dropped = bad.size
    pk = P.write_frame(profile, h, w, cpp, fid, m, st, ts, px, pad=rng)
    n = len(pk)
    assert n == w // cpp and len(pk[0]) == R.layout(profile, h, cpp)[5]
    if case == "third_missing":
        pk = [p for i, p in enumerate(pk) if i % 3 != 0 and i not in (0, n - 1)]
    elif case == "one_packet":
        pk = [pk[3]]
    elif case == "empty":
        pk = []
    elif case == "reversed":
        pk = pk[::-1]
    elif case == "shuffled":
        order = np.concatenate([rng.permutation(n), rng.integers(0, n, 3)])  # 3 identical repeats
        pk = [pk[i] for i in order]
    if case in ("third_missing", "one_packet", "empty"):
        dropped = (n - len(pk)) * cpp
    return pk, (h, w, cpp), dropped


def reference(pk, profile, h, w, cpp):
    """The four images as uint32 (None for a field the profile lacks) and the kept column ids."""
    if pk:
        scans = R.decode_frames(pk, profile, h, w, cpp)
        assert len(scans) == 1
        _, m, st, _, _ = P.read_columns(pk, profile, h, cpp)
        kept = np.unique(m[(m < w) & ((st & np.uint64(1)) == 1)]).astype(np.int64)
    else:
        scans = [{f: np.zeros((h, w), dt) for f, dt in R.PROFILES[profile][2].items()}]
        kept = np.zeros(0, np.int64)
    ref = {f: scans[0][f].astype(np.uint32) if f in scans[0] else None for f in FIELDS}
    return ref, kept


def check_not_vacuous(case, ref, kept, dropped, w):
    """On the reference: >= 100 columns dropped for the case's cause, >= 100 kept (an empty frame
    keeps none by definition), every field of the profile non-zero in >= 100 kept columns, and
    every column that is not kept all zero."""
    if case in CAUSE:
        assert dropped >= 100, dropped
    if case == "empty":
        assert kept.size == 0
    else:
        assert kept.size >= 100, kept.size
    assert ref["RANGE"] is not None
    gone = np.setdiff1d(np.arange(w), kept)
    for f, a in ref.items():
        if a is None:
            continue
        assert not a[:, gone].any(), f
        if case != "empty":
            assert int(a[:, kept].any(0).sum()) >= 100, f


# ---- CPU: the writer is the inverse of the reference decoder ------------------------------------

@pytest.mark.parametrize("js", FIXTURES, ids=[os.path.basename(f) for f in FIXTURES])
def test_writer_round_trip_on_the_fixtures(js):
    meta, fmt, digest, packets = load(js)
    size = R.layout(fmt.profile_name, fmt.h, fmt.columns_per_packet)[5]
    pk = [p for p in packets if len(p) == size]
    fid, m, st, ts, px = P.read_columns(pk, fmt.profile_name, fmt.h, fmt.columns_per_packet)
    again = P.write_frame(fmt.profile_name, fmt.h, fmt.w, fmt.columns_per_packet, fid, m, st, ts,
                          px, pad=np.random.default_rng(5))
    assert len(again) == len(pk) and all(len(p) == size for p in again)
    scans = R.decode_frames(again, fmt.profile_name, fmt.h, fmt.w, fmt.columns_per_packet)
    assert len(scans) == 1
    got, want = R.scan_digest(scans[0]), digest["scans"][0]
    keys = [k for k in want if k in got]
    assert "RANGE" in keys and "FRAME_ID" in keys and len(keys) >= 4
    for k in keys:
        assert got[k] == want[k], k
    # and the columns read back from the written packets are the ones written
    back = P.read_columns(again, fmt.profile_name, fmt.h, fmt.columns_per_packet)
    assert back[0] == fid
    for a, b in zip(back[1:], (m, st, ts, px)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("profile", PROFILES)
def test_writer_packet_size_is_the_library_s(profile):
    from tsdf_map import _abi, load_hip_library
    lib = load_hip_library()
    for h, w, cpp in [MAIN, ONE] + SHAPES:
        fmt = _abi.OsFormat(_abi.OS_PROFILES[profile], h, cpp, w)
        n = C.c_uint32()
        assert lib.tsdf_os_packet_bytes(C.byref(fmt), C.byref(n)) == 0
        fid, m, st, ts, px = P.random_frame(profile, h, cpp, cpp, 1)  # one packet of the frame
        pk = P.write_frame(profile, h, w, cpp, fid, m, st, ts, px)
        assert len(pk) == 1 and len(pk[0]) == n.value == R.layout(profile, h, cpp)[5]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("case", CASES)
def test_cases_are_not_vacuous(case, profile):
    """What the GPU tests assert on the reference, checked here without a GPU as well."""
    pk, (h, w, cpp), dropped = build(case, profile)
    ref, kept = reference(pk, profile, h, w, cpp)
    check_not_vacuous(case, ref, kept, dropped, w)
    if case in ("reversed", "shuffled"):
        clean, _ = reference(sorted(set(pk), key=lambda p: P.read_columns(
            [p], profile, h, cpp)[1][0]), profile, h, w, cpp)
        for f in FIELDS:
            assert (ref[f] is None) == (clean[f] is None)
            assert ref[f] is None or np.array_equal(ref[f], clean[f])
    if case == "clean":  # every bit above every mask is set somewhere: the masks matter
        _, _, _, _, px = P.read_columns(pk, profile, h, cpp)
        assert np.all(np.bitwise_or.reduce(px.reshape(-1, px.shape[-1]), 0) == 0xFF)


# ---- GPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vol():
    from tsdf_map import HipTSDFVolume
    v = HipTSDFVolume(0.05, 0.15, max_points=4096, max_bricks=1024)
    yield v
    v.close()


def decode_guarded(vol, profile, shape, pk, null=()):
    """tsdf_os_decode_device on images pre-filled with FILL and followed by a guard row:
    ({field: (h, w) uint32 or None where the pointer was null}, {field: guard row})."""
    import torch
    from tsdf_map import _abi
    h, w, cpp = shape
    dev = torch.device(vol.tensor_device)
    fmt = _abi.OsFormat(_abi.OS_PROFILES[profile], h, cpp, w)
    buf = None
    if pk:
        buf = torch.from_numpy(np.frombuffer(b"".join(pk), np.uint8).copy()).to(dev)
    imgs = {f: torch.full((h + 1, w), FILL, dtype=torch.int32, device=dev)
            for f in FIELDS if f not in null}
    torch.cuda.synchronize(dev)  # uploads and fills ran on torch's stream
    ptr = [C.c_void_p(imgs[f].data_ptr()) if f in imgs else None for f in FIELDS]
    rc = vol._lib.tsdf_os_decode_device(vol._ctx, C.byref(fmt),
                                        C.c_void_p(buf.data_ptr()) if pk else None, len(pk), *ptr)
    vol._check(rc, "os_decode")
    vol.sync()
    out = {f: (imgs[f].cpu().numpy().view(np.uint32) if f in imgs else None) for f in FIELDS}
    return ({f: None if a is None else a[:h] for f, a in out.items()},
            {f: None if a is None else a[h] for f, a in out.items()})


def assert_images(got, guard, ref, null=()):
    for f in FIELDS:
        if f in null:
            assert got[f] is None
            continue
        assert np.all(guard[f] == FILL), f
        if ref[f] is None:
            assert not got[f].any(), f  # a field the profile lacks: all zero
        else:
            assert np.array_equal(got[f], ref[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("case", CASES)
def test_gpu_degraded_frames_bitwise(vol, case, profile):
    pk, shape, dropped = build(case, profile)
    ref, kept = reference(pk, profile, *shape)
    check_not_vacuous(case, ref, kept, dropped, shape[1])
    got, guard = decode_guarded(vol, profile, shape, pk)
    assert_images(got, guard, ref)
    if case == "empty":
        assert all(not got[f].any() for f in FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("null", [("SIGNAL",), ("SIGNAL", "REFLECTIVITY", "NEAR_IR")],
                         ids=["no_signal", "range_only"])
def test_gpu_null_outputs(vol, profile, null):
    pk, shape, dropped = build("third_missing", profile)
    ref, kept = reference(pk, profile, *shape)
    check_not_vacuous("third_missing", ref, kept, dropped, shape[1])
    got, guard = decode_guarded(vol, profile, shape, pk, null=null)
    assert_images(got, guard, ref, null=null)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_gpu_shapes(vol, shape):
    """h = 16 (a quarter wave), h = 130 (the 128-lane loop twice, a short second pass), w = 512
    and 2048, 8 columns per packet; a third of the packets missing, so the memset matters."""
    profile = "RNG19_RFL8_SIG16_NIR16_DUAL"
    pk, shape, dropped = build("third_missing", profile, shape)
    ref, kept = reference(pk, profile, *shape)
    check_not_vacuous("third_missing", ref, kept, dropped, shape[1])
    got, guard = decode_guarded(vol, profile, shape, pk)
    assert_images(got, guard, ref)


XYZ_FILL = -7.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 8192 * 256 + 77])
def test_gpu_xyz_past_the_grid_cap(vol, n):
    """k_os_xyz strides over a grid capped at 8192 x 256 lanes: with 77 pixels more, 77 lanes run
    the loop body twice.  Bitwise against r dir + off (0 where r = 0) and the fp32 pose."""
    import torch
    dev = torch.device(vol.tensor_device)
    rng = np.random.default_rng(seed_of("xyz", n))
    r = rng.integers(0, 1 << 19, n, dtype=np.uint32)
    r[rng.random(n) < 0.1] = 0
    lut_d = rng.uniform(-1e-3, 1e-3, (n, 3)).astype(np.float32)
    lut_o = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    T = np.concatenate([np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.uniform(-20, 20, (3, 1))], 1)
    if n > 1:
        assert 0.05 < (r == 0).mean() < 0.15 and (r >= 1 << 18).any()
    d_r = torch.from_numpy(r.view(np.int32)).to(dev)
    d_d, d_o = torch.from_numpy(lut_d).to(dev), torch.from_numpy(lut_o).to(dev)
    xyz = torch.full((n + 1, 3), XYZ_FILL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if n else None  # noqa: E731
    m = np.ascontiguousarray(T).reshape(12)
    vol._check(vol._lib.tsdf_os_cartesian_device(vol._ctx, p(d_r), n, p(d_d), p(d_o),
                                                 m.ctypes.data_as(C.POINTER(C.c_double)), p(xyz)),
               "os_cartesian")
    vol.sync()
    g = xyz.cpu().numpy()
    assert np.all(g[n] == XYZ_FILL)  # nothing written past n
    s = R.cartesian_f32(r, lut_d, lut_o)
    mf = T.astype(np.float32)
    want = np.stack([mf[i, 0] * s[:, 0] + mf[i, 1] * s[:, 1] + mf[i, 2] * s[:, 2] + mf[i, 3]
                     for i in range(3)], 1).astype(np.float32)
    assert np.array_equal(g[:n].view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_gpu_degraded_frame_end_to_end():
    """The OS-2-128 recording with every third packet removed and a quarter of the remaining
    columns flagged invalid (bit 0 of their status bytes cleared), decoded, projected and
    integrated on the GPU: the oracle's field of the reference points, and as many rays as the
    reference has non-zero ranges."""
    import oracle
    js = [f for f in FIXTURES if "OS-2-128" in f][0]
    meta, fmt, digest, packets = load(js)
    vol, fe = _frontend(meta)
    (fid, pk), = fe.frames(packets)
    ph, ch, cf, pf, col, size = R.layout(fmt.profile_name, fmt.h, fmt.columns_per_packet)
    pk = [bytearray(p) for i, p in enumerate(pk) if i % 3 != 0]
    k = 0
    for p in pk:
        for icol in range(fmt.columns_per_packet):
            if k % 4 == 1:
                p[ph + icol * col + (col - 4 if fmt.legacy else 10)] &= 0xFE
            k += 1
    pk = [bytes(p) for p in pk]
    ref = R.decode_frames(pk, fmt.profile_name, fmt.h, fmt.w, fmt.columns_per_packet)[0]
    _, m, st, _, _ = P.read_columns(pk, fmt.profile_name, fmt.h, fmt.columns_per_packet)
    ok = (st & np.uint64(1)) == 1
    assert (~ok).sum() == k // 4 >= 100 and ok.sum() >= 100 and fmt.w - k >= 100
    assert not ref["RANGE"][:, m[~ok].astype(np.int64)].any()
    nz = int(np.count_nonzero(ref["RANGE"]))
    assert nz > 10000
    P4 = pose(1)
    imgs, xyz = fe.integrate_frame(pk, P4)
    fe.sync()
    assert np.array_equal(imgs["RANGE"].cpu().numpy().view(np.uint32),
                          ref["RANGE"].astype(np.uint32))
    s = R.cartesian_f32(ref["RANGE"], fe.lut_dir.cpu().numpy(), fe.lut_off.cpu().numpy())
    mf = P4[:3, :4].astype(np.float32)
    w = np.stack([mf[i, 0] * s[:, 0] + mf[i, 1] * s[:, 1] + mf[i, 2] * s[:, 2] + mf[i, 3]
                  for i in range(3)], 1).astype(np.float32)
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), w.view(np.uint32))
    o = oracle.OracleTSDFVolume(0.05, 0.15, min_range=1e-3)
    o.integrate(w, P4[:3, 3])
    assert o.export_voxels()[0].shape[0] > 10000
    for x, y in zip(vol.export_voxels(), o.export_voxels()):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32),
                              np.ascontiguousarray(y).view(np.uint32))
    assert vol.stats()["n_rays_total"] == nz
    vol.close()
