"""A context's life from tsdf_create to tsdf_destroy (tsdf_capi.cpp: the owners of its device
memory, the sizing plan's refusals): a refused create leaves nothing behind, every buffer family is
built, used and torn down in every mode that has one, and a context that grew gives its memory
back."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import decimate

pytestmark = pytest.mark.gpu

VS, TAU = 0.05, 0.15
MIB = 1 << 20


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume(kw.pop("voxel_size", VS), kw.pop("sdf_trunc", TAU), **kw)


def bitwise(g, o):
    gi, gs, gw = g.export_voxels()
    oi, os_, ow = o.export_voxels()
    return (gi.shape == oi.shape and gi.shape[0] > 0 and np.array_equal(gi, oi)
            and np.array_equal(gw, ow) and np.array_equal(gs.view(np.uint32), os_.view(np.uint32)))


# 1: more pair slots per ray (2 cm voxels carved over 120 m) than the 32-bit pair index leaves room
# for 2^22 points; 2: a scan of 2^27 points against the 2^30 samples a span record addresses
REFUSALS = [
    (dict(voxel_size=0.02, sdf_trunc=0.06, space_carving=True, max_range=120.0, max_points=1 << 22),
     "exceeds what one batch can hold"),
    (dict(voxel_size=VS, sdf_trunc=TAU, walk="single", max_points=1 << 27, max_batch=2),
     "exceeds a single-walk batch"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=["batch", "single-walk"])
def test_create_refusals_keep_code_and_text(capfd, scan0, kw, text):
    from tsdf_map import HipTSDFVolume, _abi, load_hip_library
    lib = load_hip_library()
    kw = dict(kw)
    p = HipTSDFVolume.make_params(lib, kw.pop("voxel_size"), kw.pop("sdf_trunc"), **kw)
    ctx = C.c_void_p()
    capfd.readouterr()
    rc = lib.tsdf_create(C.byref(p), C.byref(ctx))
    err = capfd.readouterr().err
    assert rc == _abi.TSDF_EINVAL
    assert not ctx.value  # the context pointer stays null
    assert "tsdf_create: max_points %d %s" % (p.max_points, text) in err
    # the next ordinary create succeeds
    pts = decimate(scan0[0], 64)
    with hip(max_bricks=4096, max_points=1 << 14) as g:
        g.integrate(pts, scan0[1])
        g.sync()
        assert g.stats()["n_bricks"] > 0


# one mode per buffer family: the two-walk lists; the single walk's 64-bit cells, regions and span
# list; 12-byte sample records; the merged pre-pass' buffers; the sector flags' block list
MODES = {
    "default": dict(),
    "single-walk": dict(walk="single"),
    "voxblox-simple": dict(semantics="voxblox", max_range=40.0),
    "voxblox-merged": dict(semantics="voxblox", method="merged", max_range=40.0),
    "sectors": dict(n_sectors=4, sector=0, sector_rule="world"),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_every_buffer_family_is_built_and_torn_down(scan0, mode):
    kw = MODES[mode]
    pts, org = decimate(scan0[0], 16), scan0[1]
    okw = {k: v for k, v in kw.items() if k != "walk"}
    o = oracle.OracleTSDFVolume(VS, TAU, **okw)
    o.integrate(pts, org)
    g = hip(max_batch=2, max_points=1 << 14, max_bricks=4096, **kw)
    try:
        g.integrate(pts, org)
        g.sync()
        assert bitwise(g, o)
    finally:
        g.close()


def _sector_inputs(sim, n):
    """test_growth.py::test_sector_sample_list_grows' inputs: n scans' points of sector 0 of 8."""
    import torch
    from tsdf_map import sector_ids
    scans = []
    for k in range(n):
        p, o = sim.scan(k)
        scans.append((np.ascontiguousarray(p[sector_ids(p, o, 8, 0.0) == 0]), o))
    offs = np.cumsum([0] + [p.shape[0] for p, _ in scans]).astype(np.uint64)
    d = torch.from_numpy(np.concatenate([p for p, _ in scans])).to("cuda:0")
    return d, offs, np.stack([o for _, o in scans])


# what the parent commit's library loses over the same four cycles (measured on an MI355X: +0 bytes
# after each of the three further cycles), and the allowance: its largest drop plus one 2 MiB
# allocation granule
PARENT_LARGEST_DROP = 0
MARGIN = PARENT_LARGEST_DROP + 2 * MIB


def test_destroy_after_growth_returns_the_memory(sim, scan0):
    """Contexts that grew their pool (4096 bricks against a full C1 scan) and, sharded, their sample
    lists (two walks: the list; single walk: the k_walk regions) are destroyed; the device's free
    memory after each of three further cycles is no lower than after the warm-up cycle, within
    MARGIN.  On the parent commit's library the same four cycles' largest drop is
    PARENT_LARGEST_DROP = 0 bytes (this tree's: 0 as well); MARGIN = 2 MiB adds one allocation
    granule to it.

    At stake are buffers of tens of MiB each (a 4096-brick pool is 32 MiB before it grows, a lane's
    run lists about 64 MiB, the sample lists more): a leaked family stands well clear of the margin.
    The test does NOT see the leak of a KiB-sized buffer, nor one smaller than the margin."""
    import torch
    # 4 sectors where that overflows the list; the two walks' list of a 4-sector context (1.44 M
    # slots for 8 x 2^15 points) holds these 6 scans' samples, so it is sized for 8 sectors, as in
    # test_sector_sample_list_grows
    inputs = {"two": (_sector_inputs(sim, 6), dict(n_sectors=8, max_batch=8, max_points=1 << 15)),
              "single": (_sector_inputs(sim, 64), dict(n_sectors=4, max_batch=64, max_points=1 << 15))}
    torch.cuda.synchronize()

    def cycle():
        g = hip(max_bricks=4096, max_batch=2)
        g.integrate(*scan0)
        g.sync()
        assert g.stats()["n_grows"] >= 1
        g.close()
        for walk, ((d, offs, org), kw) in inputs.items():
            # (the default pool: every growth counted here is a sample list's)
            g = hip(sector=0, sector_rule="world", walk=walk, **kw)
            g.integrate_batch_device(d.data_ptr(), offs, org)
            g.sync()
            assert g.stats()["n_grows"] >= 1
            g.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    base = cycle()  # warm-up: the runtime's own pools and code objects are resident after it
    drops = []
    for k in range(3):
        drops.append(base - cycle())
        print("cycle %d: free memory %+d bytes against the warm-up cycle" % (k + 1, -drops[-1]))
    assert max(drops) <= MARGIN, drops
