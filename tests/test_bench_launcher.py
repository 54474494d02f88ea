"""bench.py's own multi-rank launcher (`python3 bench.py --gpus N` with no torchrun): N rank
processes with the torch.distributed environment, the status of the first failing rank, and the
refusal to print a line whose n_gpus is not the world that ran."""
import os
import subprocess
import sys
import textwrap

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_check_world_refuses_mismatch():
    bench.check_world(2, 2)
    with pytest.raises(SystemExit):
        bench.check_world(8, 1)


def test_launch_ranks_env(tmp_path):
    out = tmp_path / "ranks"
    out.mkdir()
    child = tmp_path / "child.py"
    child.write_text(textwrap.dedent("""
        import os, sys
        keys = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
        with open(os.path.join(sys.argv[1], os.environ["RANK"]), "w") as f:
            f.write(" ".join(os.environ[k] for k in keys))
    """))
    assert bench.launch_ranks(3, script=str(child), argv=[str(out)]) == 0
    got = sorted(os.listdir(out))
    assert got == ["0", "1", "2"]
    rows = [open(out / r).read().split() for r in got]
    assert [r[0] for r in rows] == ["0", "1", "2"] and all(r[1] == r[0] for r in rows)
    assert all(r[2] == "3" and r[3] == "127.0.0.1" for r in rows)
    assert len({r[4] for r in rows}) == 1  # one rendezvous port


def test_launch_ranks_failure_stops_the_others(tmp_path):
    child = tmp_path / "child.py"
    child.write_text(textwrap.dedent("""
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(3)
        time.sleep(60)  # would wait at a barrier for the failed rank
    """))
    import time
    t = time.time()
    assert bench.launch_ranks(2, script=str(child), argv=[]) == 3
    assert time.time() - t < 30


def test_bench_gpus2_without_launcher_sets_world(tmp_path):
    """The real script with --gpus 2 and no WORLD_SIZE spawns two ranks (they fail here at the
    first GPU call: no device on the CPU runner), never one rank reporting n_gpus 1."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1",
                        "--warmup", "0", "--no-cpu"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert '"n_gpus"' not in r.stdout


def test_traffic_file_is_used_only_for_its_own_build(tmp_path, monkeypatch):
    """roofline.traffic comes from a PMC run only when that run measured THIS library build
    (VERDICT r3 weak #8): the committed profiles/traffic_r04.json carries the sha of the shipped
    libtsdf_hip.so, and a file of another build (or an unreadable one) yields None, with the reason
    in traffic_source."""
    import json
    lib = tmp_path / "libfake.so"
    lib.write_bytes(b"kernels v1")
    monkeypatch.setenv("TSDF_HIP_LIB", str(lib))
    sha = bench.lib_sha16()
    good = tmp_path / "t.json"
    good.write_text(json.dumps({"lib_sha16": sha, "bytes_per_launch": {"k_count": 123}}))
    val, src = bench.read_traffic(str(good), "count")
    assert val == 123 and src["matches_build"] and src["this_build_sha16"] == sha
    lib.write_bytes(b"kernels v2")  # the kernels changed after the PMC run
    val, src = bench.read_traffic(str(good), "count")
    assert val is None and not src["matches_build"]
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    val, src = bench.read_traffic(str(bad), "count")
    assert val is None and src["error"] == "unreadable"


def test_full_and_dump_options(monkeypatch):
    """A plain run is lean: `--full` (the serial leg, parity, CPU baseline) and `--dump-outputs`
    are off unless asked for."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "out")


def test_dump_outputs_sample_and_totals(tmp_path, monkeypatch):
    """dump_outputs on a stand-in brick map: float32 / float64 .npy files, S zeroed where W == 0,
    totals over every brick, and a brick sample that depends only on the bricks' own coordinates
    (the same bricks are picked from a map that holds more), in (z, y, x) export order."""
    import numpy as np

    class Vol:
        def __init__(self, n):
            r = np.random.default_rng(5)
            self.c = np.unique(r.integers(-40, 40, (n, 3)).astype(np.int32), axis=0)
            self.c = self.c[np.lexsort((self.c[:, 0], self.c[:, 1], self.c[:, 2]))]
            k = np.arange(self.c.shape[0] * 512, dtype=np.float32).reshape(-1, 8, 8, 8)
            key = (self.c[:, 0] * 7 + self.c[:, 1] * 3 + self.c[:, 2]).astype(np.float32)
            self.w = (k % 3) * (1 + np.abs(key))[:, None, None, None]
            self.s = np.full_like(self.w, -0.25) * (1 + (key % 5))[:, None, None, None]

        def export_bricks(self):
            return self.c, self.s, self.w

    monkeypatch.setattr(bench, "DUMP_BRICKS", 16)
    big = Vol(400)
    bench.dump_outputs(big, str(tmp_path / "a"))
    got = {n: np.load(tmp_path / "a" / (n + ".npy"))
           for n in ("brick_coords", "brick_sdf", "brick_weight", "field_totals")}
    assert got["brick_coords"].dtype == np.float64 and got["field_totals"].dtype == np.float64
    assert got["brick_sdf"].dtype == np.float32 and got["brick_weight"].dtype == np.float32
    assert got["brick_coords"].shape == (16, 3) and got["brick_sdf"].shape == (16, 8, 8, 8)
    seen = big.w > 0
    assert got["field_totals"].tolist() == [big.c.shape[0], np.count_nonzero(seen),
                                            big.w.sum(dtype=np.float64),
                                            np.abs(big.s[seen]).sum(dtype=np.float64)]
    # each sampled brick is the map's brick of those coordinates, S zeroed where W == 0
    rows = [int(np.flatnonzero((big.c == c).all(1))[0]) for c in got["brick_coords"]]
    assert rows == sorted(rows)
    assert np.array_equal(got["brick_weight"], big.w[rows])
    assert np.array_equal(got["brick_sdf"], np.where(seen[rows], big.s[rows], 0))
    assert np.all(got["brick_sdf"][got["brick_weight"] == 0] == 0)
    # a map without some bricks outside the sample gives the same sample
    small = Vol(400)
    keep = np.ones(small.c.shape[0], bool)
    keep[[i for i in range(small.c.shape[0]) if i not in rows][::2]] = False
    small.c, small.s, small.w = small.c[keep], small.s[keep], small.w[keep]
    bench.dump_outputs(small, str(tmp_path / "b"), suffix="_rank1")
    assert np.array_equal(np.load(tmp_path / "b" / "brick_coords_rank1.npy"), got["brick_coords"])
    assert np.array_equal(np.load(tmp_path / "b" / "brick_sdf_rank1.npy"), got["brick_sdf"])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_field(tmp_path, monkeypatch, capsys):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps and runs none of the
    `--full` legs; `--dump-outputs` writes the timed context's field, which is the oracle's on the
    same scans (the warmup and the timed steps, bit for bit on the sampled bricks)."""
    import json
    import numpy as np
    import torch
    import oracle
    from tsdf_map.scan_gen import TorchOusterSim
    from tsdf_map.volume import bricks_to_voxels

    out = tmp_path / "dump"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                      "--batch", "2", "--dump-outputs", str(out)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 2 / (2 * line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert line["roofline"] is None and line["parity"] is None and line["cpu_baseline"] is None
    assert line["serial_kernel_ms_per_launch"] is None
    coords = np.load(out / "brick_coords.npy")
    s, w = np.load(out / "brick_sdf.npy"), np.load(out / "brick_weight.npy")
    totals = np.load(out / "field_totals.npy")
    assert totals[0] == line["bricks"] and coords.shape[0] == min(line["bricks"], bench.DUMP_BRICKS)
    assert sum(a.nbytes for a in (coords, s, w, totals)) <= 64 << 20
    sim = TorchOusterSim(torch.device("cuda", 0))
    ov = oracle.OracleTSDFVolume(0.05, 0.15, semantics="vdbfusion_f64", threads=8)
    for k in range(6):  # (1 warmup + 2 timed) steps x 2 scans
        p, o = sim.scan(k)
        ov.integrate(p.cpu().numpy(), o)
    oi, os_, ow = ov.export_voxels()
    assert totals[1] == oi.shape[0]
    assert totals[2] == pytest.approx(ow.sum(dtype=np.float64), rel=1e-12)
    gi, gs, gw = bricks_to_voxels(coords.astype(np.int32), s, w)

    def key(b):  # one int64 per brick coordinate triple
        b = b.astype(np.int64) + (1 << 20)
        return (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]

    inb = np.isin(key(oi.astype(np.int64) >> 3), key(coords))  # the oracle's voxels in the sample
    assert gi.shape[0] > 0 and np.array_equal(gi, oi[inb])
    assert np.array_equal(gw.view(np.uint32), ow[inb].view(np.uint32))
    assert np.array_equal(gs.view(np.uint32), os_[inb].view(np.uint32))


def test_voxblox_method_and_weight_options(monkeypatch):
    """`--semantics voxblox --method merged` and `--const-weight` (round 5) reach
    the bench's arguments; the defaults are Simple with 1/z^2 weights, and a bad method is refused."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--semantics", "voxblox", "--method", "merged",
                                      "--const-weight"])
    a = bench.parse()
    assert (a.semantics, a.method, a.const_weight) == ("voxblox", "merged", True)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--semantics", "voxblox"])
    a = bench.parse()
    assert (a.method, a.const_weight) == ("simple", False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--method", "fast"])
    with pytest.raises(SystemExit):
        bench.parse()
