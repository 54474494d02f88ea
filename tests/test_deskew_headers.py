"""The column headers of a frame's packets (tsdf_os_headers, noetic-slam_amd/csrc/os_headers.h;
tsdf_map.ouster.column_headers): pinned by the reference's golden digests on the five recorded
frames, held to a numpy restatement (tests/deskewref.py) on degraded synthetic frames, and run
under the sanitizers as a stand-alone program (tests/cpp/os_headers_check.cpp).  CPU suite."""
import glob
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import deskewref as D
import ouster_ref as R
import ousterpkt
from conftest import GOLDEN, REPO

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ouster", "*[0-9].json")))
SRC = os.path.join(REPO, "tests", "cpp", "os_headers_check.cpp")
PROFILES = list(R.PROFILES)
H, W, CPP = 8, 64, 16


def load(js):
    from tsdf_map.ouster import OusterFormat, read_pcap
    fmt = OusterFormat(json.load(open(js)))
    digest = json.load(open(js.replace(".json", "_digest.json")))
    size = R.layout(fmt.profile_name, fmt.h, fmt.columns_per_packet)[5]
    packets = [p for p in read_pcap(js.replace(".json", ".pcap"), fmt.port) if len(p) == size]
    return fmt, digest, packets


def synthetic_format(profile, h=H, w=W, cpp=CPP):
    from tsdf_map.ouster import OusterFormat
    return OusterFormat(D.synthetic_meta(profile, h, w, cpp))


def same(got, want):
    for g, x, dt in zip(got, want, (np.uint64, np.uint32, np.uint16)):
        assert g.dtype == dt and np.array_equal(g, x)


@pytest.mark.parametrize("js", FIXTURES, ids=[os.path.basename(f) for f in FIXTURES])
def test_golden_digests_of_timestamp_and_measurement_id(js):
    from tsdf_map.ouster import column_headers
    fmt, digest, packets = load(js)
    ts, st, mid = column_headers(packets, fmt)
    want = digest["scans"][0]
    assert ts.dtype == np.uint64 and mid.dtype == np.uint16 and ts.shape == (fmt.w,)
    assert hashlib.md5(ts.tobytes()).hexdigest() == want["TIMESTAMP"]
    assert hashlib.md5(mid.tobytes()).hexdigest() == want["MEASUREMENT_ID"]
    # STATUS is held to the restatement, not to its digest
    same((ts, st, mid), D.headers_ref(packets, fmt.profile_name, fmt.h, fmt.w,
                                      fmt.columns_per_packet))
    assert np.count_nonzero(st & 1) > 0


def degraded(profile, seed):
    """A frame with status-0 columns, ids >= w and random bytes wherever nothing should read."""
    rng = np.random.default_rng(seed)
    fid, m_id, status, ts, px = ousterpkt.random_frame(profile, H, W, CPP, seed)
    status = rng.integers(0, 1 << (32 if profile == "LEGACY" else 16), W).astype(np.uint64) | 1
    ts = rng.integers(1, 1 << 63, W).astype(np.uint64)
    status[[3, 17, 40]] &= ~np.uint64(1)     # invalid columns (the other status bits stay set)
    status[21] = 0
    m_id[[9, 50]] = [W, 0xFFFF]              # ids past the frame
    return ousterpkt.write_frame(profile, H, W, CPP, fid, m_id, status, ts, px, pad=rng)


@pytest.mark.parametrize("profile", PROFILES)
def test_degraded_frames_equal_the_restatement(profile):
    from tsdf_map.ouster import column_headers
    fmt = synthetic_format(profile)
    packets = degraded(profile, 11)
    want = D.headers_ref(packets, profile, H, W, CPP)
    same(column_headers(packets, fmt), want)
    assert not want[1][[3, 17, 40, 21, 9, 50]].any() and not want[0][[3, 9]].any()
    assert np.count_nonzero(want[2]) == W - 7  # six columns dropped; column 0's id is 0
    # shuffled packets: the same arrays (each column goes to its id)
    order = np.random.default_rng(5).permutation(len(packets))
    assert not np.array_equal(order, np.arange(len(packets)))
    same(column_headers([packets[i] for i in order], fmt), want)
    # a dropped packet: its columns stay zero
    less = packets[:1] + packets[2:]
    got = column_headers(less, fmt)
    same(got, D.headers_ref(less, profile, H, W, CPP))
    assert not got[0][CPP:2 * CPP].any() and not got[1][CPP:2 * CPP].any()
    # no packets: all zero
    same(column_headers([], fmt), D.headers_ref([], profile, H, W, CPP))


def test_bad_format_raises():
    from tsdf_map.ouster import column_headers
    fmt = synthetic_format("LEGACY")
    fmt.c.profile = 9
    with pytest.raises(ValueError):
        column_headers([], fmt)


def _run(exe, args, timeout):
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
    return out


def _fixture_args(tmp_path):
    from tsdf_map import _abi
    fmt, digest, packets = load([f for f in FIXTURES if "OS-2-128" in f][0])
    pk = tmp_path / "packets.bin"
    pk.write_bytes(b"".join(packets))
    args = [str(_abi.OS_PROFILES[fmt.profile_name]), str(fmt.h), str(fmt.columns_per_packet),
            str(fmt.w), str(pk), str(tmp_path / "out.bin")]
    return fmt, packets, args


def _check_out(fmt, packets, path):
    b = open(path, "rb").read()
    w = fmt.w
    got = (np.frombuffer(b, np.uint64, w), np.frombuffer(b, np.uint32, w, 8 * w),
           np.frombuffer(b, np.uint16, w, 12 * w))
    assert len(b) == 14 * w
    same(got, D.headers_ref(packets, fmt.profile_name, fmt.h, fmt.w, fmt.columns_per_packet))


def test_os_headers_check(tmp_path):
    """os_headers.h compiles with plain g++ (no HIP) and holds its own restatement."""
    exe = tmp_path / "os_headers_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    fmt, packets, args = _fixture_args(tmp_path)
    _run(exe, args, 120)
    _check_out(fmt, packets, args[-1])


def test_os_headers_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer, over a recorded
    frame's packets and over random-byte packets in buffers of the exact size: no read past a
    packet, no write past the w entries, no misaligned or overflowing arithmetic."""
    exe = tmp_path / "os_headers_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    fmt, packets, args = _fixture_args(tmp_path)
    out = _run(exe, args, 300)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
    _check_out(fmt, packets, args[-1])
