"""Ouster lidar-packet writer (test helper): the inverse of oracle/ouster_ref.py's layout.

`write_frame` lays columns (measurement_id, status, timestamp, raw pixel bytes) out as the UDP
lidar packets of one frame, per profile: the status goes where the profile reads it (the legacy
column footer, 4 bytes; else the column header at byte 10, 2 bytes), the frame id into the packet
header at byte 2 (legacy: every column header at byte 10).  `read_columns` is its inverse on
recorded packets, and `random_frame` draws a frame whose pixel bytes are uniform random, so every
bit above every field mask is set somewhere.  Bytes no decoder reads (the rest of the headers, the
packet footer) are random too when an rng is given: a decoder that read them would show.
"""
import numpy as np

import ouster_ref as R


def write_frame(profile, h, w, columns_per_packet, frame_id, measurement_id, status, timestamp,
                pixels, pad=None):
    """Columns -> a list of packet byte strings of ouster_ref.layout(...)[5] bytes each.
    measurement_id, status, timestamp: (n_cols,) integers; pixels: (n_cols, h, pixel bytes) uint8,
    the raw bytes of each pixel.  n_cols is a multiple of columns_per_packet; the columns go into
    the packets in the order given.  pad: a numpy Generator for the bytes nothing reads (None: 0).
    `w` only documents the frame; ids >= w are written as they are (the decoder drops them)."""
    pixel_bytes = R.PROFILES[profile][0]
    ph, ch, cf, pf, col, pkt = R.layout(profile, h, columns_per_packet)
    legacy = profile == "LEGACY"
    m_id = np.asarray(measurement_id, np.uint64).reshape(-1)
    st = np.asarray(status, np.uint64).reshape(-1)
    ts = np.asarray(timestamp, np.uint64).reshape(-1)
    px = np.asarray(pixels, np.uint8).reshape(m_id.size, h, pixel_bytes)
    assert m_id.size == st.size == ts.size and m_id.size % columns_per_packet == 0
    n_pk = m_id.size // columns_per_packet
    if pad is None:
        buf = np.zeros((n_pk, pkt), np.uint8)
    else:
        buf = pad.integers(0, 256, (n_pk, pkt), dtype=np.uint8)

    def put(view, value, nbytes):
        for k in range(nbytes):
            view[..., k] = ((value >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8)

    if not legacy:
        put(buf[:, 0:2], np.uint64(1), 2)               # packet type: lidar data
        put(buf[:, 2:4], np.uint64(frame_id), 2)
    body = buf[:, ph: ph + columns_per_packet * col]
    cols = body.reshape(n_pk * columns_per_packet, col).copy()  # (written back below)
    put(cols[:, 0:8], ts, 8)
    put(cols[:, 8:10], m_id, 2)
    if legacy:
        put(cols[:, 10:12], np.uint64(frame_id), 2)
        put(cols[:, col - 4: col], st, 4)
    else:
        put(cols[:, 10:12], st, 2)
    cols[:, ch: ch + h * pixel_bytes] = px.reshape(m_id.size, h * pixel_bytes)
    body[:] = cols.reshape(n_pk, columns_per_packet * col)
    return [buf[k].tobytes() for k in range(n_pk)]


def read_columns(packets, profile, h, columns_per_packet):
    """(frame_id of the first packet, measurement_id, status, timestamp, pixels) of recorded
    packets, every column in stream order: what `write_frame` takes."""
    pixel_bytes = R.PROFILES[profile][0]
    ph, ch, cf, pf, col, pkt = R.layout(profile, h, columns_per_packet)
    legacy = profile == "LEGACY"
    buf = np.stack([np.frombuffer(p, np.uint8) for p in packets])
    assert buf.shape[1] == pkt
    cols = buf[:, ph: ph + columns_per_packet * col].reshape(-1, col)

    def get(view):
        v = np.zeros(view.shape[0], np.uint64)
        for k in range(view.shape[1]):
            v |= view[:, k].astype(np.uint64) << np.uint64(8 * k)
        return v

    fid = int(get(cols[:1, 10:12])[0]) if legacy else int(get(buf[:1, 2:4])[0])
    status = get(cols[:, col - 4: col]) if legacy else get(cols[:, 10:12])
    px = cols[:, ch: ch + h * pixel_bytes].reshape(-1, h, pixel_bytes).copy()
    return fid, get(cols[:, 8:10]), status, get(cols[:, 0:8]), px


def random_frame(profile, h, w, columns_per_packet, seed, frame_id=0x1234):
    """The columns of a whole frame in order, all valid (status 1), with uniform random pixel
    bytes: (frame_id, measurement_id, status, timestamp, pixels) as `write_frame` takes them."""
    rng = np.random.default_rng(seed)
    pixel_bytes = R.PROFILES[profile][0]
    assert w % columns_per_packet == 0
    px = rng.integers(0, 256, (w, h, pixel_bytes), dtype=np.uint8)
    ts = np.uint64(10 ** 9) + np.arange(w, dtype=np.uint64) * np.uint64(97656)
    return frame_id, np.arange(w, dtype=np.uint64), np.ones(w, np.uint64), ts, px
