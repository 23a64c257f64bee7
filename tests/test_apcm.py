"""nfcgpu_apcm_encode (the resampler's control points as the radio-<id>.apcm entries of a trace file) through the C ABI, and the
binding around it.

Yardstick: a numpy restatement of the reference's TraceStorageTask::writeRadioEntry (TraceStorageTask.cpp:881-1003), written
here from the rules of include/nfcgpu.h and independent of the product code: entry_of(). Every comparison is byte equality; there
are no tolerances. The control points come from nfcgpu_resample_radio (tests/test_resample_radio.py holds that call against the
reference) or are made by hand.

The same file runs on the CPU against the emulated library (tests/test_apcm_emulated.py), whose twins of the kernels compile the
same nfc_apcm.hpp; test_twin_equals_device ties the two together byte for byte."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import nfc_testlib as T
import test_signal_tap as TS
from test_signal_tap import LOC_DEVICE, LOC_HOST, DeviceArray, on_emulated_library

pytestmark = pytest.mark.gpu

gpu = TS.gpu    # (module-scoped fixture: one context for this file)

EMU = TS.EMU
FS = 10000000
EINVAL, EOVERFLOW = -1, -6
GUARD = 0x5A
CHUNK = 1024    # NfcApcmShape::kChunk
SIZES = (25, 64, 255, 256, 257, 4099)


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------

def quantise(values):
    """nfc_record_quantise: static_cast<short>(v * 32768.0f) in range, saturated beyond it, a NaN as 0"""
    t = (np.asarray(values, dtype=np.float32) * np.float32(32768.0)).astype(np.float32)
    out = np.zeros(t.shape, dtype=np.int64)
    nan = np.isnan(t)
    high, low = ~nan & (t >= 32768.0), ~nan & (t <= -32769.0)
    rest = ~nan & ~high & ~low
    out[high], out[low] = 32767, -32768
    out[rest] = np.trunc(t[rest].astype(np.float64)).astype(np.int64)
    return out


def cast_offsets(offsets):
    """(uint32)pair.offset: a negative value or a NaN gives 0, the cast saturates above"""
    f = np.asarray(offsets, dtype=np.float32).astype(np.float64)
    out = np.zeros(f.shape, dtype=np.int64)
    ok = ~np.isnan(f) & (f > 0)
    out[ok] = np.minimum(np.trunc(f[ok]), 4294967295.0).astype(np.int64)
    return out


def sample_range(rate, range_start, range_end):
    if range_start == 0 and range_end == 0:
        return 0, 0xFFFFFFFF
    return int(np.float64(rate) * np.float64(range_start)), int(np.float64(rate) * np.float64(range_end))


def entry_of(buffers, rate, stream_id, buffer_samples, first_position=0, range_start=0.0, range_end=0.0):
    """(entry bytes, K, wrapped) of the buffers of one entry: a list of float32 [k, 2] arrays of (value, offset in buffer)"""
    start, end = sample_range(rate, range_start, range_end)
    offsets = [(first_position + j * buffer_samples + cast_offsets(p[:, 1])) & 0xFFFFFFFF for j, p in enumerate(buffers)]
    samples = [quantise(p[:, 0]) for p in buffers]
    offsets = np.concatenate(offsets) if buffers else np.zeros(0, dtype=np.int64)
    samples = np.concatenate(samples) if buffers else np.zeros(0, dtype=np.int64)
    keep = (offsets >= start) & (offsets <= end)
    offsets, samples = offsets[keep], samples[keep]
    d_offset = np.diff(np.concatenate([[start], offsets])) & 0xFFFFFFFF
    d_sample = np.diff(np.concatenate([[0], samples])) & 0xFFFF
    records = np.stack([d_offset & 0xFF, d_sample & 0xFF, d_sample >> 8], axis=1).astype(np.uint8)
    header = b"APCM" + np.array([2, 0, 0, offsets.size, stream_id, rate, 0], dtype="<u4").tobytes()
    return header + records.tobytes(), int(offsets.size), int((d_offset > 255).sum())


# ---------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------

def as_ptr(a):
    return a if isinstance(a, int) or a is None else a.ctypes.data


def raw_call(gpu, pairs, pitch, counts, n_buffers, capacity, out, out_pitch, capacity_bytes, info, location=LOC_HOST, rate=FS, group=1, buffer_samples=0,
             stream_id=0, position=0, range_start=0.0, range_end=0.0, reserved0=0, reserved=0, params_null=False):
    import nfclab_amd
    p = nfclab_amd.ApcmParams(rate, group, buffer_samples, stream_id, position, reserved0, range_start, range_end)
    p.reserved[3] = reserved
    return gpu.lib.nfcgpu_apcm_encode(gpu.ctx, as_ptr(pairs), pitch, as_ptr(counts), n_buffers, capacity, None if params_null else ctypes.byref(p),
                                      as_ptr(out), out_pitch, capacity_bytes, as_ptr(info), location)


def encode(gpu, buffers, group, buffer_samples, location=LOC_HOST, capacity=None, capacity_bytes=None, counts=None, expect=0, **params):
    """The call on rows whose pitch is larger than capacity_pairs, with pairs of NaN behind every count, the entries some bytes
    apart behind guard bytes: ([entry bytes as written], info). Every byte the call must leave alone is checked."""
    import nfclab_amd
    nb = len(buffers)
    n_entries = nb // group
    sizes = [p.shape[0] for p in buffers]
    capacity = max(sizes + [1]) if capacity is None else capacity
    row = 2 * capacity + 6
    pairs = np.full((max(nb, 1), row), np.nan, dtype=np.float32)
    for b, p in enumerate(buffers):
        pairs[b, :2 * min(sizes[b], capacity)] = p.reshape(-1)[:2 * capacity]
    counts = np.array(sizes if counts is None else counts, dtype=np.uint32)
    most = max([sum(sizes[e * group:(e + 1) * group]) for e in range(n_entries)] + [0])
    capacity_bytes = 32 + 3 * most if capacity_bytes is None else capacity_bytes
    pitch = (capacity_bytes + 3 & ~3) + 8
    out = np.full((max(n_entries, 1) + 1, pitch), GUARD, dtype=np.uint8)
    info = np.full((max(n_entries, 1) + 1) * 16, GUARD, dtype=np.uint8)
    if location == LOC_HOST:
        rc = raw_call(gpu, pairs, row * 4, counts, nb, capacity, out, pitch, capacity_bytes, info, LOC_HOST, group=group, buffer_samples=buffer_samples, **params)
    else:
        d_pairs, d_counts, d_out, d_info = DeviceArray(pairs), DeviceArray(counts if nb else np.zeros(1, dtype=np.uint32)), DeviceArray(out), DeviceArray(info)
        rc = raw_call(gpu, d_pairs.ptr, row * 4, d_counts.ptr, nb, capacity, d_out.ptr, pitch, capacity_bytes, d_info.ptr, LOC_DEVICE, group=group,
                      buffer_samples=buffer_samples, **params)
        out, info = d_out.read().copy(), d_info.read().copy()
    assert rc == expect, (rc, gpu.lib.nfcgpu_last_error(gpu.ctx).decode())
    if (info == GUARD).all():   # a call that was refused before anything ran
        assert rc == EINVAL and (out == GUARD).all()
        return [], None
    assert (info[n_entries * 16:] == GUARD).all()
    info = info[:n_entries * 16].view(nfclab_amd.APCM_INFO_DTYPE)
    entries = []
    for e in range(n_entries):
        assert info["bytes"][e] == 32 + 3 * info["records"][e] and info["reserved"][e] == 0
        written = 32 + 3 * min(int(info["records"][e]), (capacity_bytes - 32) // 3)
        assert (out[e, written:] == GUARD).all(), "entry %d: bytes behind the entry were written" % e
        entries.append(out[e, :written].tobytes())
    assert (out[n_entries:] == GUARD).all()
    return entries, info


def check(gpu, buffers, group, buffer_samples, location=LOC_HOST, rate=FS, stream_id=0, position=0, range_start=0.0, range_end=0.0):
    entries, info = encode(gpu, buffers, group, buffer_samples, location, rate=rate, stream_id=stream_id, position=position, range_start=range_start,
                           range_end=range_end)
    for e, got in enumerate(entries):
        want, kept, wrapped = entry_of(buffers[e * group:(e + 1) * group], rate, stream_id + e, buffer_samples, position, range_start, range_end)
        assert info["records"][e] == kept and info["wrapped"][e] == wrapped, (e, info[e], kept, wrapped)
        assert got == want, "entry %d differs at byte %d" % (e, next(i for i in range(max(len(got), len(want))) if got[i:i + 1] != want[i:i + 1]))
    return entries, info


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

_points = {}


def signal(kind, n, n_buffers):
    """float32 [n_buffers, n] magnitudes"""
    if kind == "flat":      # a point every 255 samples and no other
        return np.full((n_buffers, n), 0.5, dtype=np.float32)
    if kind == "dense":     # every sample departs from the mean around it: every sample is a point
        x = np.where(np.arange(n_buffers * n) % 2 == 0, 0.2, 0.8).astype(np.float32)
        x += (np.arange(n_buffers * n) % 7).astype(np.float32) * np.float32(0.01)
        return x.reshape(n_buffers, n)
    x, edge = TS.capture()  # the capture around its first modulation
    return np.ascontiguousarray(x[edge - 300:edge - 300 + n_buffers * n].reshape(n_buffers, n))


def points(gpu, kind, n, n_buffers):
    """the resampler's control points of signal(): computed once, shared, never changed"""
    key = (kind, n, n_buffers)
    if key not in _points:
        got = [p.copy() for p in gpu.resample_radio(signal(kind, n, n_buffers))]
        for p in got:
            p.setflags(write=False)
        _points[key] = got
    return _points[key]


def on_a_point(rate, offset):
    """seconds t with (uint32)(rate * t) == offset"""
    t = np.float64(offset) / np.float64(rate)
    while int(np.float64(rate) * t) < offset:
        t = np.nextafter(t, np.inf)
    assert int(np.float64(rate) * t) == offset
    return float(t)


def hand(rows):
    return [np.array(r, dtype=np.float32).reshape(-1, 2) for r in rows]


# ---------------------------------------------------------------------------------------------------------------------
# 1. resampler output
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "dense", "capture"])
@pytest.mark.parametrize("n", SIZES)
def test_resampler_output_in_groups_and_entries(gpu, kind, n):
    """buffers of n samples, 1 and 3 to an entry, 1 and 5 entries; nothing wraps"""
    pts = points(gpu, kind, n, 15)
    if kind == "dense":
        assert all(p.shape[0] >= n for p in pts)
    if kind == "flat":
        assert all(p.shape[0] <= n // 255 + 52 for p in pts)   # (the window's run-in and run-out, then a point every 255)
    for group, n_entries, location in ((1, 1, LOC_HOST), (3, 1, LOC_DEVICE), (1, 5, LOC_DEVICE), (3, 5, LOC_HOST)):
        _, info = check(gpu, pts[:group * n_entries], group, n, location, stream_id=7)
        assert not info["wrapped"].any()


def test_a_first_record_at_every_byte_of_a_dword(gpu):
    """kept counts 1, 1, 1, 1, then 2, 3 and chunks of a dense buffer: a buffer's records start at the bytes 0, 3, 2, 1 of a dword"""
    dense = points(gpu, "dense", 4099, 15)
    assert dense[0].shape[0] > 4 * CHUNK
    for lead in range(4):
        buffers = [dense[0][:1]] * lead + [dense[1], dense[2][:2], dense[3][:3], dense[4][:CHUNK + 1], dense[5][:5]]
        buffers = [np.column_stack([b[:, 0], b[:, 1]]).astype(np.float32) for b in buffers]
        for location in (LOC_HOST, LOC_DEVICE):
            check(gpu, buffers, len(buffers), 4099, location)


def test_ranges(gpu):
    """entirely before and behind the data; starting and ending exactly on a point; cutting inside a buffer; 0, 0"""
    n, group = 4099, 3
    pts = points(gpu, "capture", n, 15)[:2 * group]
    flat = np.concatenate([j * n + cast_offsets(p[:, 1]) for j, p in enumerate(pts[:group])])
    assert flat.size > 40 and (np.diff(flat) >= 0).all()
    first, last = int(flat[5]), int(flat[-7])
    assert first > 0 and last > n
    for location in (LOC_HOST, LOC_DEVICE):
        # both ends are inside: the points 5 ... size - 7
        _, info = check(gpu, pts, group, n, location, range_start=on_a_point(FS, first), range_end=on_a_point(FS, last))
        assert info["records"][0] == np.count_nonzero((flat >= first) & (flat <= last)) and not info["wrapped"].any()
        # one sample further in on either side: those two points are gone
        _, tighter = check(gpu, pts, group, n, location, range_start=on_a_point(FS, first + 1), range_end=on_a_point(FS, last - 1))
        assert tighter["records"][0] == info["records"][0] - np.count_nonzero((flat == first) | (flat == last))
        # a single sample
        check(gpu, pts, group, n, location, range_start=on_a_point(FS, first), range_end=on_a_point(FS, first))
        # before the data and behind it: bare headers
        for position, a, b in ((100000, 0.0001, 0.0002), (0, 0.1, 0.2)):
            entries, info = check(gpu, pts, group, n, location, position=position, range_start=a, range_end=b)
            assert not info["records"].any() and all(len(e) == 32 for e in entries)
        # from the start to a point, and everything
        check(gpu, pts, group, n, location, range_start=0.0, range_end=on_a_point(FS, last))
        _, info = check(gpu, pts, group, n, location)
        assert info["records"][0] == flat.size
    # a position that is not 0: the range counts stream positions
    check(gpu, pts, group, n, position=123456, range_start=on_a_point(FS, 123456 + first), range_end=on_a_point(FS, 123456 + last))
    # a range that starts before the data wraps its first delta, as the reference's does
    _, info = check(gpu, pts, group, n, position=1000, range_start=on_a_point(FS, 10), range_end=1.0)
    assert (info["wrapped"] == 1).all()


def test_other_rates_ids_and_positions(gpu):
    pts = points(gpu, "capture", 257, 15)
    check(gpu, pts, 3, 257, rate=2000000, stream_id=0xFFFFFFFB, position=0xFFFFFFFF - 3 * 257)
    check(gpu, pts, 5, 300, LOC_DEVICE, rate=1, stream_id=41, position=17)


def test_the_reference_writes_the_same_entry(gpu):
    """tests/golden/apcm: the reference's SignalResamplingTask and TraceStorageTask on 32 768 samples of the capture from sample
    8192 in buffers of 4096 - everything, and a range that starts inside a buffer and ends exactly on a control point"""
    import tarfile
    import trz
    x = T.load_fixture(TS.CAPTURE)[8192:8192 + 32768]
    pts = gpu.resample_radio(x.reshape(8, 4096))
    flat = np.concatenate([j * 4096 + cast_offsets(p[:, 1]) for j, p in enumerate(pts)])
    values = np.concatenate([quantise(p[:, 0]) for p in pts])
    assert 20618 in flat and int(np.float64(FS) * np.float64(0.0020618)) == 20618 and int(np.float64(FS) * np.float64(0.0005)) == 5000
    for name, a, b, inside in (("reference_all.trz", 0.0, 1.0, flat >= 0), ("reference_cut.trz", 0.0005, 0.0020618, (flat >= 5000) & (flat <= 20618))):
        path = os.path.join(T.GOLDEN, "apcm", name)
        with tarfile.open(path, "r:gz") as tar:
            assert tar.getnames() == ["frame.json", "radio-0.apcm"]
            theirs = tar.extractfile("radio-0.apcm").read()
        for location in (LOC_HOST, LOC_DEVICE):
            entries, info = check(gpu, pts, 8, 4096, location, range_start=a, range_end=b)
            assert entries[0] == theirs and info["records"][0] == inside.sum() and info["wrapped"][0] == 0
        header, got_values, got_offsets = trz.read_trz_signal(path)[0]
        assert header["samples"] == inside.sum() and header["sample_rate"] == FS and header["info"][1] == 0
        assert (got_values == values[inside]).all() and (got_offsets == flat[inside] - int(np.float64(FS) * np.float64(a))).all()
    # 0, 0 - every point - is what the reference writes for a range that holds every point
    assert check(gpu, pts, 8, 4096)[0][0] == theirs_all(os.path.join(T.GOLDEN, "apcm", "reference_all.trz"))


def theirs_all(path):
    import tarfile
    with tarfile.open(path, "r:gz") as tar:
        return tar.extractfile("radio-0.apcm").read()


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows made by hand
# ---------------------------------------------------------------------------------------------------------------------

def hand_rows():
    inf, nan = np.inf, np.nan
    return hand([
        [(0.5, 0), (0.5, 0), (0.25, 3), (0.25, 3), (0.75, 3)],                                    # duplicate offsets
        [],
        [],
        [(1.0, 0), (1.5, 1), (-0.5, 2), (-1.0, 3), (-3.0, 4), (inf, 5), (-inf, 6), (nan, 7)],     # 1.0, above 1, negative, infinities, a NaN
        [],
        [(-1.0, 0), (1.0, 1), (-1.0, 2), (1.0, 3), (32767 / 32768.0, 4), (-32767.5 / 32768.0, 5)],  # -32768 / 32767 in turn: the delta wraps
        [(0.1, 0), (0.2, 255), (0.3, 511), (0.4, 600), (0.5, 1000)],                             # gaps of 255, 256 and 400
        [(0.1, -1.0), (0.2, nan), (0.3, 0.9), (0.4, 1.999), (0.5, 5e9), (0.6, inf), (0.7, -inf)],  # offsets the cast has to bend
        [(0.3, 900), (0.2, 10), (0.1, 500)],                                                      # offsets that go back
    ])


@pytest.mark.parametrize("location", [LOC_HOST, LOC_DEVICE])
def test_rows_made_by_hand(gpu, location):
    rows = hand_rows()
    _, info = check(gpu, rows, 9, 1024, location)
    assert info["wrapped"][0] >= 2
    check(gpu, rows, 3, 1024, location, stream_id=3)
    check(gpu, rows, 1, 1024, location, position=77)
    # the kept set is a predicate of the point, whatever the order of the offsets
    check(gpu, rows, 9, 1024, location, range_start=on_a_point(FS, 3), range_end=on_a_point(FS, 6 * 1024 + 511))
    # an entry of empty buffers alone
    entries, info = check(gpu, hand([[], [], []]), 3, 64, location)
    assert entries[0] == b"APCM" + np.array([2, 0, 0, 0, 0, FS, 0], dtype="<u4").tobytes() and info["bytes"][0] == 32


def test_the_same_call_twice_gives_the_same_bytes(gpu):
    pts = points(gpu, "capture", 4099, 15)
    for location in (LOC_HOST, LOC_DEVICE):
        assert encode(gpu, pts, 3, 4099, location)[0] == encode(gpu, pts, 3, 4099, location)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. capacity, counts
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("location", [LOC_HOST, LOC_DEVICE])
def test_an_entry_one_record_short(gpu, location):
    """the header and the records that fit whole; info says what is needed; the other entries are complete"""
    pts = points(gpu, "dense", 4099, 15)[:6]
    full, complete = encode(gpu, pts, 3, 4099, location)
    need = int(complete["bytes"].max())
    for capacity_bytes in (need - 3, need - 1, need - 3 * CHUNK - 2, 32, 33):
        entries, info = encode(gpu, pts, 3, 4099, location, capacity_bytes=capacity_bytes, expect=EOVERFLOW)
        assert info.tobytes() == complete.tobytes()
        room = (capacity_bytes - 32) // 3
        for e, got in enumerate(entries):
            there = min(room, int(complete["records"][e]))
            assert len(got) == 32 + 3 * there
            assert got[:16] == full[e][:16] and got[20:32] == full[e][20:32] and got[32:] == full[e][32:32 + 3 * there]
            assert np.frombuffer(got, dtype="<u4", count=1, offset=16)[0] == there


def test_a_count_above_the_capacity(gpu):
    pts = points(gpu, "capture", 4099, 15)[:6]
    capacity = max(p.shape[0] for p in pts)
    counts = [p.shape[0] for p in pts]
    counts[4] = capacity + 1
    # host memory: refused before anything runs
    entries, _ = encode(gpu, pts, 3, 4099, LOC_HOST, counts=counts, expect=EINVAL)
    assert entries == [] and "buffer 4" in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()
    # device memory: capacity_pairs of that buffer are taken (what lies there: NaN pairs behind the buffer's own), the rest is complete
    entries, info = encode(gpu, pts, 3, 4099, LOC_DEVICE, counts=counts, capacity_bytes=32 + 3 * 3 * capacity, expect=EINVAL)
    assert "device memory" in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()
    padded = list(pts)
    padded[4] = np.concatenate([pts[4], np.full((capacity - pts[4].shape[0], 2), np.nan, dtype=np.float32)])
    for e in range(2):
        want, kept, _ = entry_of(padded[3 * e:3 * e + 3], FS, e, 4099)
        assert entries[e] == want and info["records"][e] == kept


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------

def refusals():
    """(what, changes to the call, the word nfcgpu_last_error must carry)"""
    return [("params NULL", {"params_null": True}, "params is NULL"),
            ("reserved0", {"reserved0": 1}, "reserved"),
            ("reserved", {"reserved": 1}, "reserved"),
            ("unknown location", {"location": 2}, "location"),
            ("rate 0", {"rate": 0}, "sample rate"),
            ("no buffers to an entry", {"group": 0}, "buffers_per_entry"),
            ("buffers that do not fill the entries", {"group": 4}, "buffers_per_entry"),
            ("a buffer that ends at 2^32", {"position": 0xFFFFFFFF - 2 * 64 + 1}, "position"),
            ("a stream id beyond 2^32 - 1", {"stream_id": 0xFFFFFFFE}, "stream id"),
            ("a negative range", {"range_start": -0.5, "range_end": 1.0}, "range"),
            ("a range that ends before it starts", {"range_start": 2.0, "range_end": 1.0}, "range"),
            ("a range that is no number", {"range_start": 0.0, "range_end": float("nan")}, "range"),
            ("a range beyond 2^32 samples", {"range_start": 0.0, "range_end": 430.0}, "range"),
            ("pairs on an odd float", {"pairs_shift": 4}, "pairs"),
            ("a pairs pitch of an odd float", {"pitch": 20 * 8 + 4}, "pairs"),
            ("a pairs pitch smaller than the capacity", {"pitch": 15 * 8}, "pairs"),
            ("counts on an odd byte", {"counts_shift": 2}, "counts"),
            ("info on an odd byte", {"info_shift": 1}, "info"),
            ("out on an odd byte", {"out_shift": 2}, "out"),
            ("an out pitch that is no multiple of 4", {"out_pitch": 1002}, "out"),
            ("a capacity below a header", {"capacity_bytes": 31}, "capacity_bytes"),
            ("a capacity above the pitch", {"capacity_bytes": 1004}, "capacity_bytes"),
            ("entries of 4 GiB", {"capacity": 0x20000000, "pitch": 0x20000000 * 8, "group": 3}, "4 GiB"),
            ("pairs NULL", {"pairs_null": True}, "NULL"),
            ("counts NULL", {"counts_null": True}, "NULL"),
            ("out NULL", {"out_null": True}, "NULL"),
            ("info NULL", {"info_null": True}, "NULL")]


@pytest.mark.parametrize("what,call,word", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_return_einval_and_write_nothing(gpu, what, call, word):
    pairs = np.zeros((6, 2 * 20 + 2), dtype=np.float32)
    counts = np.full(7, 16, dtype=np.uint32)
    out = np.full(6 * 1000 + 8, GUARD, dtype=np.uint8)
    info = np.full(7 * 16, GUARD, dtype=np.uint8)
    rc = raw_call(gpu, None if call.get("pairs_null") else pairs.ctypes.data + call.get("pairs_shift", 0), call.get("pitch", 21 * 8),
                  None if call.get("counts_null") else counts.ctypes.data + call.get("counts_shift", 0), 6, call.get("capacity", 16),
                  None if call.get("out_null") else out.ctypes.data + call.get("out_shift", 0), call.get("out_pitch", 1000), call.get("capacity_bytes", 1000),
                  None if call.get("info_null") else info.ctypes.data + call.get("info_shift", 0), call.get("location", LOC_HOST), rate=call.get("rate", FS),
                  group=call.get("group", 2), buffer_samples=64, stream_id=call.get("stream_id", 0), position=call.get("position", 0),
                  range_start=call.get("range_start", 0.0), range_end=call.get("range_end", 0.0), reserved0=call.get("reserved0", 0),
                  reserved=call.get("reserved", 0), params_null=call.get("params_null", False))
    assert rc == EINVAL
    assert (out == GUARD).all() and (info == GUARD).all()
    assert word in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()


def test_the_bounds_themselves_are_accepted(gpu):
    """the last buffer may end at 2^32 - 1, the last id may be 2^32 - 1"""
    pts = points(gpu, "flat", 64, 15)[:6]
    check(gpu, pts, 2, 64, position=0xFFFFFFFF - 2 * 64, stream_id=0xFFFFFFFD)


def test_a_null_context_is_refused(gpu):
    pairs, counts, out, info = np.zeros(32, dtype=np.float32), np.zeros(1, dtype=np.uint32), np.zeros(128, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    none = type("none", (), {"lib": gpu.lib, "ctx": None})
    assert raw_call(none, pairs, 128, counts, 1, 16, out, 128, 128, info) == EINVAL


def test_no_buffers_is_success_and_writes_nothing(gpu):
    out, info = np.full(64, GUARD, dtype=np.uint8), np.full(16, GUARD, dtype=np.uint8)
    for location in (LOC_HOST, LOC_DEVICE):
        assert raw_call(gpu, None, 0, None, 0, 0, out, 64, 64, info, location) == 0
    assert (out == GUARD).all() and (info == GUARD).all()
    assert gpu.lib.nfcgpu_apcm_bound(0) == 32 and gpu.lib.nfcgpu_apcm_bound(1000) == 3032 and gpu.lib.nfcgpu_apcm_bound(1 << 40) == 32 + 3 * (1 << 40)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the binding
# ---------------------------------------------------------------------------------------------------------------------

def test_the_binding(gpu, tmp_path):
    import nfclab_amd
    import trz
    n = 4099
    pts = points(gpu, "capture", n, 15)
    entries, info = gpu.apcm_encode(pts[:6], FS, buffers_per_entry=3, buffer_samples=n, first_stream_id=4, with_info=True)
    for e in range(2):
        want, kept, _ = entry_of(pts[3 * e:3 * e + 3], FS, 4 + e, n)
        assert entries[e] == want and info["records"][e] == kept
    assert gpu.apcm_encode([], FS) == []

    # read back: the quantised control points
    header, values, offsets = trz.parse_apcm(entries[1])
    assert header["stream_id"] == 5 and header["sample_rate"] == FS and header["samples"] == info["records"][1]
    assert (values == np.concatenate([quantise(p[:, 0]) for p in pts[3:6]])).all()
    assert (offsets == np.concatenate([j * n + cast_offsets(p[:, 1]) for j, p in enumerate(pts[3:6])])).all()

    # device pointers
    cap = max(p.shape[0] for p in pts[:6])
    rows = np.zeros((6, 2 * cap), dtype=np.float32)
    for b, p in enumerate(pts[:6]):
        rows[b, :2 * p.shape[0]] = p.reshape(-1)
    counts = np.array([p.shape[0] for p in pts[:6]], dtype=np.uint32)
    pitch = int(gpu.lib.nfcgpu_apcm_bound(3 * cap)) + 3 & ~3
    d_rows, d_counts, d_out, d_info = DeviceArray(rows), DeviceArray(counts), DeviceArray(np.zeros((2, pitch), dtype=np.uint8)), DeviceArray(np.zeros(2, dtype=nfclab_amd.APCM_INFO_DTYPE))
    gpu.apcm_encode_device(d_rows.ptr, cap * 8, d_counts.ptr, 6, cap, FS, d_out.ptr, pitch, pitch, d_info.ptr, buffers_per_entry=3, buffer_samples=n, first_stream_id=4)
    assert d_info.read().tobytes() == info.tobytes()
    assert all(d_out.read()[e, :len(entries[e])].tobytes() == entries[e] for e in range(2))

    # a stream's capture and its frames as one trace
    x, edge = TS.capture()
    x = x[edge - 300:edge - 300 + 3 * n + 100]
    frames = [(1, 1, 0, 0, 106000, 400, 900, FS, b"\x26"), (1, 2, 0, 0, 106000, 5000, 7000, FS, b"\x04\x00")]
    path = str(tmp_path / "capture.trz")
    written, stored = gpu.trace_write_capture(path, x, FS, frames, buffer_samples=n, stream_id=9)
    pieces = gpu.resample_radio(x[:3 * n].reshape(3, n)) + gpu.resample_radio(x[3 * n:].reshape(1, -1))
    want, kept, _ = entry_of(pieces, FS, 9, n)
    header, values, offsets = trz.read_trz_signal(path)[9]
    assert written == 2 and stored == kept == header["samples"]
    assert (values == np.concatenate([quantise(p[:, 0]) for p in pieces])).all()
    assert (offsets == np.concatenate([j * n + cast_offsets(p[:, 1]) for j, p in enumerate(pieces)])).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the CPU twin of the emulated library and the device kernels
# ---------------------------------------------------------------------------------------------------------------------

def twin_cases(g):
    """(buffers, keyword arguments of NfcGpu.apcm_encode)"""
    capture, dense, flat = points(g, "capture", 4099, 15), points(g, "dense", 4099, 15), points(g, "flat", 257, 15)
    return [(capture, dict(buffers_per_entry=3, buffer_samples=4099)),
            (dense, dict(buffers_per_entry=5, buffer_samples=4099, first_position=1000, range_start=0.00015, range_end=0.0019)),
            (flat, dict(buffers_per_entry=1, buffer_samples=257, first_stream_id=3)),
            (hand_rows(), dict(buffers_per_entry=9, buffer_samples=1024)),
            ([dense[0][:1], dense[1][:2], dense[2][:3], dense[3], dense[4][:CHUNK + 1]], dict(buffers_per_entry=5, buffer_samples=4099))]


def dump_outputs(path):
    """Child process (NFCGPU_LIB names the library): the entries and the results of twin_cases(), in order, to one file."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    pieces = []
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for buffers, how in twin_cases(g):
            entries, info = g.apcm_encode(buffers, FS, with_info=True, **how)
            pieces += [np.frombuffer(e, dtype=np.uint8) for e in entries] + [info.view(np.uint8).reshape(-1)]
    np.save(path, np.concatenate(pieces))


def test_twin_equals_device(gpu, tmp_path):
    """every entry and every result is the same bytes from the emulated library's twins and from the device kernels"""
    if on_emulated_library():
        pytest.skip("NFCGPU_LIB is the emulated library: there is no device to compare with")
    if not os.path.exists(EMU):
        pytest.skip("tests/hostsim/libnfcgpu_emulated.so is not built")
    import nfclab_amd
    outputs = {}
    for name, lib, extra in (("device", nfclab_amd.LIB_PATH, {}), ("twin", EMU, {"NFCGPU_NO_TORCH": "1"})):
        path = str(tmp_path / (name + ".npy"))
        env = dict(os.environ, NFCGPU_LIB=lib, PYTHONPATH=os.path.join(T.ROOT, "tests"), **extra)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], cwd=T.ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-3000:]
        outputs[name] = np.load(path)
    assert outputs["device"].size > 0 and outputs["device"].tobytes() == outputs["twin"].tobytes()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump_outputs(sys.argv[2])
    else:
        sys.exit("usage: test_apcm.py --dump OUT.npy")
