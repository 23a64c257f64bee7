"""nfcgpu_trace_write_signal (host only): frame.json and the radio-<id>.apcm entries in one .trz, and trz.py's reader and writer of
the same. No device: the trace writer is host code, the emulated test build of the library exports it too. The entries are made
by the numpy yardstick of tests/test_apcm.py."""
import ctypes
import json
import os
import subprocess
import tarfile

import numpy as np
import pytest

import nfc_testlib as T
import trz
from test_apcm import cast_offsets, entry_of, quantise

EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
TRACE_REF = os.path.join(T.ROOT, "oracle", "_ref", "trace-ref")
GOLDEN = os.path.join(T.ROOT, "tests", "golden", "apcm")
FS = 10000000
EINVAL = -1


@pytest.fixture(scope="module")
def abi(built):
    if not os.path.exists(EMU):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    lib = ctypes.CDLL(EMU)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.nfcgpu_trace_write_frames.argtypes = [ctypes.c_char_p, vp, u32, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.POINTER(u32)]
    lib.nfcgpu_trace_write_signal.argtypes = lib.nfcgpu_trace_write_frames.argtypes + [ctypes.POINTER(vp), ctypes.POINTER(u64), u32]
    return lib


def c_frames(frames):
    arr = (T.Frame * max(len(frames), 1))()
    for a, (tech, ftype, flags, phase, rate, start, end, fs, payload) in zip(arr, frames):
        a.tech_type, a.frame_type, a.frame_flags, a.frame_phase, a.frame_rate = tech, ftype, flags, phase, rate
        a.sample_start, a.sample_end, a.sample_rate, a.length = start, end, fs, len(payload)
        for i, b in enumerate(payload):
            a.data[i] = b
    return arr


def write_signal(abi, path, frames, entries, sizes=None, stream_time=1700000000, range_start=0.0, range_end=0.0):
    held = [np.frombuffer(e, dtype=np.uint8) for e in entries]
    pointers = (ctypes.c_void_p * max(len(held), 1))(*[h.ctypes.data for h in held])
    lengths = (ctypes.c_uint64 * max(len(held), 1))(*(sizes or [h.size for h in held]))
    written = ctypes.c_uint32(0xFFFFFFFF)
    rc = abi.nfcgpu_trace_write_signal(str(path).encode(), ctypes.cast(c_frames(frames), ctypes.c_void_p), len(frames), stream_time, range_start, range_end,
                                       ctypes.byref(written), pointers, lengths, len(held))
    return rc, written.value


def buffers(seed, n_buffers, per_buffer):
    """control points of n_buffers buffers of 4096 samples: float32 [k, 2]; per_buffer points at random and one every 200 samples
    and at the buffer's end, as the resampler leaves none further than 255 apart (a larger step does not fit a record's byte)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_buffers):
        offsets = np.union1d(rng.choice(4096, size=per_buffer, replace=False), np.append(np.arange(0, 4096, 200), 4095)).astype(np.float32)
        out.append(np.column_stack([rng.uniform(0.0, 1.0, offsets.size).astype(np.float32), offsets]))
    return out


@pytest.fixture(scope="module")
def signals():
    """{id: (buffers, entry)}: ids in no order, one entry of more than 65535 bytes (several stored blocks), one bare header"""
    made = {}
    for sid, (n_buffers, per_buffer) in ((7, (4, 300)), (0, (8, 4000)), (0xFFFFFFFF, (1, 1)), (3, (0, 0))):
        b = buffers(sid & 0xFF, n_buffers, per_buffer)
        made[sid] = (b, entry_of(b, FS, sid, 4096)[0])
    assert len(made[0][1]) > 65535 and len(made[3][1]) == 32
    return made


def test_without_entries_the_file_is_that_of_the_frames_call(abi, tmp_path):
    frames = T.load_golden("test_NFC-A_106kbps_001")
    for name, (a, b) in (("all", (0.0, 0.0)), ("range", (frames[3][5] / 1e7 - 1e-4, frames[9][6] / 1e7 + 1e-4))):
        one, two = tmp_path / (name + "_frames.trz"), tmp_path / (name + "_signal.trz")
        written = ctypes.c_uint32()
        assert abi.nfcgpu_trace_write_frames(str(one).encode(), ctypes.cast(c_frames(frames), ctypes.c_void_p), len(frames), 1700000000, a, b, ctypes.byref(written)) == 0
        assert write_signal(abi, two, frames, [], range_start=a, range_end=b) == (0, written.value)
        assert one.read_bytes() == two.read_bytes()
    # ... and no frames at all
    assert write_signal(abi, tmp_path / "empty.trz", [], []) == (0, 0)
    with tarfile.open(tmp_path / "empty.trz", "r:gz") as tar:
        assert tar.getnames() == ["frame.json"] and json.load(tar.extractfile("frame.json")) == {"frames": []}


def test_the_frames_file_is_what_it_was(abi, tmp_path):
    """the single-entry archive, byte for byte, as tests/golden/apcm/frames_only.trz holds it from before the writer took more
    than one entry"""
    frames = T.load_golden("test_NFC-A_106kbps_001")
    path = tmp_path / "frames.trz"
    assert abi.nfcgpu_trace_write_frames(str(path).encode(), ctypes.cast(c_frames(frames), ctypes.c_void_p), len(frames), 1700000000, 0.0, 0.0, None) == 0
    with open(os.path.join(GOLDEN, "frames_only.trz"), "rb") as f:
        assert path.read_bytes() == f.read()


def test_the_archive_lists_frame_json_and_the_entries_in_the_order_given(abi, signals, tmp_path):
    frames = T.load_golden("test_POLL_ABF_001")
    order = [7, 0, 0xFFFFFFFF, 3]
    path = tmp_path / "signal.trz"
    assert write_signal(abi, path, frames, [signals[s][1] for s in order]) == (0, len(frames))
    with tarfile.open(path, "r:gz") as tar:
        members = tar.getmembers()
        assert [m.name for m in members] == ["frame.json"] + ["radio-%d.apcm" % s for s in order]
        assert [m.size for m in members[1:]] == [len(signals[s][1]) for s in order]
        assert all(m.isfile() and m.mode == 0o664 for m in members)
        assert [tar.extractfile(m).read() for m in members[1:]] == [signals[s][1] for s in order]
    # frame.json is that of the frames-only file
    only = tmp_path / "frames.trz"
    assert abi.nfcgpu_trace_write_frames(str(only).encode(), ctypes.cast(c_frames(frames), ctypes.c_void_p), len(frames), 1700000000, 0.0, 0.0, None) == 0
    with tarfile.open(path, "r:gz") as a, tarfile.open(only, "r:gz") as b:
        assert a.extractfile("frame.json").read() == b.extractfile("frame.json").read()


def check_signals(read, signals, ids):
    assert sorted(read) == sorted(ids)
    for sid in ids:
        header, values, offsets = read[sid]
        points = signals[sid][0]
        assert header["version"] == 2 and header["stream_id"] == sid and header["sample_rate"] == FS and header["info"][0] == header["info"][1] == 0
        assert values.dtype == np.int16 and offsets.dtype == np.uint32 and header["samples"] == values.size == offsets.size
        assert (values == np.concatenate([quantise(p[:, 0]) for p in points] + [np.zeros(0, dtype=np.int64)])).all()
        assert (offsets == np.concatenate([j * 4096 + cast_offsets(p[:, 1]) for j, p in enumerate(points)] + [np.zeros(0, dtype=np.int64)])).all()


def test_round_trip_through_read_trz_signal(abi, signals, tmp_path):
    """the stored archive of the C ABI and the deflated one of trz.write_trz"""
    frames = T.load_golden("test_POLL_ABF_001")
    ids = [0, 3, 7, 0xFFFFFFFF]
    stored, deflated, plain = tmp_path / "stored.trz", tmp_path / "deflated.trz", tmp_path / "plain.trz"
    assert write_signal(abi, stored, frames, [signals[s][1] for s in ids])[0] == 0
    trz.write_trz(str(deflated), frames, 1700000000, signals=[signals[s][1] for s in ids])
    assert deflated.stat().st_size < stored.stat().st_size
    for path in (stored, deflated):
        check_signals(trz.read_trz_signal(str(path)), signals, ids)
    # without the argument write_trz writes what it wrote before: frame.json and nothing else
    trz.write_trz(str(plain), frames, 1700000000)
    with tarfile.open(plain, "r:gz") as tar:
        assert tar.getnames() == ["frame.json"]
    assert trz.read_trz_signal(str(plain)) == {}
    with tarfile.open(plain, "r:gz") as a, tarfile.open(deflated, "r:gz") as b:
        assert a.extractfile("frame.json").read() == b.extractfile("frame.json").read()


def test_a_range_shifts_the_offsets_to_its_start():
    """what the reader gives for an entry that was written with a range: positions counted from the range's first sample"""
    points = buffers(5, 3, 200)
    start, end = 5000, 9000
    entry, kept, _ = entry_of(points, FS, 1, 4096, range_start=start / FS, range_end=end / FS)
    _, values, offsets = trz.parse_apcm(entry)
    flat = np.concatenate([j * 4096 + cast_offsets(p[:, 1]) for j, p in enumerate(points)])
    inside = (flat >= start) & (flat <= end)
    assert kept == inside.sum() > 0 and (offsets == flat[inside] - start).all()
    assert (values == np.concatenate([quantise(p[:, 0]) for p in points])[inside]).all()


@pytest.mark.skipif(not os.path.exists(TRACE_REF), reason="trace-ref not built (needs the reference tree and zlib at build time)")
def test_the_reference_trace_storage_task_reads_the_file(abi, signals, tmp_path):
    """the reference's own reader accepts the entries (its size and magic checks, TraceStorageTask.cpp:816-827, reject anything
    else and fail the read) and publishes the same frames as for the frames-only file"""
    frames = T.load_golden("test_POLL_ABF_001")
    with_signal, without = tmp_path / "signal.trz", tmp_path / "frames.trz"
    assert write_signal(abi, with_signal, frames, [signals[s][1] for s in (7, 0, 3)])[0] == 0
    assert write_signal(abi, without, frames, [])[0] == 0
    runs = [subprocess.run([TRACE_REF, "read", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300) for p in (with_signal, without)]
    assert runs[0].returncode == 0, runs[0].stderr[-2000:]
    assert runs[1].returncode == 0, runs[1].stderr[-2000:]
    assert runs[0].stdout == runs[1].stdout and len(runs[0].stdout.splitlines()) == len(frames)


def test_malformed_entries_are_refused(abi, signals, tmp_path):
    good = signals[7][1]
    words = lambda e, at, v: e[:at] + np.array([v], dtype="<u4").tobytes() + e[at + 4:]
    path = tmp_path / "bad.trz"
    cases = {"another magic": ([b"APCN" + good[4:]], None),
             "version 1": ([words(good, 4, 1)], None),
             "version 3": ([words(good, 4, 3)], None),
             "more bytes than samples": ([good + b"\0\0\0"], None),
             "fewer bytes than samples": ([good[:-3]], None),
             "a size that is no whole record": ([good], [len(good) - 1]),
             "shorter than a header": ([good], [31]),
             "two entries with one id": ([good, signals[0][1], words(signals[3][1], 20, 7)], None),
             # (its header says 0x60000000 samples and its size agrees: refused before a record is read)
             "an archive of 4 GiB": ([words(signals[3][1], 16, 0x60000000)], [32 + 3 * 0x60000000])}
    for what, (entries, sizes) in cases.items():
        assert write_signal(abi, path, [], entries, sizes)[0] == EINVAL, what
        assert not path.exists(), what
    # NULL arguments
    none = ctypes.POINTER(ctypes.c_void_p)()
    sizes = (ctypes.c_uint64 * 1)(32)
    assert abi.nfcgpu_trace_write_signal(str(path).encode(), None, 0, 0, 0.0, 0.0, None, none, sizes, 1) == EINVAL
    assert abi.nfcgpu_trace_write_signal(str(path).encode(), None, 0, 0, 0.0, 0.0, None, (ctypes.c_void_p * 1)(None), sizes, 1) == EINVAL
    assert abi.nfcgpu_trace_write_signal(None, None, 0, 0, 0.0, 0.0, None, none, None, 0) == EINVAL
    assert not path.exists()
    for bad in (b"APCN" + good[4:], good[:-3], good[:20]):
        with pytest.raises(ValueError):
            trz.parse_apcm(bad)
