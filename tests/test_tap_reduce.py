"""nfcgpu_signal_tap_reduce (the tap's channels over sample ranges: min, max, where they lie, mean, count of values that are no
NaN) through the C ABI, and frame_ranges of the binding.

Yardstick: the planes of the scalar walk of tests/test_signal_tap.py (tests/tap_walk_check.cpp, compiled as that file compiles
it), reduced here with numpy under the rules of include/nfcgpu.h. min, max, argmin, argmax, valid and the reserved words are
compared for equality, floats by their bits. mean is held against the exactly summed (math.fsum) float64 mean m of the same
values with the tolerance

    2^-24 |m| + (ceil(N / 64) + 7) 2^-53 mean(|v|) + 2^-149,     N the samples of the range:

one rounding to float plus the roundings of the double additions on the longest way a value takes (nfc_tap_reduce.hpp derives
that a value of a range of N samples meets at most ceil(N / 64) + 7 of them).

The same file runs on the CPU against the emulated library (tests/test_tap_reduce_emulated.py), whose twins of the kernels
compile the same nfc_tap_reduce.hpp; test_twin_equals_device ties the two together byte for byte."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import nfc_testlib as T
import test_signal_tap as TS
from test_signal_tap import (ALL, DEPTH, EINVAL, ENVELOPE, ERATE, F32, FILTERED, FS, I16, LOC_DEVICE, LOC_HOST, VALUE, DeviceArray, as_layout, magnitudes,
                             make_row, make_rows, on_emulated_library, selected)

pytestmark = pytest.mark.gpu

gpu = TS.gpu    # (module-scoped fixtures: one context, one compiled walk for this file)
walk = TS.walk

EMU = TS.EMU
SEG = 16384     # NfcTapReduceShape::kSegment
NAN_BITS, NONE = 0x7FC00000, 0xFFFFFFFF
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, SEG - 1, SEG, SEG + 1, 2 * SEG + 5)
GUARD = 0x5A


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------

def empty_record():
    import nfclab_amd
    r = np.zeros(1, dtype=nfclab_amd.TAP_STAT_DTYPE)
    r.view(np.uint32)[:3] = NAN_BITS
    r["argmin"] = r["argmax"] = NONE
    return r


def reduce_plane(p, first, count):
    """(record, m, mean(|v|)) of samples first ... first + count - 1 of the plane p by the rules of the header; m the exact mean"""
    rec = empty_record()
    v = p[first:first + count]
    ok = ~np.isnan(v)
    if not ok.any():
        return rec, None, None
    at, vals = np.nonzero(ok)[0], v[ok]
    lo, hi = int(np.argmin(vals)), int(np.argmax(vals))  # (the first of equal ones: -0.0 and 0.0 are equal)
    rec["min"], rec["argmin"] = vals[lo], first + at[lo]
    rec["max"], rec["argmax"] = vals[hi], first + at[hi]
    rec["valid"] = vals.size
    exact = [float(x) for x in vals]
    return rec, math.fsum(exact) / vals.size, math.fsum(abs(x) for x in exact) / vals.size


def ranges_of_bins(nb, n, bin_samples):
    bins = -(-n // bin_samples)
    return [(b, k * bin_samples, min(bin_samples, n - k * bin_samples)) for b in range(nb) for k in range(bins)]


def compare(got, planes_of, ranges, mask):
    """got: TAP_STAT_DTYPE [n_ranges, K]; planes_of(buffer) -> float32 [6, n] of the yardstick"""
    bits = selected(mask)
    assert got.shape == (len(ranges), len(bits))
    for r, (b, first, count) in enumerate(ranges):
        for k, bit in enumerate(bits):
            want, m, mean_abs = reduce_plane(planes_of(b)[bit], first, count)
            g = got[r:r + 1, k]
            what = "range %d (buffer %d, first %d, count %d), %s: %s, want %s" % (r, b, first, count, TS.NAMES[bit], g, want)
            for field in ("min", "max", "valid", "argmin", "argmax", "reserved"):
                assert g[field].tobytes() == want[field].tobytes(), what
            if m is None:
                assert g["mean"].view(np.uint32)[0] == NAN_BITS, what
            else:
                tolerance = 2.0 ** -24 * abs(m) + (-(-count // 64) + 7) * 2.0 ** -53 * mean_abs + 2.0 ** -149
                assert abs(float(g["mean"][0]) - m) <= tolerance, what + " (exact mean %r, tolerance %r)" % (m, tolerance)


# ---------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------

def raw_call(gpu, x, in_pitch, n_buffers, n, stride, fmt, rate, mask, state_in, ranges, n_ranges, out, state_out, bin_samples=0, scratch=0,
             report=None, location=LOC_HOST, chunk=0, tap_reserved=0, reserved0=0, reserved=0, reduce_null=False, tap_null=False):
    import nfclab_amd
    as_ptr = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data
    p = nfclab_amd.TapParams(rate, mask, chunk, 0)
    p.reserved[2] = tap_reserved
    q = nfclab_amd.TapReduceParams(bin_samples, reserved0, scratch)
    q.reserved[1] = reserved
    return gpu.lib.nfcgpu_signal_tap_reduce(gpu.ctx, as_ptr(x), in_pitch, n_buffers, n, stride, fmt, None if tap_null else ctypes.byref(p),
                                            None if reduce_null else ctypes.byref(q), as_ptr(state_in), as_ptr(ranges), n_ranges, as_ptr(out),
                                            as_ptr(state_out), None if report is None else ctypes.byref(report), location)


def reduce_rows(gpu, rows, ranges=None, bin_samples=0, stride=1, fmt=F32, rate=FS, mask=ALL, scratch=0, states=None, location=LOC_HOST, expect=0):
    """The call on rows a few samples apart from dense, the records behind a guard record: (records [n_ranges, K], states, report)."""
    import nfclab_amd
    nb, n = rows.shape[0], rows.shape[1] // stride
    k = len(selected(mask))
    in_row = rows.shape[1] + 3 * stride
    x = np.zeros((nb, in_row), dtype=rows.dtype)
    x[:, :rows.shape[1]] = rows
    given = None if ranges is None else nfclab_amd.as_tap_ranges(ranges)
    n_ranges = len(ranges_of_bins(nb, n, bin_samples)) if ranges is None else given.shape[0]
    out = np.full((n_ranges * k + 1) * 32, GUARD, dtype=np.uint8)
    state_out = np.zeros(nb, dtype=nfclab_amd.TAP_STATE_DTYPE)
    report = nfclab_amd.TapReport()
    if location == LOC_HOST:
        rc = raw_call(gpu, x, in_row * x.itemsize, nb, n, stride, fmt, rate, mask, states, given, 0 if given is None else n_ranges, out, state_out,
                      bin_samples, scratch, report)
    else:
        dx, dout, dstate = DeviceArray(x), DeviceArray(out), DeviceArray(state_out)
        din = None if states is None else DeviceArray(states)
        dranges = None if given is None else DeviceArray(given if given.size else np.zeros(1, dtype=nfclab_amd.TAP_RANGE_DTYPE))
        rc = raw_call(gpu, dx.ptr, in_row * x.itemsize, nb, n, stride, fmt, rate, mask, None if din is None else din.ptr,
                      None if dranges is None else dranges.ptr, 0 if given is None else n_ranges, dout.ptr, dstate.ptr, bin_samples, scratch, report, LOC_DEVICE)
        out, state_out = dout.read().copy(), dstate.read().copy()
    assert rc == expect, gpu.lib.nfcgpu_last_error(gpu.ctx).decode()
    assert (out[n_ranges * k * 32:] == GUARD).all()
    return out[:n_ranges * k * 32].view(nfclab_amd.TAP_STAT_DTYPE).reshape(n_ranges, k), state_out, report


def check_rows(gpu, walk, rows, ranges=None, bin_samples=0, stride=1, fmt=F32, rate=FS, mask=ALL, scratch=0, states=None, location=LOC_HOST):
    nb, n = rows.shape[0], rows.shape[1] // stride
    m = magnitudes(rows, stride, fmt)
    got, state_out, report = reduce_rows(gpu, rows, ranges, bin_samples, stride, fmt, rate, mask, scratch, states, location)
    state_of = lambda b: None if states is None else states[b:b + 1]
    compare(got, lambda b: walk(m[b], rate, state_of(b))[0], ranges_of_bins(nb, n, bin_samples) if ranges is None else ranges, mask)
    for b in range(nb):
        assert TS.same_state(state_out[b:b + 1], walk(m[b], rate, state_of(b))[1]), b
    return got, report


def starts_and_lengths(n, counts=COUNTS):
    """every count at first 0, 1, 2, 3 and ending with the buffer's last sample"""
    return [(0, first, c) for c in counts for first in (0, 1, 2, 3, n - c) if first + c <= n]


def scattered(nb, n, per_buffer, seed):
    """overlapping ranges of any length, in no order"""
    rng = np.random.default_rng(seed)
    ranges = []
    for b in range(nb):
        for _ in range(per_buffer):
            first = int(rng.integers(0, n))
            ranges.append((b, first, int(rng.integers(0, n - first + 1))))
    return [ranges[i] for i in rng.permutation(len(ranges))]


# ---------------------------------------------------------------------------------------------------------------------
# 1. ranges
# ---------------------------------------------------------------------------------------------------------------------

def test_lengths_around_a_quad_a_wave_and_a_segment_at_any_start(gpu, walk):
    """one mono float buffer of two segments and five samples of the capture"""
    n = 2 * SEG + 5
    row = make_row("capture", n)
    assert row.size == n
    check_rows(gpu, walk, row[None], starts_and_lengths(n))


def test_overlapping_and_unordered_ranges(gpu, walk):
    n = 2 * SEG + 5
    ranges = scattered(1, n, 24, 7) + [(0, 100, 2000), (0, 100, 2000), (0, 0, n), (0, 1500, 1)]
    check_rows(gpu, walk, make_row("capture", n)[None], ranges, mask=ENVELOPE | DEPTH)


@pytest.mark.parametrize("n_buffers", [3, 70])
def test_buffers_with_a_pitch_larger_than_a_row(gpu, walk, n_buffers):
    rows = make_rows("capture", 5000, n_buffers)
    check_rows(gpu, walk, rows, scattered(n_buffers, 5000, 3, n_buffers))
    got, _ = check_rows(gpu, walk, rows, bin_samples=1024, mask=ENVELOPE)
    assert got.shape == (n_buffers * 5, 1)


@pytest.mark.parametrize("mask", [VALUE, DEPTH, ALL, FILTERED | DEPTH])
def test_only_the_selected_channels_are_reduced(gpu, walk, mask):
    rows = make_rows("capture", 5000, 2)
    check_rows(gpu, walk, rows, scattered(2, 5000, 6, 3) + [(1, 0, 5000)], mask=mask)


def test_int16_iq(gpu, walk):
    rows = as_layout(make_rows("capture", 5000, 3), 2, I16)
    check_rows(gpu, walk, rows, scattered(3, 5000, 5, 11), stride=2, fmt=I16)
    check_rows(gpu, walk, rows, bin_samples=700, stride=2, fmt=I16, mask=ENVELOPE | DEPTH)


def test_a_buffer_of_zeros_has_no_depth(gpu, walk):
    rows = np.zeros((1, 3000), dtype=np.float32)
    assert np.isnan(walk(rows[0])[0][5]).all()
    got, _ = check_rows(gpu, walk, rows, [(0, 0, 3000), (0, 17, 64), (0, 2999, 1)], mask=VALUE | DEPTH)
    assert got[:, 1].tobytes() == np.repeat(empty_record(), 3).tobytes()
    assert (got["valid"][:, 0] == [3000, 64, 1]).all() and (got["argmin"][:, 0] == [0, 17, 2999]).all()


def test_a_first_sample_of_zero(gpu, walk):
    row = make_row("capture", 5000).copy()
    row[0] = 0
    assert np.isnan(walk(row)[0][5][0])
    got, _ = check_rows(gpu, walk, row[None], [(0, 0, 1), (0, 0, 2), (0, 0, 5000), (0, 1, 4999)])
    assert got["valid"][0, 5] == 0 and got["valid"][2, 5] < 5000 and got["valid"][0, 0] == 1


@pytest.mark.parametrize("bin_samples", [16, 100, 4096, 5003, 5004])
def test_bins(gpu, walk, bin_samples):
    got, _ = check_rows(gpu, walk, make_rows("capture", 5003, 2), bin_samples=bin_samples, mask=ENVELOPE | DEPTH)
    assert got.shape[0] == 2 * -(-5003 // bin_samples)


def test_bins_longer_than_a_segment(gpu, walk):
    check_rows(gpu, walk, make_row("capture", 2 * SEG + 5)[None], bin_samples=SEG + 1, mask=FILTERED)


# ---------------------------------------------------------------------------------------------------------------------
# 2. slabs, locations, states
# ---------------------------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_scratch_bytes(gpu, walk):
    """70 buffers whose planes are 6 * 20 224 bytes each: one slab, three, one per buffer (a bound smaller than one buffer's planes)"""
    rows = make_rows("capture", 5000, 70)
    ranges = scattered(70, 5000, 2, 5)
    one, report = check_rows(gpu, walk, rows, ranges)
    for scratch in (30 * 6 * 20224, 1000):
        got, _, sliced = reduce_rows(gpu, rows, ranges, scratch=scratch)
        assert got.tobytes() == one.tobytes(), scratch
        assert sliced.chunks >= report.chunks
    binned, _ = check_rows(gpu, walk, rows, bin_samples=1000)
    assert reduce_rows(gpu, rows, bin_samples=1000, scratch=24 * 6 * 20224)[0].tobytes() == binned.tobytes()


def test_device_memory(gpu, walk):
    rows = make_rows("capture", 5000, 3)
    states = gpu.tap_state_init(3)
    states["clock"] = [41, 0xFFFFFFF0, 7]
    check_rows(gpu, walk, rows, scattered(3, 5000, 4, 9), location=LOC_DEVICE)
    check_rows(gpu, walk, rows, bin_samples=333, mask=ENVELOPE | DEPTH, states=states, location=LOC_DEVICE, scratch=1000)
    check_rows(gpu, walk, make_row("capture", 2 * SEG + 5)[None], starts_and_lengths(2 * SEG + 5, (0, 1, 65, SEG + 1, 2 * SEG + 5)), location=LOC_DEVICE)


def test_a_buffer_continued_from_a_state(gpu, walk):
    row = make_row("capture", 6000)
    head = gpu.signal_tap(row[None, :1000], FS)[1]
    check_rows(gpu, walk, row[None, 1000:], [(0, 0, 5000), (0, 10, 100)], states=head)


def test_the_binding(gpu, walk):
    rows = make_rows("capture", 5000, 2)
    ranges = [(1, 5, 500), (0, 0, 5000)]
    got = gpu.signal_tap_reduce(rows, FS, ENVELOPE | DEPTH, ranges=ranges)
    compare(got, lambda b: walk(rows[b])[0], ranges, ENVELOPE | DEPTH)
    got, states, report = gpu.signal_tap_reduce(rows, FS, VALUE, bin_samples=1024, with_state=True)
    compare(got, lambda b: walk(rows[b])[0], ranges_of_bins(2, 5000, 1024), VALUE)
    assert TS.same_state(states[1:2], walk(rows[1])[1]) and report.chunks > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. frames
# ---------------------------------------------------------------------------------------------------------------------

def test_the_frames_of_the_capture_as_ranges(gpu, walk):
    """the capture decoded through submit; every frame of the buffer as a range from the state the stream stood in before"""
    import nfclab_amd
    x, _ = TS.capture()
    x = np.ascontiguousarray(x[:200000])
    sid = gpu.open()
    try:
        state = gpu.stream_tap_state(sid)
        gpu.submit(sid, x, FS)
        frames = gpu.poll(sid)
    finally:
        gpu.close_stream(sid)
    ranges, kept = nfclab_amd.frame_ranges(frames, state, x.size)
    data = [k for k in kept if frames[k][1] in (nfclab_amd.FRAME_POLL, nfclab_amd.FRAME_LISTEN)]
    assert len(data) >= 2
    for r, k in zip(ranges, kept):  # clock of sample i: state.clock + 1 + i = i for a stream just opened
        assert r["first"] == frames[k][5] and r["first"] + r["count"] - 1 == min(frames[k][6], x.size - 1)
    listed = [(int(r["buffer"]), int(r["first"]), int(r["count"])) for r in ranges]
    got, _ = check_rows(gpu, walk, x[None], listed, mask=ENVELOPE | DEPTH)
    polls = [list(kept).index(k) for k in data if frames[k][1] == nfclab_amd.FRAME_POLL]
    assert polls and (got["max"][polls, 1] > 0.5).all()  # the reader's frames of NFC-A switch the carrier off

    # ... from a state behind other samples, clipped to the buffer, frames outside it dropped
    later = state.copy()
    later["clock"] = int(frames[data[0]][5]) + 9  # sample 0 is the eleventh of the first frame
    clipped, kept_later = nfclab_amd.frame_ranges(frames, later, 1000)
    assert data[0] in kept_later and all(frames[k][6] >= frames[data[0]][5] + 10 for k in kept_later)
    first = clipped[list(kept_later).index(data[0])]
    assert first["first"] == 0 and first["count"] == min(frames[data[0]][6] - frames[data[0]][5] - 9, 1000)
    assert (clipped["first"] + clipped["count"] <= 1000).all() and (clipped["buffer"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------

def refusals():
    """(what, changes to the call, the code, the word nfcgpu_last_error must carry)"""
    return [("a range in no buffer", {"ranges": [(0, 0, 10), (2, 0, 10)]}, EINVAL, "range 1"),
            ("a range beyond the buffer", {"ranges": [(1, 60, 5)]}, EINVAL, "range 0"),
            ("a range whose first + count wraps", {"ranges": [(1, 0xFFFFFFFF, 2)]}, EINVAL, "range 0"),
            ("a range with reserved not zero", {"ranges": [(0, 0, 10)], "range_reserved": 1}, EINVAL, "range 0"),
            ("neither ranges nor bins", {"ranges": None, "bin_samples": 0}, EINVAL, "bin_samples"),
            ("bins and a count of ranges", {"ranges": None, "bin_samples": 16, "n_ranges": 1}, EINVAL, "n_ranges"),
            ("reduce NULL", {"reduce_null": True}, EINVAL, "reduce is NULL"),
            ("reserved0 of reduce", {"reserved0": 1}, EINVAL, "reserved"),
            ("reserved of reduce", {"reserved": 1}, EINVAL, "reserved"),
            ("out on an odd byte", {"out_shift": 2}, EINVAL, "out"),
            ("out NULL", {"out_null": True}, EINVAL, "out is NULL"),
            ("ranges on an odd byte", {"ranges_shift": 1}, EINVAL, "ranges"),
            ("more than 2^32 - 1 records", {"ranges": None, "bin_samples": 1, "n_buffers": 12000000}, EINVAL, "records"),
            # ... and what the tap refuses, with the tap's codes
            ("tap NULL", {"tap_null": True}, EINVAL, "params is NULL"),
            ("no channel", {"mask": 0}, EINVAL, "channels"),
            ("reserved of tap", {"tap_reserved": 1}, EINVAL, "reserved"),
            ("stride 3", {"stride": 3}, EINVAL, "stride"),
            ("unknown format", {"fmt": 2}, EINVAL, "format"),
            ("unknown location", {"location": 2}, EINVAL, "location"),
            ("chunk no multiple of 64", {"chunk": 96}, EINVAL, "chunk_samples"),
            ("in NULL", {"in_null": True}, EINVAL, "in is"),
            ("in pitch smaller than a row", {"in_pitch": 64 * 8 - 8}, EINVAL, "in_pitch_bytes"),
            ("state_in misaligned", {"state_in_shift": 2}, EINVAL, "state_in"),
            ("rate 0", {"rate": 0}, EINVAL, "sample rate"),
            ("a rate the decoder refuses", {"rate": 20000000}, ERATE, "sample rate")]


@pytest.mark.parametrize("what,call,code,word", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_return_their_code_and_write_nothing(gpu, what, call, code, word):
    import nfclab_amd
    n, nb = 64, 2
    x = as_layout(make_rows("noise", n + 6, nb), 2, F32)
    ranges = call.get("ranges", [(0, 0, 64), (1, 3, 20)])
    given = None if ranges is None else nfclab_amd.as_tap_ranges(ranges)
    if given is not None:
        given["reserved"][0] = call.get("range_reserved", 0)
    out = np.full(6 * 32 * 32, GUARD, dtype=np.uint8)
    states = np.zeros(nb + 1, dtype=nfclab_amd.TAP_STATE_DTYPE)
    state_out = np.full(nb + 1, 7, dtype=np.uint32).repeat(8).view(nfclab_amd.TAP_STATE_DTYPE)
    before = state_out.tobytes()
    report = nfclab_amd.TapReport(9, 9, 9, 9)
    rc = raw_call(gpu, None if call.get("in_null") else x, call.get("in_pitch", (n + 6) * 8), call.get("n_buffers", nb), n, call.get("stride", 2),
                  call.get("fmt", F32), call.get("rate", FS), call.get("mask", ALL), states.ctypes.data + call.get("state_in_shift", 0),
                  None if given is None else given.ctypes.data + call.get("ranges_shift", 0), call.get("n_ranges", 0 if given is None else given.shape[0]),
                  None if call.get("out_null") else out.ctypes.data + call.get("out_shift", 0), state_out, call.get("bin_samples", 0), 0, report,
                  call.get("location", LOC_HOST), call.get("chunk", 0), call.get("tap_reserved", 0), call.get("reserved0", 0), call.get("reserved", 0),
                  call.get("reduce_null", False), call.get("tap_null", False))
    assert rc == code
    assert (out == GUARD).all() and state_out.tobytes() == before and report.chunks == 9
    assert word in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()


def test_a_null_context_is_refused(gpu):
    x, out = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    assert raw_call(type("none", (), {"lib": gpu.lib, "ctx": None}), x, 256, 1, 64, 1, F32, FS, VALUE, None, None, 0, out, None, bin_samples=16) == EINVAL


def test_a_bad_range_in_device_memory(gpu, walk):
    """the kernels refuse it: its records are empty, every other record and the states are complete, the call says NFCGPU_EINVAL"""
    rows = make_rows("capture", 5000, 3)
    good = scattered(3, 5000, 3, 21)
    bad = {2: (3, 0, 10), 5: (1, 4990, 11), 7: (0xFFFFFFFF, 0, 0), 8: (2, 0xFFFFFFFF, 2)}
    ranges = list(good)
    for at, r in bad.items():
        ranges[at] = r
    for scratch in (0, 1000):
        got, state_out, _ = reduce_rows(gpu, rows, ranges, mask=ENVELOPE | DEPTH, scratch=scratch, location=LOC_DEVICE, expect=EINVAL)
        assert "range in device memory" in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()
        kept = [r for r in range(len(ranges)) if r not in bad]
        compare(got[kept], lambda b: walk(rows[b])[0], [ranges[r] for r in kept], ENVELOPE | DEPTH)
        for r in bad:
            assert got[r].tobytes() == np.repeat(empty_record(), 2).tobytes()
        assert all(TS.same_state(state_out[b:b + 1], walk(rows[b])[1]) for b in range(3))
    # reserved can only be set through the raw structure
    import nfclab_amd
    given = nfclab_amd.as_tap_ranges(good)
    given["reserved"][4] = 1
    got, _, _ = reduce_rows(gpu, rows, given, mask=VALUE, location=LOC_DEVICE, expect=EINVAL)
    assert got[4].tobytes() == empty_record().tobytes() and got["valid"][3, 0] == good[3][2]


def test_empty_calls_succeed(gpu, walk):
    import nfclab_amd
    rows = make_rows("noise", 16, 2)
    # no ranges: nothing but the states is written
    got, state_out, report = reduce_rows(gpu, rows, [], mask=ALL)
    assert got.shape == (0, 6) and report.chunks == 2 and TS.same_state(state_out[:1], walk(rows[0])[1])
    reduce_rows(gpu, rows, [], mask=ALL, location=LOC_DEVICE)
    # no buffers: nothing is written
    out = np.full(64, GUARD, dtype=np.uint8)
    state_out = np.full(2, 7, dtype=np.uint32).repeat(8).view(nfclab_amd.TAP_STATE_DTYPE)
    before = state_out.tobytes()
    assert raw_call(gpu, rows, 64, 0, 16, 1, F32, FS, ALL, None, None, 0, out, state_out, bin_samples=4) == 0
    assert (out == GUARD).all() and state_out.tobytes() == before
    # no samples: no bins; ranges of no samples are empty records; state_out is state_in
    states = gpu.tap_state_init(2)
    states["clock"] = [41, 42]
    assert raw_call(gpu, rows, 64, 2, 0, 1, F32, FS, ALL, states, None, 0, out, state_out, bin_samples=4) == 0
    assert (out == GUARD).all() and state_out.tobytes() == states.tobytes()
    ranges = nfclab_amd.as_tap_ranges([(1, 0, 0), (0, 0, 0)])
    recs = np.full(2 * 2 * 32 + 32, GUARD, dtype=np.uint8)
    assert raw_call(gpu, rows, 64, 2, 0, 1, F32, FS, VALUE | DEPTH, None, ranges, 2, recs, state_out) == 0
    assert recs[:128].tobytes() == np.repeat(empty_record(), 4).tobytes() and (recs[128:] == GUARD).all()
    assert state_out.tobytes() == gpu.tap_state_init(2).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the CPU twin of the emulated library and the device kernels
# ---------------------------------------------------------------------------------------------------------------------

def twin_cases():
    """(rows, keyword arguments of NfcGpu.signal_tap_reduce)"""
    long_row = make_row("capture", 2 * SEG + 5)[None]
    rows = np.concatenate([make_rows("capture", 5000, 3), make_rows("steps", 5000, 2), make_rows("zeros", 5000, 1)])
    return [(long_row, dict(channels=ALL, ranges=[r for r in starts_and_lengths(2 * SEG + 5)])),
            (long_row, dict(channels=FILTERED | DEPTH, bin_samples=4096)),
            (rows, dict(channels=ALL, ranges=scattered(6, 5000, 8, 13), scratch_bytes=2 * 6 * 20224)),
            (rows, dict(channels=ENVELOPE | DEPTH, bin_samples=100)),
            (as_layout(rows, 2, I16), dict(channels=ALL, bin_samples=1000, stride=2, fmt=I16))]


def dump_outputs(path):
    """Child process (NFCGPU_LIB names the library): the records of twin_cases(), in order, to one file."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    records = []
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for rows, how in twin_cases():
            records.append(g.signal_tap_reduce(rows, FS, **how).reshape(-1))
    np.save(path, np.concatenate(records).view(np.uint8))


def test_twin_equals_device(gpu, tmp_path):
    """every record - the mean and its order of additions included - is the same bytes from the emulated library's twins and from
    the device kernels"""
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
        sys.exit("usage: test_tap_reduce.py --dump OUT.npy")
