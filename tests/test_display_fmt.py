"""nfcgpu_spectrum_fmt and nfcgpu_resample_radio_fmt: the two display consumers of a capture reading the sample formats the
decoder reads (int16 PCM, mono and I/Q; float I/Q for the resampler) where they lie, through the C ABI.

Both calls are defined by the float calls they extend, so the yardstick is those calls, bit for bit (outputs compared as
uint32):
  spectrum   nfcgpu_spectrum on a float buffer holding v.astype(float32) / 32768 (int16 -> float is exact, and from
             there on the kernel takes the float kernel's operations);
  resampler  nfcgpu_resample_radio on the magnitudes the decoder's loader forms of the same bytes: v / 32768 (mono),
             nfcgpu_magnitude_fmt (I/Q). The float resampler is pinned to the reference's task and nfcgpu_magnitude to the
             reference's formula by tests/test_gpu_parity.py.
On top of that the int16 spectrum is held against the recorded reference task and the float64 statement of
tests/test_spectrum.py under that file's bounds, unchanged.

The same file runs on the CPU against the emulated library (tests/test_display_fmt_emulated.py), whose twins of the new
kernels compile the same text (nfc-laboratory_amd/csrc/nfc_spectrum.hpp, nfc_resample.hpp)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nfc_testlib as T
import test_spectrum as S

pytestmark = pytest.mark.gpu

EMU = S.EMU
EINVAL, EOVERFLOW = -1, -6
LOC_HOST, LOC_DEVICE = 0, 1
FMT_F32, FMT_I16 = 0, 1
PATTERN = S.PATTERN
FIXTURE = "test_NFC-A_106kbps_001"


@pytest.fixture(scope="module")
def gpu(built):
    import nfclab_amd
    g = nfclab_amd.NfcGpu(device=0, max_streams=64)
    yield g
    g.close()


def last_error(gpu):
    return gpu.lib.nfcgpu_last_error(gpu.ctx).decode()


def to_i16(x):
    """float values on the int16 grid as int16 (32768, which the grid of make_input("int16") can reach, becomes 32767)"""
    v = np.round(np.asarray(x, dtype=np.float64) * 32768)
    assert np.array_equal(v, np.asarray(x, dtype=np.float64) * 32768), "not on the int16 grid"
    return np.clip(v, -32768, 32767).astype(np.int16)


def to_f32(v):
    return (v.astype(np.float32) / np.float32(32768)).astype(np.float32)


def misaligned_rows(dense, pitch_items, modulo, residue):
    """dense [nb, row] copied into rows pitch_items apart that start `residue` bytes behind an address that is a multiple of
    `modulo`: (the bytes from that address on, residue). A copy of the bytes that is aligned alike - a device allocation -
    keeps the rows where they are."""
    nb, row = dense.shape
    size = nb * pitch_items * dense.itemsize
    raw = np.full(size + residue + modulo, 0xA5, dtype=np.uint8)
    lead = (-raw.ctypes.data) % modulo
    keeper = raw[lead:lead + residue + size]
    keeper[residue:].view(dense.dtype).reshape(nb, pitch_items)[:, :row] = dense
    assert keeper.ctypes.data % modulo == 0
    return keeper, residue


# ---------------------------------------------------------------------------------------------------------------------
# spectrum
# ---------------------------------------------------------------------------------------------------------------------

def spectrum_fmt_call(gpu, ptr, in_pitch, n_buffers, n_pairs, params, out, out_pitch, location=LOC_HOST, fmt=FMT_I16):
    op = out if isinstance(out, int) else out.ctypes.data
    return gpu.lib.nfcgpu_spectrum_fmt(gpu.ctx, ptr, in_pitch, n_buffers, n_pairs, ctypes.byref(params), op, out_pitch, location, fmt)


def full_range_pairs(seed, n_buffers, n_pairs):
    rng = np.random.default_rng(seed)
    v = rng.integers(-32768, 32768, (n_buffers, n_pairs, 2)).astype(np.int16)
    v[:, 0] = (-32768, 32767)
    v[:, -1] = (32767, -32768)
    return v


@pytest.mark.parametrize("window", S.WINDOWS)
@pytest.mark.parametrize("length", [256, 512, 1024, 2048, 4096])
def test_spectrum_bit_equality_with_the_float_path(gpu, length, window):
    nb = 3
    for decimation in (1, 3, 16):
        span = length * decimation
        for hop in (0, 1, 77):
            for n_pairs in (span, span - 1, span + 2 * hop + 1):
                v = full_range_pairs(length + 31 * decimation + hop, nb, n_pairs)
                want = gpu.spectrum(to_f32(v), length=length, window=window, decimation=decimation, hop=hop)
                frames = want.shape[1]
                assert frames == (0 if n_pairs < span else (1 if hop == 0 else (n_pairs - span) // hop + 1))
                # rows 3 pairs further apart than they are long, from a base that is 4-byte and not 8-byte aligned
                keeper, at = misaligned_rows(v.reshape(nb, -1), 2 * (n_pairs + 3), 8, 4)
                ptr = keeper.ctypes.data + at
                out_pitch = frames * length + 8
                out = np.full((nb, out_pitch), PATTERN, dtype=np.uint32)
                p = gpu.spectrum_params(length=length, window=window, decimation=decimation, hop=hop)
                what = (decimation, hop, n_pairs)
                assert spectrum_fmt_call(gpu, ptr, (n_pairs + 3) * 4, nb, n_pairs, p, out, out_pitch * 4) == 0, what
                assert np.array_equal(out[:, :frames * length], want.reshape(nb, -1).view(np.uint32)), what
                assert (out[:, frames * length:] == PATTERN).all(), what
                # the binding, dense rows
                got = gpu.spectrum(v, length=length, window=window, decimation=decimation, hop=hop, fmt=FMT_I16)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def test_spectrum_of_int16_against_the_recorded_task(gpu):
    """tests/golden/spectrum/fourier_task.npy, the bound of test_spectrum.py: (T / 4 + T) * 2^-24 * peak."""
    recorded = np.load(os.path.join(S.GOLDEN, "fourier_task.npy"))
    x = S.golden_inputs()
    v = to_i16(x)
    assert np.array_equal(to_f32(v), x) and v.min() == -19746 and v.max() == 19750
    got = gpu.spectrum(v, fmt=FMT_I16)
    assert got.shape == (3, 1, 1024)
    t = S.tolerance(1024)
    for b in range(3):
        peak = float(recorded[b].max())
        error = np.max(np.abs(got[b, 0].astype(np.float64) - recorded[b].astype(np.float64))) / (S.EPS * peak)
        print("buffer %d: %.2f units of 2^-24 * peak against the recorded task, bound %.2f" % (b, error, t / 4 + t))
        assert error <= t / 4 + t


@pytest.mark.parametrize("length,window,decimation,kind", S.value_cases([256, 512, 1024, 2048, 4096], ("int16",)))
def test_spectrum_values_of_int16_against_the_float64_statement(gpu, length, window, decimation, kind):
    v = to_i16(S.value_input(length, window, decimation, kind))
    fed = to_f32(v)
    got = gpu.spectrum(v, length=length, window=window, decimation=decimation, fmt=FMT_I16)
    assert got.shape == (S.VALUE_BUFFERS, 1, length) and got.dtype == np.float32
    t = S.tolerance(length)
    worst = 0.0
    for b in range(S.VALUE_BUFFERS):
        want = S.yardstick(fed[b], length, window, decimation)
        worst = max(worst, np.max(np.abs(got[b, 0].astype(np.float64) - want)) / (S.EPS * want.max()))
    print("L %d %s D %d int16: worst error %.2f units of 2^-24 * peak, T = %.2f" % (length, window, decimation, worst, t))
    assert worst <= t


def test_spectrum_host_and_device_location_give_the_same_bytes(gpu):
    L, D, hop, nb = 1024, 16, 5001, 4
    n_pairs = L * D + 2 * hop
    v = full_range_pairs(45, nb, n_pairs)
    host = gpu.spectrum(v, length=L, decimation=D, hop=hop, fmt=FMT_I16)
    assert host.shape == (nb, 3, L)
    # on the device: rows 5 pairs further apart, the base one pair behind an aligned address
    pitch_pairs = n_pairs + 5
    padded = np.zeros((1 + nb * pitch_pairs, 2), dtype=np.int16)
    padded[1:].reshape(nb, pitch_pairs, 2)[:, :n_pairs] = v
    dx, dout = S.DeviceArray(padded), S.DeviceArray(np.zeros((nb, 3, L), dtype=np.float32))
    assert dx.ptr % 8 == 0
    assert gpu.spectrum_device(dx.ptr + 4, pitch_pairs * 4, nb, n_pairs, dout.ptr, 3 * L * 4, length=L, decimation=D, hop=hop, fmt=FMT_I16) == 3
    assert np.array_equal(dout.read().view(np.uint32), host.view(np.uint32))


def test_spectrum_one_call_for_many_frames_equals_the_single_calls(gpu):
    L, D, hop, frames, nb = 1024, 16, 777, 5, 3
    span = L * D
    v = full_range_pairs(44, nb, span + (frames - 1) * hop)
    got = gpu.spectrum(v, length=L, decimation=D, hop=hop, fmt=FMT_I16)
    assert got.shape == (nb, frames, L)
    for b in range(nb):
        for f in range(frames):
            single = gpu.spectrum(v[b:b + 1, f * hop:f * hop + span], length=L, decimation=D, fmt=FMT_I16)
            assert np.array_equal(got[b, f].view(np.uint32), single[0, 0].view(np.uint32)), (b, f)


def spectrum_refusals():
    """(what, format, changes to the call); the call is two buffers of 2048 pairs, L = 1024, hop 1024: two frames each"""
    return [("unknown format", 2, {}),
            ("iq is NULL", FMT_I16, {"ptr": 0}),
            ("out is NULL", FMT_I16, {"out": 0}),
            ("int16 base at an odd 2-byte address", FMT_I16, {"offset": 2}),
            ("float base at a 4-byte address", FMT_F32, {"offset": 4}),
            ("int16 pitch not a multiple of 4", FMT_I16, {"in_pitch": 2056 * 4 + 2}),
            ("float pitch not a multiple of 8", FMT_F32, {"in_pitch": 2056 * 8 + 4}),
            ("out pitch below the frames, int16", FMT_I16, {"out_pitch": 2 * 1024 * 4 - 16}),
            ("out pitch below the frames, float", FMT_F32, {"out_pitch": 2 * 1024 * 4 - 16})]


@pytest.mark.parametrize("what,fmt,call", spectrum_refusals(), ids=[r[0] for r in spectrum_refusals()])
def test_spectrum_refusals_return_einval_and_write_nothing(gpu, what, fmt, call):
    L, n_pairs, nb = 1024, 2048, 2
    x = np.zeros(nb * 2056 * 2 + 8, dtype=np.float32)  # room for either format, 8-byte aligned
    assert x.ctypes.data % 8 == 0
    p = gpu.spectrum_params(length=L, decimation=1, hop=1024)
    out = np.full((nb, 2 * L + 64), PATTERN, dtype=np.uint32)
    ptr = call.get("ptr", x.ctypes.data + call.get("offset", 0))
    in_pitch = call.get("in_pitch", 2056 * (4 if fmt == FMT_I16 else 8))
    rc = spectrum_fmt_call(gpu, ptr, in_pitch, nb, n_pairs, p, call.get("out", out), call.get("out_pitch", (2 * L + 64) * 4), LOC_HOST, fmt)
    assert rc == EINVAL
    assert (out == PATTERN).all()
    assert "spectrum" in last_error(gpu)
    # the same call without the fault is taken
    if fmt in (FMT_F32, FMT_I16):
        assert spectrum_fmt_call(gpu, x.ctypes.data, 2056 * (4 if fmt == FMT_I16 else 8), nb, n_pairs, p, out, (2 * L + 64) * 4, LOC_HOST, fmt) == 0
        assert not out[:, :2 * L].any() and (out[:, 2 * L:] == PATTERN).all()


@pytest.mark.parametrize("what,params,call,word", S.refusals(), ids=[r[0] for r in S.refusals()])
def test_spectrum_fmt_with_float_is_nfcgpu_spectrum_code_and_text(gpu, what, params, call, word):
    L, n_pairs, nb = 1024, 2048, 2
    x = S.make_input("noise", n_pairs + 8, 3, nb)
    p = gpu.spectrum_params(length=L, decimation=1, hop=1024)
    for key, value in params.items():
        if key == "reserved":
            p.reserved[2] = value
        else:
            setattr(p, key, value)
    in_pitch, out_pitch = call.get("in_pitch", (n_pairs + 8) * 8), call.get("out_pitch", (2 * L + 64) * 4)
    results = []
    for fmt in (None, FMT_F32):
        # (a refusal with another text in between: the text compared is the one this call sets)
        assert spectrum_fmt_call(gpu, x.ctypes.data, in_pitch, nb, n_pairs, p, 0, out_pitch, LOC_HOST, 7) == EINVAL
        assert "format" in last_error(gpu)
        out = np.full((nb, 2 * L + 64), PATTERN, dtype=np.uint32)
        if fmt is None:
            rc = S.raw_call(gpu, x, in_pitch, nb, n_pairs, p, out, out_pitch)
        else:
            rc = spectrum_fmt_call(gpu, x.ctypes.data, in_pitch, nb, n_pairs, p, out, out_pitch, LOC_HOST, fmt)
        assert (out == PATTERN).all()
        results.append((rc, last_error(gpu)))
    assert results[0] == results[1] and results[0][0] == EINVAL and word in results[0][1]


def test_spectrum_fmt_with_float_gives_the_bytes_of_nfcgpu_spectrum(gpu):
    L, D, hop, nb = 512, 3, 100, 2
    n_pairs = L * D + 3 * hop
    x = S.make_input("carrier", n_pairs, 8, nb)
    want = gpu.spectrum(x, length=L, decimation=D, hop=hop)
    p = gpu.spectrum_params(length=L, decimation=D, hop=hop)
    out = np.zeros_like(want)
    assert spectrum_fmt_call(gpu, x.ctypes.data, n_pairs * 8, nb, n_pairs, p, out, 4 * L * 4, LOC_HOST, FMT_F32) == 0
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# resampler
# ---------------------------------------------------------------------------------------------------------------------

LAYOUTS = {"int16 mono": (1, FMT_I16), "int16 iq": (2, FMT_I16), "float iq": (2, FMT_F32)}
RS_SIZES = (25, 26, 51, 95, 96, 97, 255, 256, 1000, 10007)  # window, tile, ring and interval edges
RS_BUFFERS = (1, 63, 64, 65, 130)
RS_LONGEST, RS_MOST = max(RS_SIZES), max(RS_BUFFERS)


def capacity_of(n):
    return n + n // 255 + 2


def resample_fmt_call(gpu, ptr, in_pitch, n_buffers, n, stride, fmt, out, out_pitch, capacity, counts, location=LOC_HOST):
    op = out if isinstance(out, int) else out.ctypes.data
    cp = counts if isinstance(counts, int) else counts.ctypes.data
    return gpu.lib.nfcgpu_resample_radio_fmt(gpu.ctx, ptr, in_pitch, n_buffers, n, stride, fmt, op, out_pitch, capacity, cp, location)


_signal = {}


def signal_rows(layout):
    """[RS_MOST, RS_LONGEST * stride] in the layout's dtype. Buffer b is the capture from 600 samples of idle carrier before
    its first frame on (tests/golden/wav/<FIXTURE>.json: sampleStart), moved on by 37 b samples: the frame, more than 600
    samples of idle carrier, the answer and the next frames. Buffer 1 of the I/Q layouts is full scale, (-32768, -32768),
    whose magnitude exceeds 1, with a pair that departs from it now and then."""
    if layout in _signal:
        return _signal[layout]
    stride, fmt = LAYOUTS[layout]
    with open(os.path.join(T.GOLDEN, "wav", FIXTURE + ".json")) as f:
        first_frame = json.load(f)["frames"][0]["sampleStart"]
    capture = T.load_fixture_i16(FIXTURE)
    start = first_frame - 600
    assert start >= 0 and start + 37 * (RS_MOST - 1) + RS_LONGEST <= capture.size
    mono = np.stack([capture[start + 37 * b:start + 37 * b + RS_LONGEST] for b in range(RS_MOST)])
    if stride == 1:
        rows = np.ascontiguousarray(mono)
    else:
        iq = np.stack([T.magnitude_to_iq(to_f32(mono[b]), seed=b, period=997) for b in range(RS_MOST)])
        rows = np.clip(np.round(iq.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
        rows[1] = -32768
        rows[1, 2 * 300::2 * 411] = 32767
        rows[1, 2 * 700 + 1::2 * 1013] = 0
        if fmt == FMT_F32:
            rows = to_f32(rows)
            rows[1] *= np.float32(1.5)  # beyond what int16 can hold
    _signal[layout] = rows
    return rows


def loader_magnitudes(gpu, rows, layout):
    """what the decoder's loader forms of the rows: [nb, n] float32"""
    stride, fmt = LAYOUTS[layout]
    if stride == 1:
        return to_f32(rows)
    return np.stack([gpu.magnitude(row, fmt=fmt) for row in rows])


_expected = {}


def expected_points(gpu, layout, n):
    """nfcgpu_resample_radio on the loader's magnitudes of the first n samples of every buffer, once per (layout, n): a list of
    [pairs, 2] arrays. Buffers are independent, so the first nb of them are what a call with nb buffers must give."""
    key = (layout, n, os.environ.get("NFCGPU_LIB", ""))
    if key not in _expected:
        stride, _ = LAYOUTS[layout]
        mags = loader_magnitudes(gpu, signal_rows(layout)[:, :n * stride], layout)
        assert mags.shape == (RS_MOST, n)
        _expected[key] = gpu.resample_radio(mags)
    return _expected[key]


def laid_out(rows, layout, n):
    """(bytes, where the rows start in them, pitch in bytes) of rows[:, :n samples]: int16 mono with odd n dense, so that rows
    start at 2-byte alignment; elsewhere a pitch three samples larger than the row; the base one sample behind a 16-byte
    boundary"""
    stride, fmt = LAYOUTS[layout]
    dense = np.ascontiguousarray(rows[:, :n * stride])
    item = dense.itemsize
    if layout == "int16 mono":
        pitch_items = n if n & 1 else n + 3
        keeper, at = misaligned_rows(dense, pitch_items, 16, 2)
    else:
        pitch_items = (n + 3) * stride
        keeper, at = misaligned_rows(dense, pitch_items, 16, stride * item)
    return keeper, at, pitch_items * item


def check_points(want, counts, out, what):
    for b, w in enumerate(want):
        assert counts[b] == w.shape[0], (what, b, int(counts[b]), w.shape[0])
        assert np.array_equal(out[b, :2 * w.shape[0]].view(np.uint32), w.reshape(-1).view(np.uint32)), (what, b)


@pytest.mark.parametrize("n", RS_SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_resampler_bit_equality_with_the_float_path(gpu, layout, n):
    stride, fmt = LAYOUTS[layout]
    rows = signal_rows(layout)
    want_all = expected_points(gpu, layout, n)
    cap = capacity_of(n)

    if n >= 1000:
        # a condition on the inputs: deviation points, "sample before" points and interval points are all there
        deviation = before = interval = 0
        for b, w in enumerate(want_all):
            mags = loader_magnitudes(gpu, rows[b:b + 1, :n * stride], layout)[0]
            offsets = w[:, 1].astype(np.int64)
            steps = np.diff(offsets)
            interval += int(np.count_nonzero(steps == 255))
            # a point whose value is not the interval's doing: it follows its predecessor by less than 255
            deviation += int(np.count_nonzero(steps[1:] < 255))
            # "sample before": a point at p = i - 1 directly in front of a deviation point at i, behind a gap
            before += int(np.count_nonzero((steps[1:] == 1) & (steps[:-1] > 1)))
            assert np.array_equal(w[:, 0].view(np.uint32), mags[offsets].view(np.uint32))
        assert deviation and before and interval, (deviation, before, interval)

    for nb in RS_BUFFERS:
        keeper, at, pitch = laid_out(rows[:nb], layout, n)
        want = want_all[:nb]

        out = np.zeros((nb, 2 * cap + 2), dtype=np.float32)
        counts = np.zeros(nb, dtype=np.uint32)
        assert resample_fmt_call(gpu, keeper.ctypes.data + at, pitch, nb, n, stride, fmt, out, out.shape[1] * 4, cap, counts) == 0, nb
        check_points(want, counts, out, ("host", nb))

        din, dout, dcounts = S.DeviceArray(keeper), S.DeviceArray(np.zeros_like(out)), S.DeviceArray(np.zeros(nb, dtype=np.uint32))
        assert din.ptr % 16 == 0
        gpu.resample_radio_device(din.ptr + at, pitch, nb, n, dout.ptr, out.shape[1] * 4, cap, dcounts.ptr, stride=stride, fmt=fmt)
        check_points(want, dcounts.read(), dout.read(), ("device", nb))

    # the binding, dense rows
    got = gpu.resample_radio(rows[:3, :n * stride], stride=stride, fmt=fmt)
    for b in range(3):
        assert np.array_equal(got[b].view(np.uint32), want_all[b].view(np.uint32)), b


@pytest.mark.parametrize("name,per_buffer", [("test_NFC-A_106kbps_001", 65536), ("test_POLL_ABF_001", 65536), ("test_NFC-V_26kbps_001", 10007)])
def test_resampler_of_int16_matches_the_reference_task(gpu, tmp_path, name, per_buffer):
    """The capture's own int16 samples against the reference's SignalResamplingTask, bit for bit, the shorter last buffer
    included (tests/test_gpu_parity.py::test_adaptive_resampler_matches_reference_task, fed without the widening)."""
    want = T.reference_resample(name, tmp_path, per_buffer)
    if want is None:
        pytest.skip("oracle/_ref/resample-ref not available")
    v = T.load_fixture_i16(name)
    full = v.size // per_buffer
    got = []
    if full:
        got += gpu.resample_radio(v[:full * per_buffer].reshape(full, per_buffer), fmt=FMT_I16)
    if v.size % per_buffer:
        got += gpu.resample_radio(v[full * per_buffer:].reshape(1, -1), fmt=FMT_I16)
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.reshape(-1).view(np.uint32), w.view(np.uint32)), "buffer %d: %d vs %d floats" % (b, g.size, w.size)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_resampler_overflow_keeps_counting(gpu, layout):
    stride, fmt = LAYOUTS[layout]
    n, nb = 1000, 3
    rows = np.ascontiguousarray(signal_rows(layout)[:nb, :n * stride])
    want = expected_points(gpu, layout, n)[:nb]
    cap = min(w.shape[0] for w in want) - 1
    assert cap > 0
    out = np.zeros((nb, 2 * cap), dtype=np.uint32)
    counts = np.zeros(nb, dtype=np.uint32)
    rc = resample_fmt_call(gpu, rows.ctypes.data, rows.shape[1] * rows.itemsize, nb, n, stride, fmt, out, out.shape[1] * 4, cap, counts)
    assert rc == EOVERFLOW and "capacity" in last_error(gpu)
    for b, w in enumerate(want):
        assert counts[b] == w.shape[0]
        assert np.array_equal(out[b], w.reshape(-1)[:2 * cap].view(np.uint32)), b


def resampler_refusals():
    """(what, stride, format, changes to the call); the call is two buffers of 100 samples, rows 104 samples apart"""
    sample = {(1, FMT_I16): 2, (2, FMT_I16): 4, (1, FMT_F32): 4, (2, FMT_F32): 8}
    cases = [("stride 0", 0, FMT_I16, {}), ("stride 3", 3, FMT_F32, {}), ("unknown format", 1, 2, {})]
    for (stride, fmt), size in sample.items():
        tag = "%s stride %d" % ("int16" if fmt == FMT_I16 else "float", stride)
        cases.append(("misaligned in, " + tag, stride, fmt, {"offset": size // 2}))
        cases.append(("misaligned pitch, " + tag, stride, fmt, {"in_pitch": 104 * size + size // 2}))
        cases.append(("24 samples, " + tag, stride, fmt, {"n": 24}))
        cases.append(("pitch below the row, " + tag, stride, fmt, {"in_pitch": 99 * size}))
    return cases


@pytest.mark.parametrize("what,stride,fmt,call", resampler_refusals(), ids=[r[0] for r in resampler_refusals()])
def test_resampler_refusals_return_einval_and_write_nothing(gpu, what, stride, fmt, call):
    nb, n = 2, call.get("n", 100)
    size = max(stride, 1) * (2 if fmt == FMT_I16 else 4)
    x = np.zeros(nb * 104 * 8 + 16, dtype=np.uint8)
    assert x.ctypes.data % 8 == 0
    out = np.full((nb, 2 * capacity_of(100)), PATTERN, dtype=np.uint32)
    counts = np.full(nb, PATTERN, dtype=np.uint32)
    rc = resample_fmt_call(gpu, x.ctypes.data + call.get("offset", 0), call.get("in_pitch", 104 * size), nb, n, stride, fmt, out,
                           out.shape[1] * 4, capacity_of(100), counts)
    assert rc == EINVAL
    assert (out == PATTERN).all() and (counts == PATTERN).all()


def test_resampler_fmt_with_float_magnitudes_is_nfcgpu_resample_radio_code_and_text(gpu):
    n, nb = 1000, 3
    mags = np.ascontiguousarray(to_f32(signal_rows("int16 mono")[:nb, :n]))
    want = gpu.resample_radio(mags)
    assert [np.array_equal(g, w) for g, w in zip(gpu.resample_radio(mags, stride=1, fmt=FMT_F32), want)] == [True] * nb
    full, short = capacity_of(n), min(w.shape[0] for w in want) - 1
    for what, n_call, pitch, cap in (("taken", n, n * 4, full), ("overflow", n, n * 4, short), ("24 samples", 24, n * 4, full),
                                     ("pitch below the row", n, n * 4 - 4, full), ("misaligned pitch", n, n * 4 + 2, full)):
        results = []
        for through_fmt in (False, True):
            # (a refusal with a text of its own in between: the text compared is what this call leaves behind)
            assert resample_fmt_call(gpu, mags.ctypes.data, pitch, nb, n_call, 3, FMT_F32, 0, 0, 0, 0) == EINVAL
            assert "stride" in last_error(gpu)
            out = np.zeros((nb, 2 * full), dtype=np.float32)
            counts = np.zeros(nb, dtype=np.uint32)
            if through_fmt:
                rc = resample_fmt_call(gpu, mags.ctypes.data, pitch, nb, n_call, 1, FMT_F32, out, 2 * full * 4, cap, counts)
            else:
                rc = gpu.lib.nfcgpu_resample_radio(gpu.ctx, mags.ctypes.data, pitch, nb, n_call, out.ctypes.data, 2 * full * 4, cap,
                                                   counts.ctypes.data, LOC_HOST)
            written = [out[b, :2 * min(int(counts[b]), cap)].tobytes() for b in range(nb)]  # (beyond a buffer's pairs nothing is promised)
            results.append((rc, last_error(gpu), counts.tobytes(), written))
        assert results[0] == results[1], what
        assert results[0][0] == {"taken": 0, "overflow": EOVERFLOW}.get(what, EINVAL), what


# ---------------------------------------------------------------------------------------------------------------------
# the CPU twins of the emulated library and the device kernels
# ---------------------------------------------------------------------------------------------------------------------

def twin_spectrum_cases():
    return [(length, window, decimation) for length in (256, 512, 1024, 2048, 4096) for window in S.WINDOWS for decimation in (1, 16)]


def dump_outputs(path):
    """Child process (NFCGPU_LIB names the library): what both calls give for fixed inputs, in order, to one file."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    spectra, points = [], []
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for length, window, decimation in twin_spectrum_cases():
            v = full_range_pairs(length + decimation, 2, length * decimation + 2 * 33)
            spectra.append(g.spectrum(v, length=length, window=window, decimation=decimation, hop=33, fmt=FMT_I16).reshape(-1))
        for layout, (stride, fmt) in LAYOUTS.items():
            for n in (25, 97, 1000, 10007):
                for got in g.resample_radio(signal_rows(layout)[:66, :n * stride], stride=stride, fmt=fmt):
                    points.append(np.float32([got.shape[0]]))
                    points.append(got.reshape(-1))
    np.savez(path, spectra=np.concatenate(spectra), points=np.concatenate(points))


def test_twins_equal_device(built, tmp_path):
    """The emulated library's twins and the device kernels compile the same arithmetic (tables from the host, no contraction,
    the resampler's sum in its one order): what both calls write is compared as uint32, bit for bit."""
    if S.on_emulated_library():
        pytest.skip("NFCGPU_LIB is the emulated library: there is no device to compare with")
    if not os.path.exists(EMU):
        pytest.skip("tests/hostsim/libnfcgpu_emulated.so is not built")
    import nfclab_amd
    outputs = {}
    for name, lib, extra in (("device", nfclab_amd.LIB_PATH, {}), ("twin", EMU, {"NFCGPU_NO_TORCH": "1"})):
        path = str(tmp_path / (name + ".npz"))
        env = dict(os.environ, NFCGPU_LIB=lib, **extra)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], cwd=T.ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-3000:]
        outputs[name] = np.load(path)
    for key in ("spectra", "points"):
        device, twin = outputs["device"][key], outputs["twin"][key]
        assert device.shape == twin.shape and device.size, key
        differ = np.flatnonzero(device.view(np.uint32) != twin.view(np.uint32))
        assert differ.size == 0, "%s: %d of %d floats differ, first at %d" % (key, differ.size, twin.size, differ[0])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        sys.path.insert(0, os.path.join(T.ROOT, "tests"))
        dump_outputs(sys.argv[2])
    else:
        sys.exit("usage: test_display_fmt.py --dump OUT.npz")
