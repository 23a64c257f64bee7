"""int16 PCM input of the decoder (NFCGPU_FMT_I16: nfcgpu_submit_fmt, nfcgpu_submit_batch_fmt, nfcgpu_submit_uniform_fmt,
nfcgpu_magnitude_fmt), through the C ABI. The contract: the kernels convert while they load, value = (float)v / 32768.0f, which is
exact, so any sequence of calls with int16 buffers gives exactly the frames, in every field and order, that the same sequence
gives with float buffers holding the converted values - and takes the time-parallel path exactly when those would.

On the GPU (`-m gpu`) this runs the device loaders: the int16 kernels' row staging, the slice offsets in bytes per sample, the
staging of host rows as int16. tests/test_int16_input_emulated.py runs the same file against the emulated library, where int16
input is widened on the host before the float twins see it (nfcgpu.hip, widen_i16): that covers the argument checks, the rate
adoption and the binding, not the device loaders."""
import ctypes
import os

import numpy as np
import pytest

import nfc_testlib as T

pytestmark = pytest.mark.gpu

NAMES = T.fixture_names()
FS = 10000000
THRESHOLD = 32768  # shortest submission that may take the time-parallel path (nfcgpu.hip: windowedMinSamples)
EINVAL = -1

# the emulated library (tests/hostsim/build_emulated.sh): "device" memory is host memory there, and there is no torch
EMULATED = os.path.basename(os.environ.get("NFCGPU_LIB", "")) == "libnfcgpu_emulated.so"


@pytest.fixture(scope="module")
def gpu(built):
    import nfclab_amd
    g = nfclab_amd.NfcGpu(device=0, max_streams=256, frame_sink_bytes=64 << 20)
    yield g
    g.close()


def FMT():
    import nfclab_amd
    return nfclab_amd.FMT_F32, nfclab_amd.FMT_I16


def to_float(v):
    """what hw::RecordDevice::readScaledSamples<short> makes of int16 (RecordDevice.cpp:247-248, 297-300)"""
    return (np.asarray(v, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def data_frames(frames):
    return [f for f in frames if f[1] in (0x102, 0x103)]


def numpy_magnitude(iq_i16):
    """the reference's scalar formula in numpy float32: components converted, products and sum rounded separately, np.sqrt"""
    f = to_float(iq_i16)
    i, q = f[0::2], f[1::2]
    return np.sqrt((i * i).astype(np.float32) + (q * q).astype(np.float32)).astype(np.float32)


def device_copy(array):
    """(keep-alive object, device pointer) of a numpy array's contents in device memory"""
    array = np.ascontiguousarray(array)
    if EMULATED:
        return array, array.ctypes.data
    import torch
    t = torch.from_numpy(array).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def decode_pieces(gpu, pieces, stride=1):
    """one stream fed with (array, fmt) pieces in turn; returns (all frames, windowed_streams, fallback_streams)"""
    sid = gpu.open()
    gpu.sync()
    gpu.stats_reset()
    for part, fmt in pieces:
        gpu.submit(sid, np.ascontiguousarray(part), FS, stride=stride, fmt=fmt)
    frames = gpu.poll(sid)
    st = gpu.stats()
    gpu.close_stream(sid)
    return frames, int(st.windowed_streams), int(st.fallback_streams)


@pytest.mark.parametrize("name", NAMES)
def test_every_capture_whole_as_int16_gives_the_goldens_on_the_path_the_floats_take(gpu, name):
    F32, I16 = FMT()
    v = T.load_fixture_i16(name)
    got, windowed, fallback = decode_pieces(gpu, [(v, I16)])
    assert data_frames(got) == T.load_golden(name)
    want, windowed_f, fallback_f = decode_pieces(gpu, [(T.load_fixture(name), F32)])
    assert got == want
    print("%s: windowed %d fallback %d (float: %d %d)" % (name, windowed, fallback, windowed_f, fallback_f))
    assert (windowed, fallback) == (windowed_f, fallback_f)
    # every capture is longer than the threshold: the whole submission is one the time-parallel path is offered
    assert v.size >= THRESHOLD and windowed + fallback >= 1


def cut_points(name, size):
    """seeded cuts: pieces longer and shorter than the threshold in turn, the first cut at an odd sample index"""
    rng = np.random.default_rng(T.splitmix64(sum(name.encode()) + size) & 0xFFFFFFFF)
    cuts, at, long_piece = [], 0, True
    while True:
        n = int(THRESHOLD + 1 + rng.integers(0, 70000)) if long_piece else int(rng.integers(1, 20000))
        if not cuts:
            n |= 1
        if at + n >= size:
            break
        at += n
        cuts.append(at)
        long_piece = not long_piece
    return cuts


@pytest.mark.parametrize("name", NAMES)
def test_pieces_cut_anywhere_in_alternating_formats_give_the_frames_of_the_whole(gpu, name):
    F32, I16 = FMT()
    v = T.load_fixture_i16(name)
    cuts = cut_points(name, v.size)
    edges = [0] + cuts + [v.size]
    lengths = [b - a for a, b in zip(edges, edges[1:])]
    assert any(n > THRESHOLD for n in lengths) and any(n < THRESHOLD for n in lengths) and any(c & 1 for c in cuts), (cuts, lengths)
    for first in (I16, F32):
        pieces = []
        for k, (a, b) in enumerate(zip(edges, edges[1:])):
            fmt = first if k % 2 == 0 else (F32 if first == I16 else I16)
            pieces.append((v[a:b] if fmt == I16 else to_float(v[a:b]), fmt))
        got, _, _ = decode_pieces(gpu, pieces)
        assert data_frames(got) == T.load_golden(name)
        whole, _, _ = decode_pieces(gpu, [(v, I16)])
        assert got == whole


def test_device_resident_rows_uniform_and_batch_equal_the_float_submission(gpu):
    F32, I16 = FMT()
    import nfclab_amd
    streams, n = 64, 1 << 18
    rows = np.stack([T.synthetic_stream_i16(s, n) for s in range(streams)])

    def collect(first):
        out = [gpu.poll(first + s, capacity=8192) for s in range(streams)]
        for s in range(streams):
            gpu.close_stream(first + s)
        return out

    # the float submission of the converted rows
    keep_f, ptr_f = device_copy(to_float(rows).reshape(streams, n))
    first = gpu.open(count=streams)
    gpu.submit_uniform(first, streams, ptr_f, n * 4, n, FS, stride=1, location=nfclab_amd.LOC_DEVICE)
    want = collect(first)
    del keep_f
    assert sum(len(data_frames(f)) for f in want) > streams

    # one int16 tensor, uniform pitch
    keep_u, ptr_u = device_copy(rows)
    first = gpu.open(count=streams)
    gpu.submit_uniform(first, streams, ptr_u, n * 2, n, FS, stride=1, location=nfclab_amd.LOC_DEVICE, fmt=I16)
    got = collect(first)
    del keep_u
    assert got == want

    # per-stream pointers, each an odd number of samples into a larger buffer
    room = n + 64
    big = np.zeros(streams * room, dtype=np.int16)
    offsets = [s * room + 2 * (s % 16) + 1 for s in range(streams)]
    for s, at in enumerate(offsets):
        assert at & 1 and at + n <= (s + 1) * room
        big[at:at + n] = rows[s]
    keep_b, ptr_b = device_copy(big)
    first = gpu.open(count=streams)
    gpu.submit_batch([first + s for s in range(streams)], [ptr_b + 2 * at for at in offsets], [n] * streams, FS, stride=1,
                     location=nfclab_amd.LOC_DEVICE, fmt=I16)
    got = collect(first)
    del keep_b
    assert got == want


def iq_turning(name):
    """tests/test_replay_pipeline.py::_iq_wav: the capture as I/Q with the phase turning once per 5000 samples, rounded to int16"""
    m = T.load_fixture_i16(name).astype(np.float64)
    m = m[:m.size // 8 * 8]
    phase = 2 * np.pi * np.arange(m.size) / 5000.0
    iq = np.empty(2 * m.size, np.int16)
    iq[0::2] = np.clip(np.rint(m * np.cos(phase)), -32768, 32767)
    iq[1::2] = np.clip(np.rint(m * np.sin(phase)), -32768, 32767)
    return iq


@pytest.mark.parametrize("name", ["test_POLL_ABF_001", "test_NFC-V_26kbps_002"])
def test_int16_iq_is_converted_and_goes_through_the_magnitude_formula(gpu, name):
    F32, I16 = FMT()
    iq = iq_turning(name)
    mag = numpy_magnitude(iq)

    # nfcgpu_magnitude_fmt: the device's conversion and formula, bit for bit (this ties the device loader to
    # tests/test_sample_loader.py, which checks the same header against numpy on the host)
    got_mag = gpu.magnitude(iq, fmt=I16)
    assert np.array_equal(got_mag.view(np.uint32), mag.view(np.uint32))
    assert np.array_equal(gpu.magnitude(to_float(iq)).view(np.uint32), mag.view(np.uint32))
    if T.reference_lib() is not None:
        floats = to_float(iq)
        ref_mag = np.empty(iq.size // 2, np.float32)
        T.reference_lib().nfcref_magnitude(floats.ctypes.data, iq.size // 2, ref_mag.ctypes.data)
        assert np.array_equal(got_mag.view(np.uint32), ref_mag.view(np.uint32))

    got, windowed, fallback = decode_pieces(gpu, [(iq, I16)], stride=2)

    # the same magnitudes as floats, on the path they take
    want, windowed_f, fallback_f = decode_pieces(gpu, [(mag, F32)])
    assert got == want
    assert (windowed, fallback) == (windowed_f, fallback_f)
    as_float_iq, _, _ = decode_pieces(gpu, [(to_float(iq), F32)], stride=2)
    assert got == as_float_iq

    if T.reference_lib() is not None:
        ref, _ = T.reference_decode(mag, keep_carrier=True)
        assert sum(f[1] in (258, 259) for f in ref) >= 4
        assert got == ref
    assert sum(f[1] in (258, 259) for f in want) >= 4


@pytest.mark.parametrize("name", ["test_POLL_ABF_001", "test_NFC-V_26kbps_002"])
def test_axis_aligned_int16_iq_reproduces_the_goldens_on_the_time_parallel_path(gpu, name):
    F32, I16 = FMT()
    v = T.load_fixture_i16(name)
    assert v.min() > -32768
    for axis in range(4):
        iq = np.zeros(2 * v.size, dtype=np.int16)
        iq[axis & 1::2] = v if axis < 2 else -v  # I = v, Q = v, I = -v, Q = -v
        got, windowed, fallback = decode_pieces(gpu, [(iq, I16)], stride=2)
        assert data_frames(got) == T.load_golden(name)
        _, windowed_f, fallback_f = decode_pieces(gpu, [(T.load_fixture(name), F32)])
        print("%s axis %d: windowed %d fallback %d (float magnitudes: %d %d)" % (name, axis, windowed, fallback, windowed_f, fallback_f))
        assert (windowed, fallback) == (windowed_f, fallback_f) and windowed >= 1


def test_extreme_values_in_both_strides(gpu):
    F32, I16 = FMT()
    rng = np.random.default_rng(16)
    corner = np.array([-32768, 32767, 0, -32768, -32768, 32767, 32767, 0, 0, 1, -1, 0], dtype=np.int16)

    # I/Q through nfcgpu_magnitude_fmt
    iq = np.concatenate([corner, rng.integers(-32768, 32768, 4096).astype(np.int16), corner])
    got = gpu.magnitude(iq, fmt=I16)
    assert np.array_equal(got.view(np.uint32), gpu.magnitude(to_float(iq)).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), numpy_magnitude(iq).view(np.uint32))
    assert got[0] == np.float32(np.sqrt(np.float32(1.0) + np.float32(32767.0 / 32768.0) ** 2))

    # through a decode, short (sequential kernels) and long (offered to the time-parallel path), both strides
    base = T.load_fixture_i16("test_NFC-A_106kbps_001")
    for stride in (1, 2):
        for length in (4096, 2 * THRESHOLD):
            v = np.tile(base, 2)[:length * stride].copy()
            v[:corner.size] = corner
            v[length // 2:length // 2 + corner.size] = corner
            v[-corner.size:] = corner
            got, windowed, fallback = decode_pieces(gpu, [(v, I16)], stride=stride)
            want, windowed_f, fallback_f = decode_pieces(gpu, [(to_float(v), F32)], stride=stride)
            assert got == want
            assert (windowed, fallback) == (windowed_f, fallback_f)


def test_arguments(gpu):
    F32, I16 = FMT()
    import nfclab_amd
    lib, ctx = gpu.lib, gpu.ctx
    sid = gpu.open(count=2)
    buf = np.zeros(4096 + 8, dtype=np.int16)
    assert buf.ctypes.data % 8 == 0
    p = buf.ctypes.data
    out = np.zeros(4096, dtype=np.float32)

    def batch(ptr, stride, fmt, context=ctx):
        ids = (ctypes.c_uint32 * 1)(sid)
        ptrs = (ctypes.c_void_p * 1)(ptr)
        cnts = (ctypes.c_uint32 * 1)(64)
        b = nfclab_amd.Batch(1, stride, nfclab_amd.LOC_HOST, FS, ids, ptrs, cnts)
        return lib.nfcgpu_submit_batch_fmt(context, ctypes.byref(b), fmt)

    # an unknown format
    assert lib.nfcgpu_submit_fmt(ctx, sid, p, 64, 1, FS, 2) == EINVAL
    assert lib.nfcgpu_submit_fmt(ctx, sid, p, 64, 1, FS, 0xFFFFFFFF) == EINVAL
    assert batch(p, 1, 7) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p, 256, 64, 1, nfclab_amd.LOC_HOST, FS, 2) == EINVAL
    assert lib.nfcgpu_magnitude_fmt(ctx, p, 64, out.ctypes.data, nfclab_amd.LOC_HOST, 2) == EINVAL

    # int16 mono: an odd base address or pitch
    assert lib.nfcgpu_submit_fmt(ctx, sid, p + 1, 64, 1, FS, I16) == EINVAL
    assert batch(p + 1, 1, I16) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p + 1, 256, 64, 1, nfclab_amd.LOC_HOST, FS, I16) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p, 257, 64, 1, nfclab_amd.LOC_HOST, FS, I16) == EINVAL

    # int16 I/Q: a base or pitch that is not a multiple of 4
    assert lib.nfcgpu_submit_fmt(ctx, sid, p + 2, 64, 2, FS, I16) == EINVAL
    assert batch(p + 2, 2, I16) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p + 2, 512, 64, 2, nfclab_amd.LOC_HOST, FS, I16) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p, 514, 64, 2, nfclab_amd.LOC_HOST, FS, I16) == EINVAL
    assert lib.nfcgpu_magnitude_fmt(ctx, p + 2, 64, out.ctypes.data, nfclab_amd.LOC_HOST, I16) == EINVAL

    # a pitch shorter than a row of int16 (and one that only floats would find short is fine)
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p, 126, 64, 1, nfclab_amd.LOC_HOST, FS, I16) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(ctx, sid, 2, p, 128, 64, 1, nfclab_amd.LOC_HOST, FS, I16) == 0

    # no context
    assert lib.nfcgpu_submit_fmt(None, sid, p, 64, 1, FS, I16) == EINVAL
    assert batch(p, 1, I16, context=None) == EINVAL
    assert lib.nfcgpu_submit_uniform_fmt(None, sid, 2, p, 256, 64, 1, nfclab_amd.LOC_HOST, FS, I16) == EINVAL
    assert lib.nfcgpu_magnitude_fmt(None, p, 64, out.ctypes.data, nfclab_amd.LOC_HOST, I16) == EINVAL

    # the samples aligned to a sample are taken: mono at any even address, I/Q at any multiple of 4
    assert lib.nfcgpu_submit_fmt(ctx, sid, p + 2, 64, 1, FS, I16) == 0
    assert lib.nfcgpu_submit_fmt(ctx, sid, p + 4, 64, 2, FS, I16) == 0
    gpu.sync()
    gpu.close_stream(sid)
    gpu.close_stream(sid + 1)


@pytest.mark.parametrize("fmt_name", ["i16", "f32"])
def test_an_empty_buffer_with_a_new_sample_rate_starts_the_stream_over(gpu, fmt_name):
    """n_samples == 0 with a new sample rate re-initialises the stream (NfcDecoder.cpp:383-388), in either format: a capture
    decoded after it gives the frames of a fresh stream, numbered from sample 0"""
    F32, I16 = FMT()
    fmt = I16 if fmt_name == "i16" else F32
    name = "test_NFC-A_106kbps_002"
    v = T.load_fixture_i16(name)
    part = v if fmt == I16 else to_float(v)
    sid = gpu.open()
    gpu.submit(sid, part[:50000], FS, fmt=fmt)
    gpu.poll(sid)
    rc = gpu.lib.nfcgpu_submit_fmt(gpu.ctx, sid, part.ctypes.data, 0, 1, FS // 2, fmt)
    assert rc == 0
    rc = gpu.lib.nfcgpu_submit_fmt(gpu.ctx, sid, part.ctypes.data, 0, 1, FS, fmt)
    assert rc == 0
    gpu.submit(sid, part, FS, fmt=fmt)
    assert data_frames(gpu.poll(sid)) == T.load_golden(name)
    gpu.close_stream(sid)
