"""nfcgpu_record (float samples to the 16-bit PCM of a capture file, with the receiver's levels) and the capture files
nfcgpu_wav_write makes of it, through the C ABI.

PCM is compared bit for bit with the contract of include/nfcgpu.h as a numpy statement (quantise() below): one fp32
product with 32768, rounding toward zero, the ends of the range for what lies beyond it, 0 for NaN.

Levels are compared with a float64 evaluation of their definitions from the fp32 products (levels_yardstick()):
  peak, clipped  exact;
  power          within 64 * 2^-24 relative: no value passes through more than 60 fp32 additions on its way into the
                 sum (the first-order bound for non-negative terms), plus the product, the I*I + Q*Q addition and the
                 division;
  average        within 2048 * 2^-24 relative: the reference's own recurrence a = a * w0 + m * w1 is only guaranteed
                 2 u w0 / w1 = 1998 u, so anything inside that is as good as the reference can promise (the AGC compares
                 it with 0.05 and 0.25). The relative bound is one for non-negative m, which the inputs here are.
Bit parity with the reference's sequential fp32 sums is neither possible for a parallel form nor wanted: a numpy fp32
restatement of those sums, tried when this test was written, missed float64 by 1e-8 to 2e-4 (power) and 3e-7 to 3e-5
(average) on 4 099 and 65 536 samples, depending on the input.

The same file runs on the CPU against the emulated library (tests/test_record_emulated.py), whose twins of the kernels
compile the same arithmetic (nfc-laboratory_amd/csrc/nfc_record.hpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nfc_testlib as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(T.ROOT, "tests", "golden", "record")
EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
EINVAL = -1
LOC_HOST, LOC_DEVICE = 0, 1
SAME, MAGNITUDE = 0, 1
EPS = 2.0 ** -24
POWER_BOUND, AVERAGE_BOUND = 64 * EPS, 2048 * EPS
SEGMENT = 16384  # samples a workgroup takes (nfc_record.hpp: NfcRecordShape::kSegmentSamples)
SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 4099, 70001)  # the largest: four segments and a fifth, short one
KINDS = ((1, SAME), (2, SAME), (2, MAGNITUDE))
FS = 10000000
CANARY = 0x5A7E


def on_emulated_library():
    return "emulated" in os.path.basename(os.environ.get("NFCGPU_LIB", ""))


@pytest.fixture(scope="module")
def gpu(built):
    import nfclab_amd
    g = nfclab_amd.NfcGpu(device=0, max_streams=64)
    yield g
    g.close()


# ---------------------------------------------------------------------------------------------------------------------
# yardsticks
# ---------------------------------------------------------------------------------------------------------------------

def quantise(v):
    """(int16 PCM, which of them count as clipped) of float32 values: the statement of include/nfcgpu.h."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(v, dtype=np.float32) * np.float32(32768)
        q = np.trunc(t)
        nan = np.isnan(t)
        clipped = nan | (q < -32768) | (q > 32767)
        q = np.where(nan, 0, np.clip(q, -32768, 32767))
    return q.astype(np.int16), clipped


def channels_of(stride, mode):
    return 2 if (stride, mode) == (2, SAME) else 1


def magnitudes(gpu, buffer, stride):
    """what the levels are taken of: the input itself, or nfc_iq_magnitude of its pairs (nfcgpu_magnitude)"""
    return buffer if stride == 1 else gpu.magnitude(buffer)


def expected_pcm(gpu, buffer, stride, mode):
    return quantise(magnitudes(gpu, buffer, stride) if mode == MAGNITUDE else buffer)


def levels_yardstick(gpu, buffer, stride, mode):
    """(power, average, peak, clipped) of one buffer in float64, from the fp32 products"""
    n = buffer.size // stride
    with np.errstate(over="ignore", invalid="ignore"):
        squares = (buffer * buffer).astype(np.float64)
    power = (squares.sum() if stride == 1 else (squares[0::2] + squares[1::2]).sum()) / n
    m = magnitudes(gpu, buffer, stride)
    w1 = float(np.float32(0.001))
    w0 = float(np.float32(1) - np.float32(0.001))
    a = 0.0
    for v in m[::4].astype(np.float64):
        a = a * w0 + v * w1
    seen = m[~np.isnan(m)]
    peak = float(seen.max()) if seen.size else 0.0
    return power, a, peak, int(expected_pcm(gpu, buffer, stride, mode)[1].sum())


def check_levels(gpu, got, buffer, stride, mode, what=""):
    power, average, peak, clipped = levels_yardstick(gpu, buffer, stride, mode)
    errors = [abs(float(got[k]) - want) / want if want else abs(float(got[k])) for k, want in (("power", power), ("average", average))]
    print("%s n %d stride %d mode %d: power off by %.2f, average by %.2f units of 2^-24" % (what, buffer.size // stride, stride, mode,
                                                                                            errors[0] / EPS, errors[1] / EPS))
    assert float(got["peak"]) == peak and int(got["clipped"]) == clipped
    assert errors[0] <= POWER_BOUND and errors[1] <= AVERAGE_BOUND


def make_input(kind, n, stride, seed, n_buffers=1):
    """[n_buffers, n * stride] float32; magnitudes (mono) are non-negative"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "constant":
        m = np.full((n_buffers, n), 0.37)
    elif kind == "ramp":
        m = np.tile(t / max(n, 1) * 0.9, (n_buffers, 1)) + 0.01 * np.arange(n_buffers)[:, None]
    elif kind == "burst":
        m = np.full((n_buffers, n), 0.002)
        m[:, n // 2 - n // 16:n // 2 + n // 16] = 0.8
    elif kind == "noise":
        m = np.abs(0.3 + 0.2 * rng.standard_normal((n_buffers, n)))
    else:
        raise ValueError(kind)
    if stride == 1:
        return np.ascontiguousarray(m.astype(np.float32))
    phase = rng.uniform(0, 2 * np.pi, (n_buffers, n)) if kind == "noise" else 0.001 * t[None, :] + 0.7
    return np.ascontiguousarray(np.stack([m * np.cos(phase), m * np.sin(phase)], axis=-1).reshape(n_buffers, 2 * n).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. PCM values
# ---------------------------------------------------------------------------------------------------------------------

def test_every_grid_value_comes_back(gpu):
    k = np.arange(-32768, 32768)
    x = (k / 32768.0).astype(np.float32)[None]
    pcm, levels = gpu.record(x)
    assert np.array_equal(pcm[0], k) and int(levels["clipped"][0]) == 0
    # a left inverse of the int16 loader
    assert np.array_equal(gpu.record((pcm.astype(np.float32) / np.float32(32768)))[0], pcm)


def near_integers():
    k = np.array([-32769, -32768, -32767, -1000, -2, -1, 0, 1, 2, 1000, 32766, 32767, 32768], dtype=np.float64)
    d = np.array([-0.75, -0.5, -0.25, -2.0 ** -9, 0, 2.0 ** -9, 0.25, 0.5, 0.75])
    return ((k[:, None] + d[None, :]) / 32768.0).reshape(-1).astype(np.float32)


def test_values_beside_integers_are_truncated_not_floored(gpu):
    x = near_integers()
    pcm, levels = gpu.record(x[None])
    want, clipped = quantise(x)
    assert np.array_equal(pcm[0], want) and int(levels["clipped"][0]) == int(clipped.sum())
    assert clipped.sum() > 0 and (~clipped).sum() > 80
    assert gpu.record(np.array([[-0.5 / 32768, 0.5 / 32768, -1.5 / 32768]], dtype=np.float32))[0].tolist() == [[0, 0, -1]]


SPECIAL = np.array([1.0, -1.0, -1.00003, 0.99999, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e30, -1e30, np.inf, -np.inf, np.nan, 32767.5 / 32768,
                    -32768.5 / 32768, -32769.0 / 32768, 2.5], dtype=np.float32)


def test_special_values_saturate_and_are_counted(gpu):
    pcm, levels = gpu.record(SPECIAL[None])
    want, clipped = quantise(SPECIAL)
    assert np.array_equal(pcm[0], want)
    assert want[:4].tolist() == [32767, -32768, -32768, 32767] and want[9:14].tolist() == [32767, -32768, 32767, -32768, 0]
    assert int(levels["clipped"][0]) == int(clipped.sum()) == 8  # 1.0, +-1e30, +-inf, NaN, -32769 / 32768, 2.5
    assert float(levels["peak"][0]) == np.inf  # NaN ignored


def test_the_components_of_iq_go_through_independently(gpu):
    x = np.concatenate([SPECIAL, near_integers()])
    iq = np.stack([x, x[::-1]], axis=-1).reshape(1, -1)
    pcm, levels = gpu.record(iq, stride=2, mode=SAME)
    want, clipped = quantise(iq[0])
    assert pcm.shape == (1, 2 * x.size) and np.array_equal(pcm[0], want)
    assert int(levels["clipped"][0]) == int(clipped.sum())


def test_magnitude_mode_quantises_the_decoders_magnitude(gpu):
    rng = np.random.default_rng(5)
    iq = (0.5 * rng.standard_normal((2, 2 * 5001))).astype(np.float32)
    iq[0, :8] = [1.0, 0.0, 0.8, 0.8, np.nan, 0.1, 1e30, 1e30]  # magnitudes of 1, beyond 1, NaN and inf
    pcm, levels = gpu.record(iq, stride=2, mode=MAGNITUDE)
    for b in range(2):
        want, clipped = quantise(gpu.magnitude(iq[b]))
        assert np.array_equal(pcm[b], want) and int(levels["clipped"][b]) == int(clipped.sum())
    assert pcm[0, :4].tolist() == [32767, 32767, 0, 32767] and int(levels["clipped"][0]) >= 4


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes, pitches, locations
# ---------------------------------------------------------------------------------------------------------------------

class DeviceArray:
    """A numpy array's bytes in device memory. With the emulated library device memory is host memory."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        if on_emulated_library():
            self.tensor = None
            self.copy = self.host.copy()
            self.ptr = self.copy.ctypes.data
        else:
            import torch
            self.tensor = torch.from_numpy(self.host.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            self.ptr = self.tensor.data_ptr()

    def read(self):
        if self.tensor is None:
            return self.copy
        import torch
        torch.cuda.synchronize()
        return self.tensor.cpu().numpy().view(self.host.dtype).reshape(self.host.shape)


def raw_call(gpu, x, in_pitch, n_buffers, n, stride, mode, out, out_pitch, levels, location=LOC_HOST):
    as_ptr = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data
    return gpu.lib.nfcgpu_record(gpu.ctx, as_ptr(x), in_pitch, n_buffers, n, stride, mode, as_ptr(out), out_pitch, as_ptr(levels), location)


@pytest.mark.parametrize("n_buffers", [1, 3])
@pytest.mark.parametrize("stride,mode", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_shapes_pitches_and_locations(gpu, n, stride, mode, n_buffers):
    import nfclab_amd
    ch = channels_of(stride, mode)
    dense = make_input("noise", n, stride, 1000 * n + 10 * stride + mode, n_buffers) * np.float32(2.5)  # some of it clips
    # rows one sample apart from dense: odd mono rows start on a 2-byte boundary and no better; input rows padded with NaN
    in_row = (n + 3) * stride
    x = np.full((n_buffers, in_row), np.nan, dtype=np.float32)
    x[:, :n * stride] = dense
    out_row = (n + 1) * ch
    out = np.full((n_buffers, out_row), CANARY, dtype=np.int16)
    levels = np.zeros(n_buffers, dtype=nfclab_amd.LEVELS_DTYPE)
    assert raw_call(gpu, x, in_row * 4, n_buffers, n, stride, mode, out, out_row * 2, levels) == 0
    for b in range(n_buffers):
        want, clipped = expected_pcm(gpu, dense[b], stride, mode)
        assert np.array_equal(out[b, :n * ch], want), b
        assert int(levels["clipped"][b]) == int(clipped.sum())
        check_levels(gpu, levels[b], dense[b], stride, mode, "buffer %d" % b)
    assert (out[:, n * ch:] == CANARY).all()

    # the same on device memory
    dx, dout, dlevels = DeviceArray(x), DeviceArray(np.full((n_buffers, out_row), CANARY, dtype=np.int16)), DeviceArray(np.zeros_like(levels))
    gpu.record_device(dx.ptr, in_row * 4, n_buffers, n, dout.ptr, out_row * 2, stride=stride, mode=mode, levels_ptr=dlevels.ptr)
    assert np.array_equal(dout.read(), out)
    assert dlevels.read().tobytes() == levels.tobytes()

    # a second call, each buffer alone (dense rows, which lie differently), and without levels
    again_pcm, again_levels = gpu.record(dense, stride=stride, mode=mode)
    assert np.array_equal(again_pcm, out[:, :n * ch]) and again_levels.tobytes() == levels.tobytes()
    for b in range(n_buffers):
        alone_pcm, alone_levels = gpu.record(dense[b:b + 1], stride=stride, mode=mode)
        assert np.array_equal(alone_pcm[0], out[b, :n * ch]) and alone_levels.tobytes() == levels[b:b + 1].tobytes(), b
    bare = np.full((n_buffers, out_row), CANARY, dtype=np.int16)
    assert raw_call(gpu, x, in_row * 4, n_buffers, n, stride, mode, bare, out_row * 2, None) == 0
    assert np.array_equal(bare, out)


@pytest.mark.parametrize("stride,mode", KINDS)
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5])
def test_rows_at_every_offset_from_a_word_boundary(gpu, shift, stride, mode):
    """PCM rows that start `shift` PCM samples behind an aligned address, in device memory, over a segment boundary"""
    import nfclab_amd
    ch = channels_of(stride, mode)
    n = 2 * SEGMENT + 1
    dense = make_input("noise", n, stride, 77 + shift, 2)
    want_pcm, want_levels = gpu.record(dense, stride=stride, mode=mode)
    room = n + 11
    dx, dout = DeviceArray(dense), DeviceArray(np.full((2, room * ch), CANARY, dtype=np.int16))
    dlevels = DeviceArray(np.zeros(2, dtype=nfclab_amd.LEVELS_DTYPE))
    gpu.record_device(dx.ptr, n * stride * 4, 2, n, dout.ptr + shift * ch * 2, room * ch * 2, stride=stride, mode=mode, levels_ptr=dlevels.ptr)
    got = dout.read()
    assert np.array_equal(got[:, shift * ch:(shift + n) * ch], want_pcm)
    assert (got[:, :shift * ch] == CANARY).all() and (got[:, (shift + n) * ch:] == CANARY).all()
    assert dlevels.read().tobytes() == want_levels.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. levels
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride,mode", KINDS)
@pytest.mark.parametrize("kind", ["constant", "ramp", "burst", "noise"])
@pytest.mark.parametrize("n", [4099, 70001])
def test_levels_against_their_definitions(gpu, n, kind, stride, mode):
    x = make_input(kind, n, stride, 31 * n + stride, 2)
    _, levels = gpu.record(x, stride=stride, mode=mode)
    for b in range(2):
        check_levels(gpu, levels[b], x[b], stride, mode, kind)
    if kind == "ramp":
        # restarted per buffer: the second buffer is the first plus 0.01 and nothing else
        assert 0.005 < float(levels["average"][1]) - float(levels["average"][0]) < 0.011


def test_the_average_takes_every_fourth_sample_from_the_first(gpu):
    n = 4099
    x = make_input("ramp", n, 1, 3)
    base = gpu.record(x)[1]
    y = x.copy()
    y[0, 1::4] = 1.0
    y[0, 2::4] = 0.9
    y[0, 3::4] = 0.8
    moved = gpu.record(y)[1]
    assert moved["average"].tobytes() == base["average"].tobytes() and float(moved["power"][0]) > float(base["power"][0])
    z = x.copy()
    z[0, 4096] = 0.0  # the last sample the average reads (n is no multiple of 4: ceil(n / 4) of them), about 0.9 * 0.001 of it
    assert float(gpu.record(z)[1]["average"][0]) < float(base["average"][0]) - 0.0008
    pair = np.concatenate([x, x])
    both = gpu.record(pair)[1]
    assert both[0].tobytes() == both[1].tobytes() == base[0].tobytes()


def test_peak_is_the_largest_value_nans_aside(gpu):
    x = np.array([[-0.5, -0.25, np.nan, -0.75], [np.nan] * 4, [-0.0, 0.0, -0.0, 0.0]], dtype=np.float32)
    levels = gpu.record(x)[1]
    assert levels["peak"].tolist() == [-0.25, 0.0, 0.0] and levels["clipped"].tolist() == [1, 4, 0]
    assert np.isnan(levels["power"][1]) and not np.signbit(levels["peak"][2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------

def refusals():
    """(what, changes to the call, the word nfcgpu_last_error must carry)"""
    return [("stride 0", {"stride": 0}, "stride"),
            ("stride 3", {"stride": 3}, "stride"),
            ("magnitude of mono", {"stride": 1, "mode": MAGNITUDE}, "stride 2"),
            ("unknown mode", {"mode": 2}, "mode"),
            ("unknown location", {"location": 2}, "location"),
            ("in not aligned to a pair", {"in_shift": 4}, "in is"),
            ("out not aligned to a pair", {"mode": SAME, "out_shift": 2}, "out is"),
            ("mono out on an odd byte", {"mode": MAGNITUDE, "out_shift": 1}, "out is"),
            ("in pitch not a multiple of a pair", {"in_pitch": 64 * 8 + 4}, "in_pitch_bytes"),
            ("out pitch not a multiple of a pair", {"mode": SAME, "out_pitch": 64 * 4 + 2}, "out_pitch_bytes"),
            ("out pitch smaller than the row", {"mode": SAME, "out_pitch": 64 * 4 - 4}, "out_pitch_bytes"),
            ("mono out pitch smaller than the row", {"mode": MAGNITUDE, "out_pitch": 64 * 2 - 2}, "out_pitch_bytes"),
            ("in NULL", {"in_null": True}, "in is"),
            ("out NULL", {"out_null": True}, "out is")]


@pytest.mark.parametrize("what,call,word", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_return_their_code_and_write_nothing(gpu, what, call, word):
    import nfclab_amd
    n, nb = 64, 2
    x = make_input("noise", n + 4, 2, 9, nb)
    out = np.full((nb, 2 * n + 16), CANARY, dtype=np.int16)
    levels = np.full(nb, 7, dtype=np.uint32).repeat(4).view(nfclab_amd.LEVELS_DTYPE)
    before = levels.tobytes()
    stride, mode = call.get("stride", 2), call.get("mode", MAGNITUDE)
    xp = None if call.get("in_null") else x.ctypes.data + call.get("in_shift", 0)
    op = None if call.get("out_null") else out.ctypes.data + call.get("out_shift", 0)
    rc = raw_call(gpu, xp, call.get("in_pitch", (n + 4) * 8), nb, n, stride, mode, op, call.get("out_pitch", (2 * n + 16) * 2), levels,
                  call.get("location", LOC_HOST))
    assert rc == EINVAL
    assert (out == CANARY).all() and levels.tobytes() == before
    assert word in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()


def test_a_null_context_is_refused():
    import nfclab_amd
    lib = nfclab_amd.load_library()
    x, out = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.int16)
    assert lib.nfcgpu_record(None, x.ctypes.data, 32, 1, 8, 1, SAME, out.ctypes.data, 16, None, LOC_HOST) == EINVAL


def test_empty_calls_succeed_and_write_no_pcm(gpu):
    import nfclab_amd
    x = make_input("noise", 16, 2, 1, 2)
    out = np.full((2, 40), CANARY, dtype=np.int16)
    levels = np.full(2, 7, dtype=np.uint32).repeat(4).view(nfclab_amd.LEVELS_DTYPE)
    before = levels.tobytes()
    assert raw_call(gpu, x, 128, 0, 16, 2, SAME, out, 80, levels) == 0
    assert (out == CANARY).all() and levels.tobytes() == before
    assert raw_call(gpu, x, 128, 2, 0, 2, MAGNITUDE, out, 0, levels) == 0
    assert (out == CANARY).all() and levels.tobytes() == bytes(32)
    dlevels = DeviceArray(np.full(8, 7, dtype=np.uint32))
    dx, dout = DeviceArray(x), DeviceArray(out)
    gpu.record_device(dx.ptr, 128, 2, 0, dout.ptr, 80, stride=1, levels_ptr=dlevels.ptr)
    assert not dlevels.read().any() and (dout.read() == CANARY).all()
    pcm, lv = gpu.record(np.zeros((3, 0), dtype=np.float32))
    assert pcm.shape == (3, 0) and lv.tobytes() == bytes(48)


# ---------------------------------------------------------------------------------------------------------------------
# 5. against the reference's writer
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_a_recording_is_the_file_the_reference_writes(gpu, channels, tmp_path):
    """tests/golden/record/{mono,iq}.wav: what hw::RecordDevice wrote of tests/golden/record/input.f32 through
    tests/dropin/record_harness.cpp (tests/golden/record/README.md), every byte but the epoch (48-51, the time of writing)."""
    import nfclab_amd
    x = np.fromfile(os.path.join(GOLDEN, "input.f32"), dtype=np.float32)
    assert x.size == 8192 and np.isfinite(x).all()
    with open(os.path.join(GOLDEN, "mono.wav" if channels == 1 else "iq.wav"), "rb") as f:
        want = f.read()
    pcm, levels = gpu.record(x[None], stride=channels, mode=SAME)
    assert int(levels["clipped"][0]) == 0
    samples = pcm[0].reshape(-1, channels)
    epoch = int.from_bytes(want[48:52], "little")

    whole = str(tmp_path / "whole.wav")
    nfclab_amd.wav_write(whole, samples, FS, channels=channels, stream_time=epoch)
    with open(whole, "rb") as f:
        assert f.read() == want
    nfclab_amd.wav_write(whole, samples, FS, channels=channels)
    with open(whole, "rb") as f:
        got = f.read()
    assert got[:48] == want[:48] and got[48:52] == bytes(4) and got[52:] == want[52:]

    pieces = str(tmp_path / "pieces.wav")
    nfclab_amd.wav_write(pieces, samples[:1000], FS, channels=channels, stream_time=epoch)
    nfclab_amd.wav_append(pieces, samples[1000:1024])
    nfclab_amd.wav_append(pieces, samples[1024:])
    with open(pieces, "rb") as f:
        assert f.read() == want


# ---------------------------------------------------------------------------------------------------------------------
# 6. decoding a recording
# ---------------------------------------------------------------------------------------------------------------------

def data_frames(frames):
    return [f for f in frames if f[1] in (0x102, 0x103)]


def record_and_decode(gpu, iq):
    """the live flow on the device: float I/Q -> nfcgpu_record (MAGNITUDE) -> nfcgpu_submit_uniform_fmt (I16) of the recording;
    returns (PCM, levels, frames, windowed_streams)"""
    import nfclab_amd
    n = iq.size // 2
    dx, dout = DeviceArray(iq), DeviceArray(np.zeros(n, dtype=np.int16))
    dlevels = DeviceArray(np.zeros(1, dtype=nfclab_amd.LEVELS_DTYPE))
    gpu.record_device(dx.ptr, n * 8, 1, n, dout.ptr, n * 2, stride=2, mode=MAGNITUDE, levels_ptr=dlevels.ptr)
    sid = gpu.open()
    gpu.sync()
    gpu.stats_reset()
    gpu.submit_uniform(sid, 1, dout.ptr, n * 2, n, FS, stride=1, location=LOC_DEVICE, fmt=nfclab_amd.FMT_I16)
    frames = gpu.poll(sid)
    windowed = int(gpu.stats().windowed_streams)
    gpu.close_stream(sid)
    return dout.read().copy(), dlevels.read().copy(), frames, windowed


@pytest.mark.parametrize("name", ["test_NFC-A_106kbps_001", "test_POLL_ABF_001"])
def test_recording_a_capture_gives_the_capture_and_its_frames(gpu, name):
    """T.magnitude_to_iq puts every sample on an axis, so the magnitude of the I/Q is exactly |sample|: the recording is the
    capture's int16, but for the few samples below zero both captures hold (an I/Q magnitude has no sign), which come back as
    their absolute values - the magnitudes the decoder forms of this I/Q itself."""
    v = T.load_fixture_i16(name).astype(np.int32)
    assert np.count_nonzero(v < 0) < v.size // 1000
    iq = T.magnitude_to_iq(T.load_fixture(name), seed=3)
    pcm, levels, frames, _ = record_and_decode(gpu, iq)
    assert np.array_equal(pcm, np.abs(v)) and np.array_equal(pcm[v >= 0], v[v >= 0]) and int(levels["clipped"][0]) == 0
    assert data_frames(frames) == T.load_golden(name)


@pytest.mark.skipif(T.reference_lib() is None, reason="oracle/_ref not built")
def test_decoding_a_recording_of_off_grid_floats_gives_the_frames_of_the_recording(gpu):
    """The yardstick is the reference on the recorded values, never on the floats: the recording is what a replay would read."""
    name = "test_NFC-A_106kbps_001"
    mag = T.load_fixture(name)
    rng = np.random.default_rng(20261018)
    noisy = np.abs(mag * np.float32(0.83) + (0.002 * rng.standard_normal(mag.size)).astype(np.float32)).astype(np.float32)
    assert noisy.size >= 32768
    turn = rng.uniform(0, 2 * np.pi, noisy.size)
    iq = np.stack([noisy * np.cos(turn), noisy * np.sin(turn)], axis=-1).astype(np.float32).reshape(-1)
    pcm, levels, frames, windowed = record_and_decode(gpu, iq)
    assert np.array_equal(pcm, quantise(gpu.magnitude(iq))[0])
    off_grid = np.count_nonzero(gpu.magnitude(iq) * np.float32(32768) != pcm)
    assert off_grid > pcm.size // 2
    want, _ = T.reference_decode(pcm.astype(np.float32) / np.float32(32768))
    assert data_frames(frames) == want and len(want) > 0
    assert windowed == 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. the CPU twin of the emulated library and the device kernels
# ---------------------------------------------------------------------------------------------------------------------

def twin_cases():
    return [(n, stride, mode, kind) for n in (5, 1023, 70001) for stride, mode in KINDS for kind in ("noise", "burst")]


def twin_input(n, stride, mode, kind):
    x = make_input(kind, n, stride, 7 * n + stride + mode, 2) * np.float32(1.7)
    x[1, :min(3, x.shape[1])] = [np.nan, 3.0, -3.0][:min(3, x.shape[1])]
    return x


def dump_outputs(path):
    """Child process (NFCGPU_LIB names the library): PCM and levels of twin_cases(), in order, to one file."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    pcm, levels = [], []
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for n, stride, mode, kind in twin_cases():
            p, lv = g.record(twin_input(n, stride, mode, kind), stride=stride, mode=mode)
            pcm.append(p.reshape(-1))
            levels.append(lv)
    np.savez(path, pcm=np.concatenate(pcm), levels=np.concatenate(levels))


def test_twin_equals_device(gpu, tmp_path):
    """PCM, peak and clipped are bit-equal between the emulated library's twins and the device kernels; power and average of
    both lie inside the bounds above (they are built to take the same operations in the same order, which is not asserted)."""
    if on_emulated_library():
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
    device, twin = outputs["device"], outputs["twin"]
    assert np.array_equal(device["pcm"], twin["pcm"])
    for key in ("peak", "clipped"):
        assert device["levels"][key].tobytes() == twin["levels"][key].tobytes(), key
    at = 0
    for n, stride, mode, kind in twin_cases():
        x = twin_input(n, stride, mode, kind)
        for b in range(2):
            if not np.isnan(x[b]).any():
                check_levels(gpu, device["levels"][at + b], x[b], stride, mode, "device")
                check_levels(gpu, twin["levels"][at + b], x[b], stride, mode, "twin")
        at += 2
    same = sum(device["levels"][k].tobytes() == twin["levels"][k].tobytes() for k in ("power", "average"))
    print("power and average bit-equal between twin and device: %d of 2 columns" % same)


def write_wavs(directory):
    """Child process (NFCGPU_LIB names the emulated library): two fixtures as float magnitudes, recorded and written with
    nfcgpu_wav_write, for the reference's reader (tests/test_record_emulated.py)."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for name in sys.argv[3:]:
            pcm, levels = g.record(T.load_fixture(name)[None])
            assert int(levels["clipped"][0]) == 0
            nfclab_amd.wav_write(os.path.join(directory, name + ".wav"), pcm[0], FS, stream_time=1700000000)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump_outputs(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--write-wavs":
        write_wavs(sys.argv[2])
    else:
        sys.exit("usage: test_record.py --dump OUT.npz | --write-wavs DIR NAME...")
