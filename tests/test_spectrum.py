"""nfcgpu_spectrum (the spectrum the reference's FourierProcessTask publishes on "signal.fft", for every frame of every
buffer) through the C ABI. The yardstick for values is the contract of include/nfcgpu.h evaluated by numpy in float64
inside this file: window tables by the reference's expressions in the reference's types, the gather
s(m) = 4 D (m >> 2) + (m & 3), one fp32 product with the window, numpy.fft.fft in complex128, abs, swap of halves.

The bound on values is T * 2^-24 * (largest bin of the frame), T read from tests/golden/spectrum/tolerance.json: four
times what the reference's own FFT (its vendored mufft, built the way the reference builds it) misses the same
yardstick by on the same inputs; one T per length. See tests/golden/spectrum/README.md for how both recordings under
that directory were made.

The same file runs on the CPU against the emulated library (tests/test_spectrum_emulated.py), whose twin of the kernel
compiles the same arithmetic (nfc-laboratory_amd/csrc/nfc_spectrum.hpp)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nfc_testlib as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(T.ROOT, "tests", "golden", "spectrum")
EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
WINDOWS = ("none", "hamming", "hann")
KINDS = ("noise", "int16", "carrier", "constant", "zeros")
EINVAL = -1
LOC_HOST, LOC_DEVICE = 0, 1
EPS = 2.0 ** -24


def tolerance(length):
    with open(os.path.join(GOLDEN, "tolerance.json")) as f:
        return float(json.load(f)["T"][str(length)])


def on_emulated_library():
    return "emulated" in os.path.basename(os.environ.get("NFCGPU_LIB", ""))


@pytest.fixture(scope="module")
def gpu(built):
    import nfclab_amd
    g = nfclab_amd.NfcGpu(device=0, max_streams=64)
    yield g
    g.close()


# ---------------------------------------------------------------------------------------------------------------------
# inputs and yardstick
# ---------------------------------------------------------------------------------------------------------------------

def make_input(kind, n_pairs, seed, n_buffers=1):
    """[n_buffers, n_pairs, 2] float32 from numpy.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    shape = (n_buffers, n_pairs)
    if kind == "noise":
        z = 0.25 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    elif kind == "int16":
        # what capture files hold
        z = np.round(rng.uniform(-1, 1, shape) * 32768) / 32768 + 1j * np.round(rng.uniform(-1, 1, shape) * 32768) / 32768
    elif kind == "carrier":
        # a carrier off every bin of every length and decimation used here, 10 % ASK, noise at 1e-3
        f = rng.uniform(-0.4, 0.4, (n_buffers, 1))
        n = np.arange(n_pairs)[None, :]
        ask = 1.0 - 0.1 * ((n // rng.integers(40, 400, (n_buffers, 1))) & 1)
        z = 0.6 * ask * np.exp(2j * np.pi * (f * n + rng.uniform(0, 1, (n_buffers, 1))))
        z = z + 1e-3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    elif kind == "constant":
        # the peak bin far above the rest
        z = (0.5 + 0.5j) + 1e-4 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    elif kind == "zeros":
        z = np.zeros(shape, dtype=np.complex128)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1).astype(np.float32))


def window_table(name, length):
    """The reference's tables under the reference's names (FourierProcessTask.cpp:121-143), in the reference's types."""
    n = np.arange(length)
    if name == "hamming":
        # float(pow(sin(float(M_PI * n / L)), 2)): sine of a float in float, its square in double
        s = np.sin((np.pi * n / length).astype(np.float32)).astype(np.float32)
        return (s.astype(np.float64) ** 2).astype(np.float32)
    if name == "hann":
        return (0.5 * (1.0 - np.cos((2.0 * np.pi * n) / (length - 1)))).astype(np.float32)
    assert name == "none"
    return np.ones(length, dtype=np.float32)


def source_pairs(length, decimation):
    m = np.arange(length)
    return 4 * decimation * (m >> 2) + (m & 3)


def windowed_frame(buffer, length, window, decimation, start=0):
    """What enters the FFT: [length, 2] float32, the gathered pairs times the window, one fp32 product each."""
    x = buffer[start + source_pairs(length, decimation)]
    return (x * window_table(window, length)[:, None]).astype(np.float32)


def yardstick(buffer, length, window, decimation, start=0):
    x = windowed_frame(buffer, length, window, decimation, start).astype(np.float64)
    return np.fft.fftshift(np.abs(np.fft.fft(x[:, 0] + 1j * x[:, 1])))


def seed_of(kind, length, window, decimation):
    return 1000003 * KINDS.index(kind) + 1009 * length + 17 * WINDOWS.index(window) + decimation


def value_cases(lengths, kinds):
    return [(length, window, decimation, kind) for length in lengths for window in WINDOWS for decimation in (1, 16) for kind in kinds]


VALUE_BUFFERS = 4


def value_input(length, window, decimation, kind):
    return make_input(kind, length * decimation, seed_of(kind, length, window, decimation), VALUE_BUFFERS)


def check_values(gpu, length, window, decimation, kind):
    buffers = value_input(length, window, decimation, kind)
    got = gpu.spectrum(buffers, length=length, window=window, decimation=decimation)
    assert got.shape == (VALUE_BUFFERS, 1, length) and got.dtype == np.float32
    t = tolerance(length)
    worst = 0.0
    for b in range(VALUE_BUFFERS):
        want = yardstick(buffers[b], length, window, decimation)
        if kind == "zeros":
            assert not got[b, 0].view(np.uint32).any()
            continue
        error = np.max(np.abs(got[b, 0].astype(np.float64) - want)) / (EPS * want.max())
        worst = max(worst, error)
    print("L %d %s D %d %s: worst error %.2f units of 2^-24 * peak, T = %.2f" % (length, window, decimation, kind, worst, t))
    assert worst <= t


# ---------------------------------------------------------------------------------------------------------------------
# 1. values, 4. other lengths
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length,window,decimation,kind", value_cases([1024], KINDS))
def test_values(gpu, length, window, decimation, kind):
    check_values(gpu, length, window, decimation, kind)


@pytest.mark.parametrize("length,window,decimation,kind", value_cases([256, 512, 2048, 4096], ("noise", "int16")))
def test_values_other_lengths(gpu, length, window, decimation, kind):
    check_values(gpu, length, window, decimation, kind)


# ---------------------------------------------------------------------------------------------------------------------
# 2. structure
# ---------------------------------------------------------------------------------------------------------------------

def impulse_bound(length):
    """An impulse meets at most one rounded unit-modulus twiddle per pass, each product moves the modulus by at most about
    three roundings, and the magnitude adds two: a derived bound, relative."""
    return (3 * np.log2(length) + 2) * EPS


@pytest.mark.parametrize("k0", [5, 200, 511, -7, -300, -512])
def test_a_tone_on_a_bin_peaks_at_its_shifted_index(gpu, k0):
    L = 1024
    n = np.arange(L)
    z = 0.5 * np.exp(2j * np.pi * k0 * n / L)
    x = np.stack([z.real, z.imag], axis=-1).astype(np.float32)[None]
    got = gpu.spectrum(x, length=L, window="none", decimation=1)[0, 0]
    assert int(np.argmax(got)) == (k0 + L // 2) % L
    assert abs(got.max() - 0.5 * L) <= 1e-4 * L


def test_conjugating_the_input_mirrors_the_output(gpu):
    L = 1024
    x = make_input("noise", L, 77)
    y = x.copy()
    y[..., 1] = -y[..., 1]
    a = gpu.spectrum(x, length=L, window="none", decimation=1)[0, 0].astype(np.float64)
    b = gpu.spectrum(y, length=L, window="none", decimation=1)[0, 0].astype(np.float64)
    mirrored = a[(L - np.arange(L)) % L]
    assert np.max(np.abs(b - mirrored)) <= tolerance(L) * EPS * a.max()


@pytest.mark.parametrize("length", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("a", [0.7, -0.3])
def test_an_impulse_at_pair_zero_is_flat(gpu, length, a):
    x = np.zeros((1, length, 2), dtype=np.float32)
    x[0, 0, 0] = a
    got = gpu.spectrum(x, length=length, window="none", decimation=1)[0, 0].astype(np.float64)
    want = abs(float(np.float32(a)))
    assert np.max(np.abs(got - want)) <= impulse_bound(length) * want


@pytest.mark.parametrize("window", WINDOWS)
def test_an_impulse_at_a_source_pair_gives_its_window_factor(gpu, window):
    """Pins the gather (a wrong source pair gives 0) and both window formulas, including the L / L-1 difference."""
    L, D = 1024, 16
    w = window_table(window, L).astype(np.float64)
    s = source_pairs(L, D)
    for m in (0, 1, 2, 3, 4, 5, 100, 511, 512, 777, 1022, 1023):
        x = np.zeros((1, L * D, 2), dtype=np.float32)
        x[0, s[m], 0] = 1.0
        got = gpu.spectrum(x, length=L, window=window, decimation=D)[0, 0].astype(np.float64)
        assert np.max(np.abs(got - w[m])) <= impulse_bound(L) * w[m], m
    # pairs between the groups of four are not read at all
    x = np.zeros((1, L * D, 2), dtype=np.float32)
    x[0, 4:4 * D, :] = 1.0
    x[0, L * D - 4 * D + 4:, :] = 1.0
    assert not gpu.spectrum(x, length=L, window=window, decimation=D).view(np.uint32).any()


def test_decimation_derived_from_the_sample_rate(gpu):
    L = 1024
    x = make_input("noise", L * 16, 5)
    a = gpu.spectrum(x, length=L)
    assert a.shape == (1, 1, L)
    assert np.array_equal(a, gpu.spectrum(x, length=L, decimation=16))
    assert gpu.spectrum_frames(L * 8, sample_rate=5000000) == 1 and gpu.spectrum_frames(L * 8 - 1, sample_rate=5000000) == 0
    assert gpu.spectrum_frames(L, sample_rate=100000) == 1  # a rate below the bandwidth: D = 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. frames and layout
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


@pytest.mark.parametrize("decimation", [1, 16])
@pytest.mark.parametrize("hop", [0, 1, 1000, None])
def test_frame_f_is_the_single_frame_of_the_buffer_advanced_by_f_hops(gpu, hop, decimation):
    L = 1024
    span = L * decimation
    hop = span if hop is None else hop
    frames = 4 if hop else 1
    x = make_input("carrier", span + (frames - 1) * hop, 31 + decimation, 2)
    got = gpu.spectrum(x, length=L, decimation=decimation, hop=hop)
    assert got.shape == (2, frames, L)
    for f in range(frames):
        single = gpu.spectrum(x[:, f * hop:f * hop + span], length=L, decimation=decimation, hop=0)
        assert np.array_equal(got[:, f].view(np.uint32), single[:, 0].view(np.uint32)), f


@pytest.mark.parametrize("hop", [1, 1000, 16384])
def test_frame_counts_at_the_edges(gpu, hop):
    L, D = 1024, 16
    span = L * D
    x = make_input("noise", span + hop, 9)
    for n_pairs, frames in ((span - 1, 0), (span, 1), (span + hop - 1, 1), (span + hop, 2)):
        assert gpu.spectrum_frames(n_pairs, length=L, decimation=D, hop=hop) == frames
        got = gpu.spectrum(x[:, :n_pairs], length=L, decimation=D, hop=hop)
        assert got.shape == (1, frames, L)
    assert gpu.spectrum_frames(span - 1, length=L, decimation=D, hop=0) == 0
    assert gpu.spectrum_frames(span + 5 * hop, length=L, decimation=D, hop=0) == 1


PATTERN = 0x7FC0FFEE


def raw_call(gpu, x, in_pitch, n_buffers, n_pairs, params, out, out_pitch, location=LOC_HOST):
    xp = x if isinstance(x, int) else x.ctypes.data
    op = out if isinstance(out, int) else out.ctypes.data
    return gpu.lib.nfcgpu_spectrum(gpu.ctx, xp, in_pitch, n_buffers, n_pairs, ctypes.byref(params), op, out_pitch, location)


def test_pitches_larger_than_the_data_leave_the_padding_alone(gpu):
    L, D, hop, frames, nb = 1024, 1, 300, 3, 3
    n_pairs = L * D + (frames - 1) * hop
    dense = make_input("int16", n_pairs, 12, nb)
    in_pitch_pairs = n_pairs + 6
    x = np.full((nb, in_pitch_pairs, 2), np.nan, dtype=np.float32)
    x[:, :n_pairs] = dense
    out_pitch_floats = frames * L + 8
    out = np.full((nb, out_pitch_floats), PATTERN, dtype=np.uint32)
    p = gpu.spectrum_params(length=L, decimation=D, hop=hop)
    assert raw_call(gpu, x, in_pitch_pairs * 8, nb, n_pairs, p, out, out_pitch_floats * 4) == 0
    want = gpu.spectrum(dense, length=L, decimation=D, hop=hop)
    assert np.array_equal(out[:, :frames * L], want.reshape(nb, -1).view(np.uint32))
    assert (out[:, frames * L:] == PATTERN).all()

    # the same on device memory
    dx, dout = DeviceArray(x), DeviceArray(np.full((nb, out_pitch_floats), PATTERN, dtype=np.uint32))
    assert raw_call(gpu, dx.ptr, in_pitch_pairs * 8, nb, n_pairs, p, dout.ptr, out_pitch_floats * 4, LOC_DEVICE) == 0
    assert np.array_equal(dout.read(), out)


def test_one_call_for_many_frames_equals_the_single_calls(gpu):
    L, D, hop, frames, nb = 1024, 16, 777, 5, 3
    span = L * D
    x = make_input("carrier", span + (frames - 1) * hop, 44, nb)
    got = gpu.spectrum(x, length=L, decimation=D, hop=hop)
    assert got.shape == (nb, frames, L)
    for b in range(nb):
        for f in range(frames):
            single = gpu.spectrum(x[b:b + 1, f * hop:f * hop + span], length=L, decimation=D)
            assert np.array_equal(got[b, f].view(np.uint32), single[0, 0].view(np.uint32)), (b, f)


def test_host_and_device_location_give_the_same_bytes(gpu):
    L, D, hop, nb = 1024, 16, 5000, 4
    n_pairs = L * D + 2 * hop
    x = make_input("int16", n_pairs, 45, nb)
    host = gpu.spectrum(x, length=L, decimation=D, hop=hop)
    dx, dout = DeviceArray(x), DeviceArray(np.zeros((nb, 3, L), dtype=np.float32))
    assert gpu.spectrum_device(dx.ptr, n_pairs * 8, nb, n_pairs, dout.ptr, 3 * L * 4, length=L, decimation=D, hop=hop) == 3
    assert np.array_equal(dout.read().view(np.uint32), host.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 5. arguments
# ---------------------------------------------------------------------------------------------------------------------

def test_default_params(gpu):
    import nfclab_amd
    p = nfclab_amd.SpectrumParams()
    p.reserved[1] = 9
    gpu.lib.nfcgpu_spectrum_default_params(ctypes.byref(p))
    assert (p.length, p.window, p.decimation, p.hop, p.sample_rate, list(p.reserved)) == (1024, 1, 0, 0, 10000000, [0, 0, 0])
    assert ctypes.sizeof(p) == 32


def refusals():
    """(what, changes to the parameters, changes to the call, the word nfcgpu_last_error must carry)"""
    return [("length not a power of two", {"length": 1000}, {}, "length"),
            ("length too small", {"length": 128}, {}, "length"),
            ("length too large", {"length": 8192}, {}, "length"),
            ("unknown window", {"window": 3}, {}, "window"),
            ("reserved word", {"reserved": 1}, {}, "reserved"),
            ("out pitch smaller than the frames", {}, {"out_pitch": 2 * 1024 * 4 - 16}, "out_pitch_bytes"),
            ("out pitch not a multiple of 16", {}, {"out_pitch": 2 * 1024 * 4 + 8}, "out_pitch_bytes"),
            ("in pitch not a multiple of 8", {}, {"in_pitch": 2048 * 8 + 4}, "in_pitch_bytes")]


@pytest.mark.parametrize("what,params,call,word", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_return_their_code_and_write_nothing(gpu, what, params, call, word):
    L, n_pairs, nb = 1024, 2048, 2
    x = make_input("noise", n_pairs + 8, 3, nb)
    p = gpu.spectrum_params(length=L, decimation=1, hop=1024)  # two frames per buffer
    for key, value in params.items():
        if key == "reserved":
            p.reserved[2] = value
        else:
            setattr(p, key, value)
    out = np.full((nb, 2 * L + 64), PATTERN, dtype=np.uint32)
    rc = raw_call(gpu, x, call.get("in_pitch", (n_pairs + 8) * 8), nb, n_pairs, p, out, call.get("out_pitch", (2 * L + 64) * 4))
    assert rc == EINVAL
    assert (out == PATTERN).all()
    assert word in gpu.lib.nfcgpu_last_error(gpu.ctx).decode()
    if params:
        assert gpu.lib.nfcgpu_spectrum_frames(ctypes.byref(p), n_pairs) == 0


def test_zero_frames_is_success_and_writes_nothing(gpu):
    L, D = 1024, 16
    x = make_input("noise", L * D - 1, 4, 2)
    out = np.full((2, 64), PATTERN, dtype=np.uint32)
    p = gpu.spectrum_params(length=L, decimation=D, hop=100)
    assert raw_call(gpu, x, (L * D - 1) * 8, 2, L * D - 1, p, out, 0) == 0
    assert raw_call(gpu, x, (L * D - 1) * 8, 0, L * D - 1, p, out, 256) == 0
    assert (out == PATTERN).all()
    assert gpu.spectrum(x, length=L, decimation=D, hop=100).shape == (2, 0, L)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the shipped configuration against the reference's own task
# ---------------------------------------------------------------------------------------------------------------------

GOLDEN_SEEDS = (20261, 20262, 20263)
GOLDEN_PAIRS = 16384


def golden_inputs():
    """Three IQ buffers of 16 384 pairs on the int16 grid of a capture file: noise, a modulated carrier, both at once."""
    a = make_input("int16", GOLDEN_PAIRS, GOLDEN_SEEDS[0])[0] * np.float32(0.25)
    b = make_input("carrier", GOLDEN_PAIRS, GOLDEN_SEEDS[1])[0]
    c = make_input("carrier", GOLDEN_PAIRS, GOLDEN_SEEDS[2])[0] * np.float32(0.5) + make_input("noise", GOLDEN_PAIRS, GOLDEN_SEEDS[2] + 1)[0] * np.float32(0.2)
    x = np.stack([a, b, c])
    return np.ascontiguousarray((np.round(x.astype(np.float64) * 32768) / 32768).astype(np.float32))


def test_the_shipped_configuration_against_the_recorded_task(gpu):
    """tests/golden/spectrum/fourier_task.npy: what the reference's FourierProcessTask published on "signal.fft" for
    golden_inputs(), one buffer each (tests/dropin/fourier_harness.cpp; tests/golden/spectrum/README.md). The bound is the
    reference's own error plus ours, (T / 4 + T) * 2^-24 * peak."""
    recorded = np.load(os.path.join(GOLDEN, "fourier_task.npy"))
    x = golden_inputs()
    assert recorded.shape == (3, 1024) and recorded.dtype == np.float32
    got = gpu.spectrum(x)  # defaults: 1024, "hamming", decimation from 10 MS/s, one frame at pair 0
    assert got.shape == (3, 1, 1024)
    t = tolerance(1024)
    for b in range(3):
        peak = float(recorded[b].max())
        error = np.max(np.abs(got[b, 0].astype(np.float64) - recorded[b].astype(np.float64))) / (EPS * peak)
        print("buffer %d: %.2f units of 2^-24 * peak against the recorded task, bound %.2f" % (b, error, t / 4 + t))
        assert error <= t / 4 + t


# ---------------------------------------------------------------------------------------------------------------------
# 7. the CPU twin of the emulated library and the device kernel
# ---------------------------------------------------------------------------------------------------------------------

def dump_value_outputs(path):
    """Child process (NFCGPU_LIB names the library): the outputs of test 1's and test 4's inputs, in order, to one file."""
    sys.path.insert(0, os.path.join(T.ROOT, "nfc-laboratory_amd"))
    import nfclab_amd
    rows = []
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as g:
        for length, window, decimation, kind in value_cases([1024], KINDS) + value_cases([256, 512, 2048, 4096], ("noise", "int16")):
            out = g.spectrum(value_input(length, window, decimation, kind), length=length, window=window, decimation=decimation)
            rows.append(out.reshape(-1))
    np.save(path, np.concatenate(rows))


def test_twin_equals_device(built, tmp_path):
    """The emulated library's twin and the device kernel run the same fp32 operations in the same order per output (tables
    from the host, no contraction): their outputs are compared as uint32, bit for bit."""
    if on_emulated_library():
        pytest.skip("NFCGPU_LIB is the emulated library: there is no device to compare with")
    if not os.path.exists(EMU):
        pytest.skip("tests/hostsim/libnfcgpu_emulated.so is not built")
    import nfclab_amd
    outputs = {}
    for name, lib, extra in (("device", nfclab_amd.LIB_PATH, {}), ("twin", EMU, {"NFCGPU_NO_TORCH": "1"})):
        path = str(tmp_path / (name + ".npy"))
        env = dict(os.environ, NFCGPU_LIB=lib, **extra)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], cwd=T.ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-3000:]
        outputs[name] = np.load(path)
    assert outputs["device"].shape == outputs["twin"].shape
    differ = np.flatnonzero(outputs["device"].view(np.uint32) != outputs["twin"].view(np.uint32))
    assert differ.size == 0, "%d of %d outputs differ, first at %d" % (differ.size, outputs["twin"].size, differ[0])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump_value_outputs(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--golden-inputs":
        golden_inputs().tofile(sys.argv[2])  # three buffers of 16 384 float32 pairs, one after the other
    else:
        sys.exit("usage: test_spectrum.py --dump OUT.npy | --golden-inputs OUT.f32")
