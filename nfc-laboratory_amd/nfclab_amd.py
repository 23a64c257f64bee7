"""ctypes binding of libnfcgpu.so (include/nfcgpu.h) for the tests and bench.py.

This is plumbing only: the product is the C-ABI library; the reference's host language is C++ and
its drop-in host side lives in nfc-laboratory_amd/host/. Nothing here decodes on the CPU: if the
library or a GPU is missing, NfcGpu() raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFCGPU_LIB", os.path.join(HERE, "libnfcgpu.so"))

TECH_A, TECH_B, TECH_F, TECH_V = 1, 2, 4, 8
LOC_HOST, LOC_DEVICE = 0, 1
# sample formats of the decoder's input (NFCGPU_FMT_*): float32, or the little-endian int16 PCM capture files hold,
# value = v / 32768, converted by the kernels as they load
FMT_F32, FMT_I16 = 0, 1

# what nfcgpu_record writes (NFCGPU_RECORD_*): the input as it is (mono PCM, or two-channel I/Q PCM for stride 2), or the magnitude
# of stride-2 I/Q as mono PCM
RECORD_SAME, RECORD_MAGNITUDE = 0, 1
# one nfcgpu_record_levels per buffer
LEVELS_DTYPE = np.dtype([("power", np.float32), ("average", np.float32), ("peak", np.float32), ("clipped", np.uint32)])

# the planes of nfcgpu_signal_tap (NFCGPU_TAP_*), in the order they are written
TAP_VALUE, TAP_FILTERED, TAP_DEVIATION, TAP_AVERAGE, TAP_ENVELOPE, TAP_DEPTH = 1, 2, 4, 8, 16, 32
TAP_ALL = 0x3F
TAP_NAMES = ("value", "filtered", "deviation", "average", "envelope", "depth")
# one nfcgpu_tap_state per buffer
TAP_STATE_DTYPE = np.dtype([("clock", np.uint32), ("pulse_filter", np.uint32), ("envelope", np.float32), ("filter_n1", np.float32),
                            ("deviation", np.float32), ("average", np.float32), ("reserved", np.uint32, (2,))])

# nfcgpu_signal_tap_reduce: one nfcgpu_tap_range per range, one nfcgpu_tap_stat per range and selected channel
APCM_INFO_DTYPE = np.dtype([("bytes", np.uint32), ("records", np.uint32), ("wrapped", np.uint32), ("reserved", np.uint32)])
TAP_RANGE_DTYPE = np.dtype([("buffer", np.uint32), ("first", np.uint32), ("count", np.uint32), ("reserved", np.uint32)])
TAP_STAT_DTYPE = np.dtype([("min", np.float32), ("max", np.float32), ("mean", np.float32), ("valid", np.uint32), ("argmin", np.uint32),
                           ("argmax", np.uint32), ("reserved", np.uint32, (2,))])

FRAME_CARRIER_OFF, FRAME_CARRIER_ON, FRAME_POLL, FRAME_LISTEN = 0x100, 0x101, 0x102, 0x103


class Params(ctypes.Structure):
    _fields_ = [
        ("sample_rate", ctypes.c_uint32),
        ("tech_mask", ctypes.c_uint32),
        ("stream_time", ctypes.c_int64),
        ("power_level_threshold", ctypes.c_float),
        ("corr_threshold", ctypes.c_float * 4),
        ("min_modulation_depth", ctypes.c_float * 4),
        ("max_modulation_depth", ctypes.c_float * 4),
    ]


class Frame(ctypes.Structure):
    _fields_ = [
        ("stream_id", ctypes.c_uint32),
        ("tech_type", ctypes.c_uint32),
        ("frame_type", ctypes.c_uint32),
        ("frame_flags", ctypes.c_uint32),
        ("frame_phase", ctypes.c_uint32),
        ("frame_rate", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("sample_start", ctypes.c_uint64),
        ("sample_end", ctypes.c_uint64),
        ("sample_rate", ctypes.c_uint64),
        ("data", ctypes.c_uint8 * 512),
    ]

    def as_tuple(self):
        return (self.tech_type, self.frame_type, self.frame_flags, self.frame_phase, self.frame_rate,
                self.sample_start, self.sample_end, self.sample_rate, bytes(self.data[:self.length]))


class Options(ctypes.Structure):
    _fields_ = [
        ("max_streams", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("frame_sink_bytes", ctypes.c_uint64),
    ]


class Batch(ctypes.Structure):
    _fields_ = [
        ("n_streams", ctypes.c_uint32),
        ("stride", ctypes.c_uint32),
        ("location", ctypes.c_uint32),
        ("sample_rate", ctypes.c_uint32),
        ("stream_ids", ctypes.POINTER(ctypes.c_uint32)),
        ("data", ctypes.POINTER(ctypes.c_void_p)),
        ("n_samples", ctypes.POINTER(ctypes.c_uint32)),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("launches", ctypes.c_uint64),
        ("samples", ctypes.c_uint64),
        ("frames", ctypes.c_uint64),
        ("dropped_frames", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("scan_ms", ctypes.c_double),
        ("window_ms", ctypes.c_double),
        ("scan_samples", ctypes.c_uint64),
        ("windows", ctypes.c_uint64),
        ("window_passes", ctypes.c_uint64),
        ("windowed_streams", ctypes.c_uint64),
        ("fallback_streams", ctypes.c_uint64),
        ("scan_repairs", ctypes.c_uint64),
        ("wave_ms", ctypes.c_double),
        ("wave_launches", ctypes.c_uint64),
        ("planes_ms", ctypes.c_double),
        ("wave_busy_ms", ctypes.c_double),
        ("pipelined_submissions", ctypes.c_uint64),
        ("pipeline_refronts", ctypes.c_uint64),
        ("pipeline_zeroed_edges", ctypes.c_uint64),
    ]


class SpectrumParams(ctypes.Structure):
    _fields_ = [
        ("length", ctypes.c_uint32),
        ("window", ctypes.c_uint32),
        ("decimation", ctypes.c_uint32),
        ("hop", ctypes.c_uint32),
        ("sample_rate", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 3),
    ]


class TapParams(ctypes.Structure):
    _fields_ = [
        ("sample_rate", ctypes.c_uint32),
        ("channels", ctypes.c_uint32),
        ("chunk_samples", ctypes.c_uint32),
        ("warm_samples", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 4),
    ]


class TapReport(ctypes.Structure):
    _fields_ = [
        ("chunks", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32),
        ("rewalked_chunks", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class TapReduceParams(ctypes.Structure):
    _fields_ = [
        ("bin_samples", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32),
        ("scratch_bytes", ctypes.c_uint64),
        ("reserved", ctypes.c_uint32 * 4),
    ]


class ApcmParams(ctypes.Structure):
    _fields_ = [
        ("sample_rate", ctypes.c_uint32),
        ("buffers_per_entry", ctypes.c_uint32),
        ("buffer_samples", ctypes.c_uint32),
        ("first_stream_id", ctypes.c_uint32),
        ("first_position", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32),
        ("range_start", ctypes.c_double),
        ("range_end", ctypes.c_double),
        ("reserved", ctypes.c_uint32 * 4),
    ]


# the reference's window names (FourierProcessTask.cpp:121-143; see include/nfcgpu.h for what they compute)
WINDOWS = {"none": 0, "hamming": 1, "hann": 2}


class NfcGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("nfcgpu error %d: %s" % (code, message))
        self.code = code


_lib = None


def load_library(path=LIB_PATH):
    """Load libnfcgpu.so and declare prototypes. Raises OSError if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own ROCm runtime (same SONAMEs as /opt/rocm). Whichever copy is loaded first serves the
    # whole process, and torch only finds the GPU through its own copy: load torch first when it is installed.
    if os.environ.get("NFCGPU_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = ctypes.CDLL(path)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    P = ctypes.POINTER
    lib.nfcgpu_default_params.argtypes = [P(Params)]
    lib.nfcgpu_default_params.restype = None
    lib.nfcgpu_init.argtypes = [i32, P(Options), P(vp)]
    lib.nfcgpu_shutdown.argtypes = [vp]
    lib.nfcgpu_stream_open.argtypes = [vp, P(Params), P(u32)]
    lib.nfcgpu_stream_open_many.argtypes = [vp, P(Params), u32, P(u32)]
    lib.nfcgpu_stream_configure.argtypes = [vp, u32, P(Params)]
    lib.nfcgpu_stream_reset.argtypes = [vp, u32]
    lib.nfcgpu_stream_close.argtypes = [vp, u32]
    lib.nfcgpu_submit.argtypes = [vp, u32, vp, u32, u32, u32]
    lib.nfcgpu_submit_batch.argtypes = [vp, P(Batch)]
    lib.nfcgpu_submit_uniform.argtypes = [vp, u32, u32, vp, u64, u32, u32, u32, u32]
    lib.nfcgpu_magnitude.argtypes = [vp, vp, u64, vp, u32]
    lib.nfcgpu_submit_fmt.argtypes = [vp, u32, vp, u32, u32, u32, u32]
    lib.nfcgpu_submit_batch_fmt.argtypes = [vp, P(Batch), u32]
    lib.nfcgpu_submit_uniform_fmt.argtypes = [vp, u32, u32, vp, u64, u32, u32, u32, u32, u32]
    lib.nfcgpu_magnitude_fmt.argtypes = [vp, vp, u64, vp, u32, u32]
    lib.nfcgpu_resample_radio.argtypes = [vp, vp, u64, u32, u32, vp, u64, u32, vp, u32]
    lib.nfcgpu_resample_radio_fmt.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, u64, u32, vp, u32]
    lib.nfcgpu_spectrum_default_params.argtypes = [P(SpectrumParams)]
    lib.nfcgpu_spectrum_default_params.restype = None
    lib.nfcgpu_spectrum_frames.argtypes = [P(SpectrumParams), u32]
    lib.nfcgpu_spectrum_frames.restype = u32
    lib.nfcgpu_spectrum.argtypes = [vp, vp, u64, u32, u32, P(SpectrumParams), vp, u64, u32]
    lib.nfcgpu_spectrum_fmt.argtypes = [vp, vp, u64, u32, u32, P(SpectrumParams), vp, u64, u32, u32]
    lib.nfcgpu_record.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, u64, vp, u32]
    lib.nfcgpu_tap_state_init.argtypes = [vp]
    lib.nfcgpu_tap_state_init.restype = None
    lib.nfcgpu_signal_tap.argtypes = [vp, vp, u64, u32, u32, u32, u32, P(TapParams), vp, vp, u64, u64, vp, P(TapReport), u32]
    lib.nfcgpu_stream_tap_state.argtypes = [vp, u32, vp]
    lib.nfcgpu_signal_tap_reduce.argtypes = [vp, vp, u64, u32, u32, u32, u32, P(TapParams), P(TapReduceParams), vp, vp, u32, vp, vp, P(TapReport), u32]
    lib.nfcgpu_apcm_bound.argtypes = [u64]
    lib.nfcgpu_apcm_bound.restype = u64
    lib.nfcgpu_apcm_encode.argtypes = [vp, vp, u64, vp, u32, u32, P(ApcmParams), vp, u64, u64, vp, u32]
    lib.nfcgpu_trace_write_signal.argtypes = [ctypes.c_char_p, vp, u32, ctypes.c_int64, ctypes.c_double, ctypes.c_double, P(u32), P(vp), P(u64), u32]
    lib.nfcgpu_wav_write.argtypes = [ctypes.c_char_p, vp, u64, u32, u32, u32, vp]
    lib.nfcgpu_wav_append.argtypes = [ctypes.c_char_p, vp, u64]
    lib.nfcgpu_flush.argtypes = [vp, u32]
    lib.nfcgpu_sync.argtypes = [vp]
    lib.nfcgpu_poll.argtypes = [vp, u32, P(Frame), u32, P(u32)]
    lib.nfcgpu_pending.argtypes = [vp, u32, P(u32)]
    lib.nfcgpu_sink_device_view.argtypes = [vp, P(vp), P(vp), P(u64)]
    lib.nfcgpu_sink_attach.argtypes = [vp, vp, u64, vp]
    lib.nfcgpu_sink_hold.argtypes = [vp, i32]
    lib.nfcgpu_sink_rewind.argtypes = [vp]
    lib.nfcgpu_stats_get.argtypes = [vp, P(Stats)]
    lib.nfcgpu_stats_get_sized.argtypes = [vp, P(Stats), ctypes.c_uint32]
    lib.nfcgpu_stats_reset.argtypes = [vp]
    lib.nfcgpu_profile.argtypes = [vp, i32]
    lib.nfcgpu_comm_unique_id.argtypes = [vp]
    lib.nfcgpu_comm_init.argtypes = [vp, vp, i32, i32]
    lib.nfcgpu_comm_destroy.argtypes = [vp]
    lib.nfcgpu_gather_frames.argtypes = [vp, vp, ctypes.c_uint64, P(ctypes.c_uint32), P(ctypes.c_uint64)]
    lib.nfcgpu_gather_frames_packed.argtypes = [vp, vp, ctypes.c_uint64, P(ctypes.c_uint32)]
    lib.nfcgpu_trace_write.argtypes = [vp, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_double, ctypes.c_double, P(ctypes.c_uint32)]
    lib.nfcgpu_trace_write_frames.argtypes = [ctypes.c_char_p, vp, ctypes.c_uint32, ctypes.c_int64, ctypes.c_double, ctypes.c_double, P(ctypes.c_uint32)]
    lib.nfcgpu_read_bandwidth.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, P(ctypes.c_double)]
    lib.nfcgpu_hip_stream.argtypes = [vp]
    lib.nfcgpu_hip_stream.restype = vp
    lib.nfcgpu_strerror.argtypes = [i32]
    lib.nfcgpu_strerror.restype = ctypes.c_char_p
    lib.nfcgpu_last_error.argtypes = [vp]
    lib.nfcgpu_last_error.restype = ctypes.c_char_p
    lib.nfcgpu_version.restype = ctypes.c_char_p
    _lib = lib
    return lib


def default_params(sample_rate=0, tech_mask=0xF):
    p = Params()
    load_library().nfcgpu_default_params(ctypes.byref(p))
    p.sample_rate = sample_rate
    p.tech_mask = tech_mask
    return p


def _wav_check(rc):
    if rc != 0:
        raise NfcGpuError(rc, load_library().nfcgpu_strerror(rc).decode())


def wav_write(path, pcm, sample_rate, channels=1, stream_time=0, keys=None):
    """A capture file as the reference's hw::RecordDevice writes it (nfcgpu_wav_write): int16 samples, interleaved for
    channels > 1. No context and no device."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
    assert channels and pcm.size % channels == 0
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.int32)
    assert k is None or k.size == channels
    _wav_check(load_library().nfcgpu_wav_write(os.fsencode(path), pcm.ctypes.data, pcm.size // channels, channels, sample_rate, stream_time,
                                               None if k is None else k.ctypes.data))


def wav_append(path, pcm):
    """More samples behind those of a file wav_write made (nfcgpu_wav_append); the channel count is the file's."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
    with open(path, "rb") as f:
        header = f.read(24)
    channels = int.from_bytes(header[22:24], "little") if len(header) == 24 else 0
    if channels == 0 or pcm.size % channels:
        raise NfcGpuError(-1, "not a capture file, or samples that do not fill its channels")
    _wav_check(load_library().nfcgpu_wav_append(os.fsencode(path), pcm.ctypes.data, pcm.size // channels))


def as_frames(frames):
    """A ctypes array of Frame records of such an array or of the tuples NfcGpu.poll returns."""
    if isinstance(frames, ctypes.Array):
        return frames
    out = (Frame * max(len(frames), 1))()
    for f, t in zip(out, frames):
        f.tech_type, f.frame_type, f.frame_flags, f.frame_phase, f.frame_rate, f.sample_start, f.sample_end, f.sample_rate = (int(v) for v in t[:8])
        payload = bytes(t[8])
        f.length = len(payload)
        ctypes.memmove(f.data, payload, min(len(payload), 512))
    return out


def trace_write_signal(path, frames, entries, stream_time=0, range_start=0.0, range_end=0.0):
    """A .trz with frame.json and one radio-<id>.apcm per APCM entry (nfcgpu_trace_write_signal): frames as NfcGpu.poll returns
    them (or a ctypes array of Frame), entries a list of bytes-like APCM entries as apcm_encode returns them. range_start /
    range_end select and shift the frames as nfcgpu_trace_write_frames does; the entries go in as they are. No context and no
    device. Returns the number of frames written."""
    records = as_frames(frames)
    held = [np.frombuffer(bytes(e), dtype=np.uint8) for e in entries]
    pointers = (ctypes.c_void_p * max(len(held), 1))(*[h.ctypes.data for h in held])
    sizes = (ctypes.c_uint64 * max(len(held), 1))(*[h.size for h in held])
    n = ctypes.c_uint32()
    _wav_check(load_library().nfcgpu_trace_write_signal(os.fsencode(path), ctypes.cast(records, ctypes.c_void_p), len(frames), int(stream_time),
                                                        range_start, range_end, ctypes.byref(n), pointers, sizes, len(held)))
    return int(n.value)


def as_tap_ranges(ranges):
    """TAP_RANGE_DTYPE [n] of such an array or of rows (buffer, first, count)."""
    if isinstance(ranges, np.ndarray) and ranges.dtype == TAP_RANGE_DTYPE:
        return np.ascontiguousarray(ranges).reshape(-1)
    rows = np.asarray(ranges, dtype=np.uint32).reshape(-1, 3)
    out = np.zeros(rows.shape[0], dtype=TAP_RANGE_DTYPE)
    out["buffer"], out["first"], out["count"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return out


def frame_ranges(frames, state, n_samples, buffer=0):
    """Decoded frames (the tuples of NfcGpu.poll) as ranges of a buffer of n_samples samples tapped from `state`
    (TAP_STATE_DTYPE [1], as NfcGpu.stream_tap_state gave it before the buffer was submitted): (TAP_RANGE_DTYPE [kept], the indices
    into `frames` of the frames kept). Sample i of the buffer has the clock state.clock + 1 + i (32-bit), the number a frame's
    sample_start and sample_end carry. sample_end is taken as inclusive: it is the clock of the sample at which the frame's last
    symbol ends (a carrier frame has sample_start == sample_end and gives a range of one sample). A frame is clipped to the
    buffer; a frame that lies outside it altogether is dropped."""
    clock0 = (int(np.asarray(state)["clock"].reshape(-1)[0]) + 1) & 0xFFFFFFFF
    ranges, kept = [], []
    for at, frame in enumerate(frames):
        first, last = ((int(v) - clock0 + 0x80000000) % 0x100000000 - 0x80000000 for v in (frame[5], frame[6]))
        first, last = max(first, 0), min(last, n_samples - 1)
        if first <= last:
            ranges.append((buffer, first, last - first + 1))
            kept.append(at)
    return as_tap_ranges(ranges), np.array(kept, dtype=np.int64)


class NfcGpu:
    """One nfcgpu context (one GPU, one HIP stream)."""

    def __init__(self, device=0, max_streams=1024, frame_sink_bytes=64 << 20):
        self.lib = load_library()
        self.ctx = ctypes.c_void_p()
        opts = Options(max_streams, 0, frame_sink_bytes)
        rc = self.lib.nfcgpu_init(device, ctypes.byref(opts), ctypes.byref(self.ctx))
        if rc != 0:
            self.ctx = None
            raise NfcGpuError(rc, self.lib.nfcgpu_strerror(rc).decode())

    def _check(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            msg = self.lib.nfcgpu_strerror(rc).decode()
            detail = self.lib.nfcgpu_last_error(self.ctx).decode()
            raise NfcGpuError(rc, "%s (%s)" % (msg, detail))
        return rc

    def close(self):
        if self.ctx:
            self.lib.nfcgpu_shutdown(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def open(self, params=None, count=1):
        first = ctypes.c_uint32()
        p = params or default_params()
        self._check(self.lib.nfcgpu_stream_open_many(self.ctx, ctypes.byref(p), count, ctypes.byref(first)))
        return first.value

    def configure(self, stream, params):
        self._check(self.lib.nfcgpu_stream_configure(self.ctx, stream, ctypes.byref(params)))

    def reset(self, stream):
        self._check(self.lib.nfcgpu_stream_reset(self.ctx, stream))

    def close_stream(self, stream):
        self._check(self.lib.nfcgpu_stream_close(self.ctx, stream))

    def submit(self, stream, samples, sample_rate, stride=1, fmt=FMT_F32):
        """samples: contiguous numpy array (host) of stride values per sample: float32, or with fmt=FMT_I16 int16 PCM.
        The format is what `fmt` says, never the array's dtype: the bytes are read as that format."""
        n = samples.size // stride
        if fmt == FMT_F32:
            self._check(self.lib.nfcgpu_submit(self.ctx, stream, samples.ctypes.data, n, stride, sample_rate))
        else:
            self._check(self.lib.nfcgpu_submit_fmt(self.ctx, stream, samples.ctypes.data, n, stride, sample_rate, fmt))

    def submit_batch(self, stream_ids, pointers, counts, sample_rate, stride=1, location=LOC_HOST, fmt=FMT_F32):
        n = len(stream_ids)
        ids = (ctypes.c_uint32 * n)(*stream_ids)
        ptrs = (ctypes.c_void_p * n)(*pointers)
        cnts = (ctypes.c_uint32 * n)(*counts)
        b = Batch(n, stride, location, sample_rate, ids, ptrs, cnts)
        if fmt == FMT_F32:
            self._check(self.lib.nfcgpu_submit_batch(self.ctx, ctypes.byref(b)))
        else:
            self._check(self.lib.nfcgpu_submit_batch_fmt(self.ctx, ctypes.byref(b), fmt))

    def submit_uniform(self, first, count, base_ptr, pitch_bytes, n_samples, sample_rate, stride=1, location=LOC_DEVICE, fmt=FMT_F32):
        if fmt == FMT_F32:
            self._check(self.lib.nfcgpu_submit_uniform(self.ctx, first, count, base_ptr, pitch_bytes, n_samples, stride,
                                                       location, sample_rate))
        else:
            self._check(self.lib.nfcgpu_submit_uniform_fmt(self.ctx, first, count, base_ptr, pitch_bytes, n_samples, stride,
                                                           location, sample_rate, fmt))

    def magnitude(self, iq, fmt=FMT_F32):
        """|IQ| of an interleaved numpy array (host memory) - float32, or with fmt=FMT_I16 int16 PCM, converted v / 32768 -
        computed on the device with the reference's roundings."""
        if fmt == FMT_F32:
            iq = np.ascontiguousarray(iq, dtype=np.float32)
            n = iq.size // 2
            out = np.empty(n, dtype=np.float32)
            self._check(self.lib.nfcgpu_magnitude(self.ctx, iq.ctypes.data, n, out.ctypes.data, LOC_HOST))
            return out
        iq = np.ascontiguousarray(iq, dtype=np.int16) if fmt == FMT_I16 else np.ascontiguousarray(iq)
        n = iq.size // 2
        out = np.empty(n, dtype=np.float32)
        self._check(self.lib.nfcgpu_magnitude_fmt(self.ctx, iq.ctypes.data, n, out.ctypes.data, LOC_HOST, fmt))
        return out

    def resample_radio(self, buffers, capacity_pairs=None, stride=1, fmt=FMT_F32):
        """Adaptive (value, offset) control points of each row of a 2-D array [n_buffers, n * stride] of buffers (host memory):
        float32 magnitudes, or with stride=2 interleaved IQ, or with fmt=FMT_I16 the int16 PCM of a capture file - the format is
        what `fmt` says, never the array's dtype. The resampled value is the magnitude the decoder forms of a sample. Returns a
        list of (pairs, 2) arrays."""
        buffers = np.ascontiguousarray(buffers, dtype=np.int16 if fmt == FMT_I16 else np.float32)
        nb, width = buffers.shape
        assert stride and width % stride == 0
        n = width // stride
        cap = capacity_pairs or (n + n // 255 + 2)
        out = np.zeros((nb, 2 * cap), dtype=np.float32)
        counts = np.zeros(nb, dtype=np.uint32)
        if stride == 1 and fmt == FMT_F32:
            self._check(self.lib.nfcgpu_resample_radio(self.ctx, buffers.ctypes.data, n * 4, nb, n, out.ctypes.data, 2 * cap * 4, cap,
                                                       counts.ctypes.data, LOC_HOST))
        else:
            self._check(self.lib.nfcgpu_resample_radio_fmt(self.ctx, buffers.ctypes.data, width * buffers.itemsize, nb, n, stride, fmt,
                                                           out.ctypes.data, 2 * cap * 4, cap, counts.ctypes.data, LOC_HOST))
        return [out[b, :2 * counts[b]].reshape(-1, 2) for b in range(nb)]

    def resample_radio_device(self, in_ptr, in_pitch_bytes, n_buffers, n_samples, out_ptr, out_pitch_bytes, capacity_pairs, counts_ptr,
                              stride=1, fmt=FMT_F32):
        """Same with device pointers (input, output and counts resident in HBM)."""
        if stride == 1 and fmt == FMT_F32:
            self._check(self.lib.nfcgpu_resample_radio(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_samples, out_ptr, out_pitch_bytes,
                                                       capacity_pairs, counts_ptr, LOC_DEVICE))
        else:
            self._check(self.lib.nfcgpu_resample_radio_fmt(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_samples, stride, fmt, out_ptr,
                                                           out_pitch_bytes, capacity_pairs, counts_ptr, LOC_DEVICE))

    def spectrum_params(self, length=1024, window="hamming", decimation=0, hop=0, sample_rate=10000000):
        p = SpectrumParams()
        self.lib.nfcgpu_spectrum_default_params(ctypes.byref(p))
        p.length, p.decimation, p.hop, p.sample_rate = length, decimation, hop, sample_rate
        p.window = WINDOWS[window] if isinstance(window, str) else window
        return p

    def spectrum_frames(self, n_pairs, **params):
        """Frames a buffer of n_pairs IQ pairs gives with these parameters (nfcgpu_spectrum_frames)."""
        return self.lib.nfcgpu_spectrum_frames(ctypes.byref(self.spectrum_params(**params)), n_pairs)

    def spectrum(self, buffers, length=1024, window="hamming", decimation=0, hop=0, sample_rate=10000000, fmt=FMT_F32):
        """Magnitude spectra of an array [n_buffers, n_pairs, 2] of IQ buffers (host memory) - float32, or with fmt=FMT_I16 the
        int16 PCM of a two-channel capture file, converted v / 32768 as it is loaded; the format is what `fmt` says, never the
        array's dtype - as the reference's FourierProcessTask publishes them (negative frequencies first):
        [n_buffers, frames, length]; hop = 0 gives the one frame the task publishes for a buffer, hop > 0 a frame every hop
        pairs."""
        buffers = np.ascontiguousarray(buffers, dtype=np.int16 if fmt == FMT_I16 else np.float32)
        nb, n, two = buffers.shape
        assert two == 2
        p = self.spectrum_params(length, window, decimation, hop, sample_rate)
        frames = self.lib.nfcgpu_spectrum_frames(ctypes.byref(p), n)
        out = np.zeros((nb, frames, length), dtype=np.float32)
        if fmt == FMT_F32:
            self._check(self.lib.nfcgpu_spectrum(self.ctx, buffers.ctypes.data, n * 8, nb, n, ctypes.byref(p), out.ctypes.data,
                                                 frames * length * 4, LOC_HOST))
        else:
            self._check(self.lib.nfcgpu_spectrum_fmt(self.ctx, buffers.ctypes.data, n * 2 * buffers.itemsize, nb, n, ctypes.byref(p),
                                                     out.ctypes.data, frames * length * 4, LOC_HOST, fmt))
        return out

    def spectrum_device(self, in_ptr, in_pitch_bytes, n_buffers, n_pairs, out_ptr, out_pitch_bytes, length=1024, window="hamming",
                        decimation=0, hop=0, sample_rate=10000000, fmt=FMT_F32):
        """Same with device pointers (IQ and spectra resident in HBM); returns the frames written per buffer."""
        p = self.spectrum_params(length, window, decimation, hop, sample_rate)
        if fmt == FMT_F32:
            self._check(self.lib.nfcgpu_spectrum(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_pairs, ctypes.byref(p), out_ptr,
                                                 out_pitch_bytes, LOC_DEVICE))
        else:
            self._check(self.lib.nfcgpu_spectrum_fmt(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_pairs, ctypes.byref(p), out_ptr,
                                                     out_pitch_bytes, LOC_DEVICE, fmt))
        return self.lib.nfcgpu_spectrum_frames(ctypes.byref(p), n_pairs)

    def record(self, buffers, stride=1, mode=RECORD_SAME, levels=True):
        """16-bit PCM of a float32 array [n_buffers, n * stride] (host memory) as a capture file holds it, and the levels of
        every buffer (nfcgpu_record): (int16 [n_buffers, n * channels], LEVELS_DTYPE [n_buffers] or None)."""
        buffers = np.ascontiguousarray(buffers, dtype=np.float32)
        nb, width = buffers.shape
        assert width % stride == 0
        n = width // stride
        channels = 2 if stride == 2 and mode == RECORD_SAME else 1
        out = np.zeros((nb, n * channels), dtype=np.int16)
        lv = np.zeros(nb, dtype=LEVELS_DTYPE) if levels else None
        self._check(self.lib.nfcgpu_record(self.ctx, buffers.ctypes.data, width * 4, nb, n, stride, mode, out.ctypes.data, n * channels * 2,
                                           lv.ctypes.data if levels else None, LOC_HOST))
        return out, lv

    def record_device(self, in_ptr, in_pitch_bytes, n_buffers, n_samples, out_ptr, out_pitch_bytes, stride=1, mode=RECORD_SAME, levels_ptr=None):
        """Same with device pointers (samples, PCM and levels resident in HBM); levels_ptr None skips the levels."""
        self._check(self.lib.nfcgpu_record(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_samples, stride, mode, out_ptr, out_pitch_bytes,
                                           levels_ptr, LOC_DEVICE))

    def tap_state_init(self, count=1):
        """TAP_STATE_DTYPE [count] of streams just opened (nfcgpu_tap_state_init)."""
        states = np.zeros(count, dtype=TAP_STATE_DTYPE)
        for i in range(count):
            self.lib.nfcgpu_tap_state_init(states.ctypes.data + i * TAP_STATE_DTYPE.itemsize)
        return states

    def signal_tap(self, buffers, sample_rate, channels=TAP_ALL, stride=1, fmt=FMT_F32, state=None, chunk=0, warm=0):
        """The front end's per-sample signals of a 2-D array [n_buffers, n * stride] (host memory; float32, or with fmt=FMT_I16
        int16 PCM) as the decoder forms them (nfcgpu_signal_tap): (dict name -> float32 [n_buffers, n] of the selected
        channels, TAP_STATE_DTYPE [n_buffers] behind the last sample, TapReport). state: TAP_STATE_DTYPE [n_buffers] to start
        from, None = streams just opened. chunk, warm: how the buffers are cut (0, 0: the library's choice); results do not
        depend on it."""
        buffers = np.ascontiguousarray(buffers, dtype=np.int16 if fmt == FMT_I16 else np.float32)
        nb, width = buffers.shape
        assert width % stride == 0
        n = width // stride
        names = [name for bit, name in enumerate(TAP_NAMES) if channels >> bit & 1]
        plane = (n * 4 + 15) & ~15
        out = np.zeros((nb, max(len(names), 1), plane // 4), dtype=np.float32)
        if state is not None:
            state = np.ascontiguousarray(state, dtype=TAP_STATE_DTYPE)
            assert state.shape == (nb,)
        states = np.zeros(nb, dtype=TAP_STATE_DTYPE)
        p = TapParams(sample_rate, channels, chunk, warm)
        report = TapReport()
        self._check(self.lib.nfcgpu_signal_tap(self.ctx, buffers.ctypes.data, width * buffers.itemsize, nb, n, stride, fmt, ctypes.byref(p),
                                               None if state is None else state.ctypes.data, out.ctypes.data, out.shape[1] * plane, plane,
                                               states.ctypes.data, ctypes.byref(report), LOC_HOST))
        return {name: np.ascontiguousarray(out[:, k, :n]) for k, name in enumerate(names)}, states, report

    def signal_tap_device(self, in_ptr, in_pitch_bytes, n_buffers, n_samples, sample_rate, out_ptr, out_pitch_bytes, plane_pitch_bytes,
                          channels=TAP_ALL, stride=1, fmt=FMT_F32, state_in_ptr=None, state_out_ptr=None, chunk=0, warm=0):
        """Same with device pointers (samples, planes and states resident in HBM); returns the TapReport."""
        p = TapParams(sample_rate, channels, chunk, warm)
        report = TapReport()
        self._check(self.lib.nfcgpu_signal_tap(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_samples, stride, fmt, ctypes.byref(p), state_in_ptr,
                                               out_ptr, out_pitch_bytes, plane_pitch_bytes, state_out_ptr, ctypes.byref(report), LOC_DEVICE))
        return report

    def signal_tap_reduce(self, buffers, sample_rate, channels=TAP_ALL, ranges=None, bin_samples=0, stride=1, fmt=FMT_F32, state=None,
                          chunk=0, warm=0, scratch_bytes=0, with_state=False):
        """The tap's channels reduced over sample ranges (nfcgpu_signal_tap_reduce) of a 2-D array [n_buffers, n * stride] in host
        memory: TAP_STAT_DTYPE [n_ranges, K], K the channels selected, in bit order. ranges: TAP_RANGE_DTYPE [n_ranges] (or rows
        of buffer, first, count), or None: every buffer in bins of bin_samples, range r = buffer r // bins, bin r % bins.
        scratch_bytes bounds the planes held on the device at a time (0: the library's choice). with_state: (records,
        TAP_STATE_DTYPE [n_buffers] behind the last sample, TapReport)."""
        buffers = np.ascontiguousarray(buffers, dtype=np.int16 if fmt == FMT_I16 else np.float32)
        nb, width = buffers.shape
        assert width % stride == 0
        n = width // stride
        k = bin(channels & TAP_ALL).count("1")
        if ranges is None:
            n_ranges, rp = nb * (-(-n // bin_samples) if bin_samples else 0), None
        else:
            ranges = as_tap_ranges(ranges)
            n_ranges, rp = ranges.shape[0], ranges.ctypes.data
        if state is not None:
            state = np.ascontiguousarray(state, dtype=TAP_STATE_DTYPE)
            assert state.shape == (nb,)
        out = np.zeros((n_ranges, max(k, 1)), dtype=TAP_STAT_DTYPE)
        states = np.zeros(nb, dtype=TAP_STATE_DTYPE)
        p, q, report = TapParams(sample_rate, channels, chunk, warm), TapReduceParams(bin_samples, 0, scratch_bytes), TapReport()
        self._check(self.lib.nfcgpu_signal_tap_reduce(self.ctx, buffers.ctypes.data, width * buffers.itemsize, nb, n, stride, fmt, ctypes.byref(p),
                                                      ctypes.byref(q), None if state is None else state.ctypes.data, rp,
                                                      0 if ranges is None else n_ranges, out.ctypes.data, states.ctypes.data, ctypes.byref(report), LOC_HOST))
        return (out, states, report) if with_state else out

    def signal_tap_reduce_device(self, in_ptr, in_pitch_bytes, n_buffers, n_samples, sample_rate, out_ptr, channels=TAP_ALL, ranges_ptr=None,
                                 n_ranges=0, bin_samples=0, stride=1, fmt=FMT_F32, state_in_ptr=None, state_out_ptr=None, chunk=0, warm=0,
                                 scratch_bytes=0):
        """Same with device pointers (samples, ranges, records and states resident in HBM); returns the TapReport. A range that is
        not inside the buffers gets the empty record and the call raises NfcGpuError (NFCGPU_EINVAL) with the other records complete."""
        p, q, report = TapParams(sample_rate, channels, chunk, warm), TapReduceParams(bin_samples, 0, scratch_bytes), TapReport()
        self._check(self.lib.nfcgpu_signal_tap_reduce(self.ctx, in_ptr, in_pitch_bytes, n_buffers, n_samples, stride, fmt, ctypes.byref(p), ctypes.byref(q),
                                                      state_in_ptr, ranges_ptr, n_ranges, out_ptr, state_out_ptr, ctypes.byref(report), LOC_DEVICE))
        return report

    def apcm_encode(self, points, sample_rate, buffers_per_entry=1, buffer_samples=0, first_stream_id=0, first_position=0, range_start=0.0,
                    range_end=0.0, with_info=False):
        """The control points of consecutive buffers (a list of (pairs, 2) float32 arrays as resample_radio returns them; host
        memory) as APCM entries (nfcgpu_apcm_encode): buffers_per_entry buffers make an entry, buffer j of an entry stands at the
        stream position first_position + j * buffer_samples, entry e carries the id first_stream_id + e. Returns a list of bytes,
        one per entry; with_info: (entries, APCM_INFO_DTYPE [n_entries])."""
        points = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) for p in points]
        nb = len(points)
        assert buffers_per_entry and nb % buffers_per_entry == 0
        n_entries = nb // buffers_per_entry
        counts = np.array([p.shape[0] for p in points], dtype=np.uint32)
        cap = int(counts.max()) if nb else 0
        rows = np.zeros((max(nb, 1), 2 * max(cap, 1)), dtype=np.float32)
        for b, p in enumerate(points):
            rows[b, :2 * p.shape[0]] = p.reshape(-1)
        most = max([int(counts[e * buffers_per_entry:(e + 1) * buffers_per_entry].sum()) for e in range(n_entries)], default=0)
        pitch = (int(self.lib.nfcgpu_apcm_bound(most)) + 3) & ~3
        out = np.zeros((max(n_entries, 1), pitch), dtype=np.uint8)
        info = np.zeros(max(n_entries, 1), dtype=APCM_INFO_DTYPE)
        p = ApcmParams(sample_rate, buffers_per_entry, buffer_samples, first_stream_id, first_position, 0, range_start, range_end)
        self._check(self.lib.nfcgpu_apcm_encode(self.ctx, rows.ctypes.data, rows.shape[1] * 4, counts.ctypes.data, nb, cap, ctypes.byref(p),
                                                out.ctypes.data, pitch, pitch, info.ctypes.data, LOC_HOST))
        entries = [out[e, :int(info["bytes"][e])].tobytes() for e in range(n_entries)]
        return (entries, info[:n_entries]) if with_info else entries

    def apcm_encode_device(self, pairs_ptr, pairs_pitch_bytes, counts_ptr, n_buffers, capacity_pairs, sample_rate, out_ptr, out_pitch_bytes,
                           capacity_bytes, info_ptr, buffers_per_entry=1, buffer_samples=0, first_stream_id=0, first_position=0, range_start=0.0,
                           range_end=0.0):
        """Same with device pointers: the rows and counts nfcgpu_resample_radio left in HBM, the entries and their APCM_INFO_DTYPE
        records written there. An entry that does not fit raises NfcGpuError (NFCGPU_EOVERFLOW), a count above capacity_pairs
        NFCGPU_EINVAL, with every entry complete as far as it goes."""
        p = ApcmParams(sample_rate, buffers_per_entry, buffer_samples, first_stream_id, first_position, 0, range_start, range_end)
        self._check(self.lib.nfcgpu_apcm_encode(self.ctx, pairs_ptr, pairs_pitch_bytes, counts_ptr, n_buffers, capacity_pairs, ctypes.byref(p), out_ptr,
                                                out_pitch_bytes, capacity_bytes, info_ptr, LOC_DEVICE))

    def trace_write_capture(self, path, samples, sample_rate, frames=(), buffer_samples=65536, stride=1, fmt=FMT_F32, stream_id=0, stream_time=0,
                            range_start=0.0, range_end=0.0):
        """A stream's capture and its frames as a .trz whose signal view is filled: the samples (1-D, host memory; the format is
        what `fmt` and `stride` say) are cut into buffers of buffer_samples (the last one may be shorter, at least 25 samples),
        resampled (resample_radio), encoded as one APCM entry (apcm_encode) and written with the frames (trace_write_signal).
        range_start / range_end apply to the signal and to the frames alike. Returns (frames written, points stored)."""
        samples = np.ascontiguousarray(samples, dtype=np.int16 if fmt == FMT_I16 else np.float32).reshape(-1)
        n = samples.size // stride
        whole = n // buffer_samples
        points = []
        if whole:
            points += self.resample_radio(samples[:whole * buffer_samples * stride].reshape(whole, -1), stride=stride, fmt=fmt)
        if n - whole * buffer_samples >= 25:
            points += self.resample_radio(samples[whole * buffer_samples * stride:n * stride].reshape(1, -1), stride=stride, fmt=fmt)
        entries, info = self.apcm_encode(points, sample_rate, buffers_per_entry=max(len(points), 1), buffer_samples=buffer_samples,
                                         first_stream_id=stream_id, range_start=range_start, range_end=range_end, with_info=True) if points else ([], [])
        written = trace_write_signal(path, frames, entries, stream_time, range_start, range_end)
        return written, int(info["records"][0]) if points else 0

    def stream_tap_state(self, stream):
        """TAP_STATE_DTYPE [1]: the front-end state the stream's next buffer will start from (nfcgpu_stream_tap_state)."""
        state = np.zeros(1, dtype=TAP_STATE_DTYPE)
        self._check(self.lib.nfcgpu_stream_tap_state(self.ctx, stream, state.ctypes.data))
        return state

    def flush(self, stream):
        self._check(self.lib.nfcgpu_flush(self.ctx, stream))

    def sync(self):
        self._check(self.lib.nfcgpu_sync(self.ctx))

    def poll(self, stream, capacity=4096):
        out = (Frame * capacity)()
        n = ctypes.c_uint32()
        self._check(self.lib.nfcgpu_poll(self.ctx, stream, out, capacity, ctypes.byref(n)))
        return [out[i].as_tuple() for i in range(n.value)]

    def sink_view(self):
        words, cursor, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        self._check(self.lib.nfcgpu_sink_device_view(self.ctx, ctypes.byref(words), ctypes.byref(cursor), ctypes.byref(cap)))
        return words.value, cursor.value, cap.value

    def sink_attach(self, words_ptr, capacity_words, ctl_ptr):
        self._check(self.lib.nfcgpu_sink_attach(self.ctx, words_ptr, capacity_words, ctl_ptr))

    def sink_hold(self, hold):
        self._check(self.lib.nfcgpu_sink_hold(self.ctx, int(hold)))

    def sink_rewind(self):
        self._check(self.lib.nfcgpu_sink_rewind(self.ctx))

    def profile(self, enable):
        self._check(self.lib.nfcgpu_profile(self.ctx, int(enable)))

    def stats(self):
        s = Stats()
        self._check(self.lib.nfcgpu_stats_get_sized(self.ctx, ctypes.byref(s), ctypes.sizeof(Stats)))
        return s

    def stats_reset(self):
        self._check(self.lib.nfcgpu_stats_reset(self.ctx))

    def hip_stream(self):
        return self.lib.nfcgpu_hip_stream(self.ctx)

    # ---- multi-GPU frame gather over RCCL, behind the C ABI ----
    def comm_unique_id(self):
        """128 opaque bytes made by rank 0 (ncclGetUniqueId); carry them to the other ranks"""
        buf = ctypes.create_string_buffer(128)
        self._check(self.lib.nfcgpu_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, n_ranks):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self.lib.nfcgpu_comm_init(self.ctx, buf, rank, n_ranks))
        self._n_ranks = n_ranks

    def comm_destroy(self):
        self._check(self.lib.nfcgpu_comm_destroy(self.ctx))

    def gather_frames(self, gathered_ptr, capacity_words, packed=True):
        """every rank's frame records into the device buffer at gathered_ptr (RCCL behind the C ABI); returns (counts, stride):
        packed (nfcgpu_gather_frames_packed): rank r's records start at sum(counts[:r]), stride 0; otherwise
        (nfcgpu_gather_frames, the layout of rounds 1-2) at r * stride, stride = max(counts)"""
        counts = (ctypes.c_uint32 * self._n_ranks)()
        if packed:
            self._check(self.lib.nfcgpu_gather_frames_packed(self.ctx, gathered_ptr, capacity_words, counts), allow=(-6,))
            return list(counts), 0
        stride = ctypes.c_uint64()
        self._check(self.lib.nfcgpu_gather_frames(self.ctx, gathered_ptr, capacity_words, counts, ctypes.byref(stride)), allow=(-6,))
        return list(counts), int(stride.value)

    def trace_write(self, stream_id, path, range_start=0.0, range_end=0.0):
        """the frames decoded for a stream (still queued) as a .trz the reference application opens; returns the frame count"""
        n = ctypes.c_uint32()
        self._check(self.lib.nfcgpu_trace_write(self.ctx, stream_id, os.fsencode(path), range_start, range_end, ctypes.byref(n)), allow=(-6,))
        return int(n.value)

    def read_bandwidth(self, device_ptr, n_bytes, repeats=5):
        """streaming-read GB/s over a device buffer (16-byte loads): the measured HBM roofline denominator"""
        g = ctypes.c_double()
        self._check(self.lib.nfcgpu_read_bandwidth(self.ctx, device_ptr, n_bytes, repeats, ctypes.byref(g)))
        return g.value
