"""Modulated exchanges that no capture holds (tests/modulated_cases.py) through the C ABI of libnfcgpu.so: ragged batches a
buffer per step, the IQ entry, whole streams in one submission and per-stream thresholds, every stream compared with the live
reference decoder on the same float32 samples (all nine fields of every frame, carrier frames included).

On the device every leg takes every scenario (ids "everything ..."). tests/test_modulated_emulated.py runs this file on the CPU
against the emulated runtime, which decodes some 30 000 samples a second (20 minutes of one core for the table): there the whole
table goes through once, in buffers of 65 536 samples, a fixed third of it once more through the IQ entry in buffers of 4 099
samples, and a ninth of it as whole streams in one submission (ids "host ...", in slices so that they can run side by side); the
"everything" ids are deselected. Which scenarios a leg takes is a constant below."""
import ctypes

import numpy as np
import pytest

import modulated_cases as C
import nfc_testlib as T
from test_modulated import complaints

pytestmark = pytest.mark.gpu

EVERYTHING = [c.name for c in C.CASES]
HOST_WHOLE = [c.name for c in C.CASES if c.where == "all"]       # without the long waits of FWI 8 and 14
# every technology, rate, polarity and defect, the protocol feedback of each technology, a mix, both other sample rates
HOST_THIRD = [
    "a212 short and long", "b212 polls short and long", "b424", "f424 reversed short and long", "v 1-of-256",
    "a106 wrong parity", "a424 wrong crc and parity", "a106 truncated", "a106 answers absent, early and late",
    "b106 wrong crc", "b106 truncated", "f212 wrong crc and sync", "f424 truncated", "v wrong crc", "v truncated",
    "a106 rats fsdi 5 then frames over 64 bytes", "a106 ats fwi 0", "a106 mifare auth then ciphered frames", "b106 atqb fsdi 0 fwi 0",
    "b106 attrib tr0 2 fsdi 5", "f212 reqc with 4 slots", "f424 v a212 b",
    "weak a106 step 3", "weak a424 step 2", "weak b106 step 4", "weak f212 step 3", "weak f424 step 5", "weak v step 2",
    "a106 defects at 5 MS/s", "b106 short and long at 2.5 MS/s", "f212 defects at 5 MS/s", "v defects at 2.5 MS/s",
    "a b f v a with carrier gaps at 2.5 MS/s",
]
WEAK = [c.name for c in C.CASES if c.group == 5]
HOST_WEAK = [n for n in WEAK if n.endswith("step 2")]
assert set(HOST_THIRD) <= set(HOST_WHOLE) and 3 * len(HOST_THIRD) <= len(HOST_WHOLE) + 2

_streams = {}


def stream(name):
    """(samples, sample rate, reference frames) of a scenario, built once per run"""
    if name not in _streams:
        if T.reference_lib() is None:
            pytest.skip("oracle/_ref not available")
        x, sent = C.build(name)
        fs = C.BY_NAME[name].fs
        ref, _ = T.reference_decode(x, sample_rate=fs, keep_carrier=True, cap=16384, defined_storage=True)
        if C.BY_NAME[name].where == "device":
            assert complaints(sent, ref) == [], name     # (tests/test_modulated.py checks the others without a device)
        _streams[name] = (x, fs, ref)
    return _streams[name]


@pytest.fixture(scope="module")
def gpu(built):
    import nfclab_amd
    g = nfclab_amd.NfcGpu(device=0, max_streams=4096, frame_sink_bytes=64 << 20)
    yield g
    g.close()


def decode(gpu, inputs, chunk, stride=1, params=None):
    """inputs: [(samples, sample rate)], one stream each; all of them in one ragged submit_batch per step of `chunk` samples and
    sample rate (chunk None: a stream in one piece). Returns the frames of every stream."""
    sids = [gpu.open(params[i] if params else None) for i in range(len(inputs))]
    fed = [T.magnitude_to_iq(x, seed=i) if stride == 2 else x for i, (x, fs) in enumerate(inputs)]
    for fs in sorted({fs for x, fs in inputs}):
        mine = [i for i, (x, f) in enumerate(inputs) if f == fs]
        longest = max(inputs[i][0].size for i in mine)
        step = chunk or longest
        for pos in range(0, longest, step):
            parts = [(i, np.ascontiguousarray(fed[i][pos * stride:(pos + step) * stride])) for i in mine]
            parts = [(i, p) for i, p in parts if p.size]
            gpu.submit_batch([sids[i] for i, p in parts], [p.ctypes.data for i, p in parts], [p.size // stride for i, p in parts], fs, stride=stride)
    out = []
    for sid in sids:
        out.append(gpu.poll(sid, capacity=16384))
        gpu.close_stream(sid)
    return out


def check(gpu, names, chunk, stride=1):
    data = [stream(n) for n in names]
    got = decode(gpu, [(x, fs) for x, fs, ref in data], chunk, stride)
    bad = [n for n, g, (x, fs, ref) in zip(names, got, data) if g != ref]
    assert bad == []
    return sum(len(ref) for x, fs, ref in data)


@pytest.mark.parametrize("names,chunk,stride", [
    pytest.param(EVERYTHING, 65536, 1, id="everything in buffers of 65536"),
    pytest.param(EVERYTHING, 4099, 1, id="everything in buffers of 4099"),
    pytest.param(EVERYTHING, 65536, 2, id="everything through the IQ entry"),
] + [pytest.param(HOST_WHOLE[k::6], 65536, 1, id="host whole table in buffers of 65536, slice %d of 6" % k) for k in range(6)]
  + [pytest.param(HOST_THIRD[k::2], 4099, 2, id="host third through the IQ entry in buffers of 4099, slice %d of 2" % k) for k in range(2)])
def test_every_scenario_in_one_ragged_batch_per_step(gpu, names, chunk, stride):
    assert check(gpu, names, chunk, stride) > 3 * len(names)      # (more than the three carrier frames that open every stream)


@pytest.mark.parametrize("names", [pytest.param(EVERYTHING, id="everything")]
                         + [pytest.param(HOST_THIRD[::3], id="host ninth")])
def test_every_scenario_as_one_submission(gpu, names):
    """each stream whole in one submission: the route the runtime picks by itself for long input"""
    assert check(gpu, names, None) > 3 * len(names)


# thresholds moved both ways: (power level, correlation, minimum depth, maximum depth), None = the default
MOVED = [(None, 0.05, None, None), (None, 0.9, None, None), (None, None, 0.05, None), (None, None, 0.93, None), (None, None, None, 0.5),
         (0.5, None, None, None), (0.004, 0.3, 0.5, 0.8)]


@pytest.mark.parametrize("names,moves", [pytest.param(WEAK, MOVED, id="everything"), pytest.param(HOST_WEAK, MOVED[2:4], id="host step 2")])
def test_weak_signals_with_the_thresholds_moved(gpu, names, moves):
    """The weak-signal sweeps again with every stream's power level, correlation and modulation-depth thresholds moved (the
    reference run with the same parameters): the same samples are decoded with one setting and not with another, on both sides."""
    import nfclab_amd
    if T.reference_lib() is None:
        pytest.skip("oracle/_ref not available")
    nan = float("nan")
    counts = {n: set() for n in names}
    for power, corr, low, high in moves:
        params, refs, inputs = [], [], []
        for n in names:
            x, fs, plain = stream(n)
            p = nfclab_amd.default_params()
            rp = T.RefParams(p.tech_mask, nan, *[(ctypes.c_float * 4)(nan, nan, nan, nan) for _ in range(3)])
            if power is not None:
                p.power_level_threshold = rp.power_level_threshold = float(np.float32(power))
            for t in range(4):
                if corr is not None:
                    p.corr_threshold[t] = rp.corr_threshold[t] = float(np.float32(corr))
                if low is not None:
                    p.min_modulation_depth[t] = rp.min_depth[t] = float(np.float32(low))
                if high is not None:
                    p.max_modulation_depth[t] = rp.max_depth[t] = float(np.float32(high))
            ref, _ = T.reference_decode(x, sample_rate=fs, keep_carrier=True, cap=16384, params=rp, defined_storage=True)
            params.append(p)
            refs.append(ref)
            inputs.append((x, fs))
            counts[n].add(sum(f[1] in (0x102, 0x103) for f in ref))
            counts[n].add(sum(f[1] in (0x102, 0x103) for f in plain))
        got = decode(gpu, inputs, 65536, params=params)
        bad = [n for n, g, r in zip(names, got, refs) if g != r]
        assert bad == [], (power, corr, low, high)
    # (on the reference's side alone: in every technology's sweep the settings change how many frames come out of the same samples)
    for tech in "abfv":
        assert any(len(counts[n]) > 1 for n in names if n.startswith("weak " + tech)), (tech, counts)
