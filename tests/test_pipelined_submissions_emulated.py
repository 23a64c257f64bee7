"""Pipelined submissions on the emulated runtime of tests/hostsim: submissions of the same streams through
nfcgpu_submit_uniform without a synchronisation in between run their front (scan, seam rounds, planes) under the pending tail
of the submission before (run_windowed, nfcgpu.hip). Every case is decoded twice, with NFCGPU_PIPELINE=1 and 0, and the
frames - every field, the order per stream - have to be the same; the plain cases are also held against the reference decoder
where oracle/_ref is built. The knobs force the time-parallel path on small inputs, as in tests/test_time_parallel.py."""
import json
import os
import subprocess
import sys

import pytest

import nfc_testlib as T

DRIVER = os.path.join(T.ROOT, "tests", "pipelined_driver.py")
EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")


@pytest.fixture(scope="module")
def emulated(built):
    if not os.path.exists(EMU):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    return EMU


def run(scenario, pipeline, extra=None):
    env = dict(os.environ, NFCGPU_LIB=EMU, NFCGPU_NO_TORCH="1", NFCGPU_WINDOWED_MIN="4096", NFCGPU_SCAN_CHUNK="32768", NFCGPU_SOLO_SAMPLES="0",
               NFCGPU_PIPELINE="1" if pipeline else "0")
    env.update(extra or {})
    sc = dict({"streams": "dense", "count": 3, "samples": 98304, "submissions": 4, "fmt": "f32", "location": "device", "between": None,
               "reference": pipeline and T.reference_lib() is not None}, **scenario)
    done = subprocess.run([sys.executable, DRIVER, json.dumps(sc)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=3000)
    assert done.returncode == 0, done.stderr[-3000:]
    return json.loads(done.stdout.strip().splitlines()[-1])


def both(scenario, extra=None):
    piped, plain = run(scenario, True, extra), run(scenario, False, extra)
    assert plain["stats"]["pipelined"] == 0 and plain["stats"]["refronts"] == 0, plain["stats"]
    assert piped["total"] > 0
    assert piped["frames"] == plain["frames"]
    assert piped["log"] == plain["log"]
    assert piped.get("mismatching", []) == [], piped["mismatching"]
    return piped


@pytest.mark.parametrize("scenario", [
    {},                                                       # dense, on the grid, float rows, device-resident
    {"location": "host"},
    {"fmt": "i16"},
    {"fmt": "i16", "location": "host"},
    {"streams": "offgrid"},                                   # carry lanes alone
    {"streams": "sparse", "count": 6, "samples": 131072},
    {"streams": "sparse", "count": 6, "samples": 131072, "location": "host", "submissions": 5},
], ids=["dense", "dense-host", "dense-i16", "dense-i16-host", "offgrid", "sparse", "sparse-host"])
def test_back_to_back_submissions_decode_the_same_frames_and_overlap(emulated, scenario):
    """the overlap really taken: every submission but the first runs its front under the tail of the one before"""
    piped = both(scenario)
    assert piped["stats"]["pipelined"] == scenario.get("submissions", 4) - 1, piped["stats"]
    assert piped["stats"]["fallback"] == 0, piped["stats"]


def test_both_orders_of_the_planes_walk(emulated):
    """more than 4 Mi samples per submission: the planes are written beside the rounds of second walks, on the lowest-priority
    stream - run at once (NFC_EMU_DEFER_LOW unset) or only when somebody waits for them (set)"""
    sc = {"count": 5, "samples": 1 << 20, "submissions": 2}
    for low in ({}, {"NFC_EMU_DEFER_LOW": "1"}):
        piped = both(sc, low)
        assert piped["stats"]["pipelined"] == 1, piped["stats"]


@pytest.mark.parametrize("between", ["poll", "flush", "pending", "stats", "reset", "configure", "reopen", "other_range", "sequential", "sink_rewind"])
def test_a_call_between_two_submissions_completes_the_pending_tail(emulated, between):
    """every other entry point completes the pending tail before it does anything else: same frames, same answers - and the
    reference decoder's frames for the samples every stream was fed. For initialize() and changed thresholds in mid-stream the
    reference wrapper of the tests has no entry (one call decodes one stream from its start); there the same calls with the
    time-parallel path switched off - the sequential kernels, which share nothing with run_windowed and are held against the
    reference's own setters and initialize() by tests/test_interface_sequences.py - are the expectation."""
    by_reference = between not in ("reset", "configure")
    sc = {"between": between} if by_reference else {"between": between, "reference": False}
    piped = both(sc)
    assert piped["stats"]["pipelined"] == 0, piped["stats"]
    if by_reference:
        assert T.reference_lib() is None or piped["reference_frames"] > 0, piped
    else:
        sequential = run(sc, True, {"NFCGPU_WINDOWED": "0"})
        assert sequential["stats"]["windowed"] == 0, sequential["stats"]
        assert piped["frames"] == sequential["frames"]


def test_a_spoilt_shadow_state_is_found_and_the_front_walked_again(emulated):
    """test switch of the emulated / tuning builds: the shadow state of one stream is spoilt, the comparison after the tail finds it
    and the front is walked again from the true state"""
    piped = both({}, {"NFCGPU_TEST_SPOIL_SHADOW": "2"})
    assert piped["stats"]["pipelined"] == 3 and piped["stats"]["refronts"] >= 3, piped["stats"]


def test_a_second_buffer_set_the_device_cannot_give_means_no_overlap(emulated):
    """(NFCGPU_TEST_ALLOC_LIMIT_SECOND: the sibling of NFCGPU_TEST_ALLOC_LIMIT for the planes of the second set alone)"""
    piped = both({}, {"NFCGPU_TEST_ALLOC_LIMIT_SECOND": "65536"})
    assert piped["stats"]["pipelined"] == 0 and piped["stats"]["fallback"] == 0, piped["stats"]
