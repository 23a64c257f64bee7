"""nfcgpu_record on a box without a GPU: tests/test_record.py run against the emulated library
(tests/hostsim/build_emulated.sh), where the launches of the record kernels are calls of their CPU twins: the quads,
lanes, waves and segments of nfc-laboratory_amd/csrc/nfc_record.hpp, the text the device kernels compile, as loops
(nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD). What this covers without a device: the quantiser, the levels and the order of
their sums, rows, pitches and the argument checks, the binding, the capture files against the reference's writer and
the decoding of a recording. tests/test_record.py::test_twin_equals_device ties it to the kernels on the GPU; how the
device packs its stores is the one thing only the GPU run sees.

The second test hands recordings to the reference's own reader: its test-sdr harness opens the files nfcgpu_wav_write
made with hw::RecordDevice, decodes them and compares the frames with the goldens."""
import os
import shutil
import subprocess
import sys

import pytest

import nfc_testlib as T

EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
SUITE = os.path.join(T.ROOT, "tests", "test_record.py")


@pytest.fixture(scope="module")
def emulated(built):
    sources = [os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc", f) for f in os.listdir(os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc"))]
    sources += [os.path.join(T.ROOT, "tests", "hostsim", f) for f in ("emu_kernels.cpp", "build_emulated.sh", "fakehip/hip/hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in sources):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    return EMU


def test_record_suite_on_the_emulated_runtime(emulated):
    env = dict(os.environ, NFCGPU_LIB=emulated, NFCGPU_NO_TORCH="1")
    cmd = [sys.executable, "-m", "pytest", SUITE, "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    run = subprocess.run(cmd, cwd=T.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    tail = run.stdout[-3000:]
    assert run.returncode == 0, tail
    # (test_twin_equals_device needs a device to compare with and skips itself here; the off-grid decode leg needs oracle/_ref)
    skipped = "1 skipped" if T.reference_lib() is not None else "2 skipped"
    assert " passed" in tail and "failed" not in tail and skipped in tail, tail


def test_the_reference_reads_and_decodes_what_was_recorded(emulated, tmp_path):
    exe = os.path.join(T.ROOT, "oracle", "_ref", "test-sdr-ref")
    if not os.path.exists(exe):
        pytest.skip("test-sdr-ref not built (needs the reference tree at build time)")
    names = ["test_NFC-A_106kbps_001", "test_POLL_ABF_001"]
    env = dict(os.environ, NFCGPU_LIB=emulated, NFCGPU_NO_TORCH="1", PYTHONPATH=os.path.join(T.ROOT, "tests"))
    run = subprocess.run([sys.executable, SUITE, "--write-wavs", str(tmp_path)] + names, cwd=T.ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:]
    for name in names:
        shutil.copyfile(os.path.join(T.GOLDEN, "wav", name + ".json"), tmp_path / (name + ".json"))
    out = subprocess.run([exe, str(tmp_path) + "/"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900).stdout
    for name in names:
        assert "TEST FILE %s.wav: PASS" % name in out, out
