"""nfcgpu_spectrum_fmt and nfcgpu_resample_radio_fmt on a box without a GPU: tests/test_display_fmt.py run against the
emulated library (tests/hostsim/build_emulated.sh), where the launches of the new kernels are calls of their CPU twins:
the loader of nfc-laboratory_amd/csrc/nfc_spectrum.hpp compiled for int16 pairs, and the tiles, the ring and the
decision loop of nfc_resample.hpp, buffer after buffer (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD). What this covers without
a device: the conversion on load, the arithmetic behind it against the float calls bit for bit, rows, pitches and
alignments, the argument checks, the staging of host input in its own format and the binding.
tests/test_display_fmt.py::test_twins_equal_device ties it to the kernels on the GPU; how a wave stages its 64 rows is
the one thing only the GPU run sees."""
import os
import re
import subprocess
import sys

import pytest

import nfc_testlib as T

EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
SUITE = os.path.join(T.ROOT, "tests", "test_display_fmt.py")


@pytest.fixture(scope="module")
def emulated(built):
    sources = [os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc", f) for f in os.listdir(os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc"))]
    sources += [os.path.join(T.ROOT, "tests", "hostsim", f) for f in ("emu_kernels.cpp", "build_emulated.sh", "fakehip/hip/hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in sources):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    return EMU


def test_display_fmt_suite_on_the_emulated_runtime(emulated):
    env = dict(os.environ, NFCGPU_LIB=emulated, NFCGPU_NO_TORCH="1")
    cmd = [sys.executable, "-m", "pytest", SUITE, "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    run = subprocess.run(cmd, cwd=T.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    tail = run.stdout[-3000:]
    assert run.returncode == 0, tail
    # (test_twins_equal_device needs a device to compare with and skips itself here; the three legs against the reference's task
    # need oracle/_ref)
    expected = 1 if os.path.exists(os.path.join(T.ROOT, "oracle", "_ref", "resample-ref")) else 4
    last = run.stdout.strip().splitlines()[-1]
    assert re.search(r"\b\d+ passed\b", last) and "failed" not in last and "error" not in last, tail
    assert re.findall(r"\b(\d+) skipped\b", last) == [str(expected)], tail
