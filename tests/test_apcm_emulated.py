"""nfcgpu_apcm_encode on a box without a GPU: tests/test_apcm.py run against the emulated library
(tests/hostsim/build_emulated.sh), where the launches of the three kernels are calls of their CPU twins: the units, parts, bases,
windows and the staging area of nfc-laboratory_amd/csrc/nfc_apcm.hpp, the text the device kernels compile, as loops (nfcgpu.hip,
NFCGPU_EMULATED_TEST_BUILD). What this covers without a device: the quantiser and the offset cast, the range, the merge of parts
across chunks, buffers and empty buffers, the header and the results, how a staging area is written out dword by dword and byte
by byte, the capacity rule, the staging of host memory, the argument checks and the binding. tests/test_apcm.py::
test_twin_equals_device ties it to the kernels on the GPU."""
import os
import subprocess
import sys

import pytest

import nfc_testlib as T

EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")
SUITE = os.path.join(T.ROOT, "tests", "test_apcm.py")


@pytest.fixture(scope="module")
def emulated(built):
    sources = [os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc", f) for f in os.listdir(os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc"))]
    sources += [os.path.join(T.ROOT, "tests", "hostsim", f) for f in ("emu_kernels.cpp", "build_emulated.sh", "fakehip/hip/hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in sources):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    return EMU


def test_apcm_suite_on_the_emulated_runtime(emulated):
    env = dict(os.environ, NFCGPU_LIB=emulated, NFCGPU_NO_TORCH="1")
    cmd = [sys.executable, "-m", "pytest", SUITE, "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    run = subprocess.run(cmd, cwd=T.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    tail = run.stdout[-3000:]
    assert run.returncode == 0, tail
    # (test_twin_equals_device needs a device to compare with and skips itself here)
    assert " passed" in tail and "failed" not in tail and "1 skipped" in tail, tail
