"""The modulated exchanges through the C ABI on a box without a GPU: tests/test_modulated_gpu.py run against the emulated
library (tests/hostsim/build_emulated.sh: the product's host runtime and device code on a stand-in HIP). The ids that take
every scenario are for the device and are deselected here; see that file's docstring for what goes through on the CPU."""
import os
import subprocess
import sys

import pytest

import nfc_testlib as T

EMU = os.path.join(T.ROOT, "tests", "hostsim", "libnfcgpu_emulated.so")


@pytest.fixture(scope="module")
def emulated(built):
    sources = [os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc", f) for f in os.listdir(os.path.join(T.ROOT, "nfc-laboratory_amd", "csrc"))]
    sources += [os.path.join(T.ROOT, "tests", "hostsim", f) for f in ("emu_kernels.cpp", "build_emulated.sh", "fakehip/hip/hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in sources):
        subprocess.check_call(["bash", os.path.join(T.ROOT, "tests", "hostsim", "build_emulated.sh")])
    return EMU


@pytest.mark.skipif(T.reference_lib() is None, reason="oracle/_ref not built")
def test_modulated_suite_on_the_emulated_runtime(emulated):
    env = dict(os.environ, NFCGPU_LIB=emulated, NFCGPU_NO_TORCH="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(T.ROOT, "tests", "test_modulated_gpu.py"), "-m", "gpu", "-q", "-k", "not everything",
           "-p", "no:cacheprovider"]
    # (the legs are independent of each other: side by side where pytest-xdist is there)
    try:
        import xdist  # noqa: F401
        workers = max(1, min(6, (os.cpu_count() or 2) // 2))
        if workers > 1:
            cmd += ["-n", str(workers)]
    except ImportError:
        pass
    run = subprocess.run(cmd, cwd=T.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=3000)
    tail = run.stdout[-3000:]
    assert run.returncode == 0, tail
    assert "10 passed" in tail and "failed" not in tail and "skipped" not in tail, tail
