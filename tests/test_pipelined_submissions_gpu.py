"""Pipelined submissions on the GPU, at size and with default knobs: four submissions of the same streams without a
synchronisation in between - every submission after the first runs its front under the tail of the one before (run_windowed,
nfcgpu.hip) - EVERY stream compared frame by frame with the reference decoder (tests/parity_sweep_driver.py as it is), and the
same calls on libnfcgpu_tuning.so with NFCGPU_PIPELINE=0 and 1: the same frames per stream, every field and the payload."""
import json
import os
import subprocess
import sys

import pytest

import nfc_testlib as T

DRIVER = os.path.join(T.ROOT, "tests", "parity_sweep_driver.py")
TUNING = os.path.join(T.ROOT, "nfc-laboratory_amd", "libnfcgpu_tuning.so")

pytestmark = pytest.mark.gpu

# S dense streams x L samples x K submissions through the C ABI, no synchronisation in between; prints the frames per stream
# (every field and the payload, in the order of the sink per stream) as a digest, and the statistics
AB = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(sys.argv[1], "nfc-laboratory_amd")); sys.path.insert(0, sys.argv[1])
import nfclab_amd, synth, frames as framelib
S, L, K, FS = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), 10000000
dev = torch.device("cuda", 0)
template = synth.load_template(os.path.join(sys.argv[1], "tests", "golden"))
data = torch.empty((S, K * L, 2), dtype=torch.float32, device=dev)
synth.fill_iq_torch(data, torch.from_numpy(template.astype(np.int16)).to(dev), first_stream=0, chunk_streams=max(1, min(1024, (1 << 26) // (K * L))))
words = 64 << 20
sink = torch.zeros(words, dtype=torch.int32, device=dev); ctl = torch.zeros(4, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
gpu = nfclab_amd.NfcGpu(device=0, max_streams=max(64, S), frame_sink_bytes=1 << 20)
gpu.sink_attach(sink.data_ptr(), words, ctl.data_ptr()); gpu.sink_hold(True)
first = gpu.open(nfclab_amd.default_params(), count=S)
for k in range(K):
    gpu.submit_uniform(first, S, data.data_ptr() + k * L * 8, K * L * 8, L, FS, stride=2)
gpu.sync(); torch.cuda.synchronize()
st = gpu.stats()
used = int(ctl[0].item())
got = framelib.parse_sink(sink[:used].cpu().numpy(), used, FS)
digest = hashlib.sha256()
frames = 0
for stream in sorted(got):
    frames += len(got[stream])
    digest.update(repr((stream, got[stream])).encode())
print(json.dumps({"frames": frames, "dropped": int(ctl[1].item()), "rows": digest.hexdigest(), "streams": len(got),
                  "pipelined": int(st.pipelined_submissions), "refronts": int(st.pipeline_refronts),
                  "windowed": int(st.windowed_streams), "fallback": int(st.fallback_streams)}))
gpu.close()
"""


def _sweep(kind, streams, samples, submissions):
    run = subprocess.run([sys.executable, DRIVER, kind, str(streams), str(samples), str(submissions)], env=dict(os.environ), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=3000)
    assert run.returncode == 0, run.stderr[-3000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    assert res["streams_compared"] == streams and res["streams_mismatching"] == [], res
    assert res["frames_dropped"] == 0 and res["reference_frames"] > 0, res
    return res


def _ab(pipeline, streams=512, samples=1 << 19, submissions=4):
    env = dict(os.environ, NFCGPU_LIB=TUNING, NFCGPU_PIPELINE=str(pipeline))
    run = subprocess.run([sys.executable, "-c", AB, T.ROOT, str(streams), str(samples), str(submissions)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=1500)
    assert run.returncode == 0, run.stderr[-3000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return res


def test_dense_streams_in_four_submissions_match_the_reference(built):
    _sweep("dense", 512, 1 << 20, 4)


def test_modulated_streams_in_four_submissions_match_the_reference(built):
    _sweep("modulated", 512, 1 << 19, 4)


def test_the_same_frames_with_the_pipeline_off_and_on_and_the_overlap_taken(built):
    off, on = _ab(0), _ab(1)
    assert off["pipelined"] == 0 and off["refronts"] == 0, off
    assert on["pipelined"] >= 3, on
    assert on["dropped"] == 0 and on["frames"] > 0, on
    assert (on["frames"], on["streams"], on["rows"]) == (off["frames"], off["streams"], off["rows"]), (off, on)
