"""Driver of tests/test_pipelined_submissions_emulated.py (run in a subprocess: the library under test and its switches come
from the environment). Several submissions of the same streams through nfcgpu_submit_uniform without a synchronisation in
between - the front of one then runs under the pending tail of the one before (run_windowed, nfcgpu.hip) - with one call of
the C ABI between two of them if the scenario names one.

argv[1]: a JSON object {"streams": "dense" | "sparse" | "offgrid", "count": streams, "samples": per submission, "submissions": n,
"fmt": "f32" | "i16", "location": "host" | "device", "between": name of the call or null, "reference": bool}.
Prints one JSON object: the frames per stream (as the poll returns them), whether they are the reference decoder's, the statistics."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))

import numpy as np

import nfc_testlib as T
import nfclab_amd
import synth

FS = 10000000


def make_streams(kind, count, total):
    template = synth.load_template(os.path.join(ROOT, "tests", "golden"))
    if kind == "sparse":
        segs = synth.sparse_segments(template)
        return [synth.sparse_magnitude_f32(template, segs, s, 0, total) for s in range(count)]
    streams = [synth.magnitude_f32(template, 29 + 7 * s, 0, total) for s in range(count)]
    if kind == "offgrid":
        streams = [(m * np.float32(1.0000153)).astype(np.float32) for m in streams]
    return streams


def main():
    sc = json.loads(sys.argv[1])
    count, n, subs = sc["count"], sc["samples"], sc["submissions"]
    fmt = nfclab_amd.FMT_I16 if sc.get("fmt") == "i16" else nfclab_amd.FMT_F32
    location = nfclab_amd.LOC_HOST if sc.get("location") == "host" else nfclab_amd.LOC_DEVICE
    between = sc.get("between")

    streams = make_streams(sc["streams"], count, n * subs)

    if fmt == nfclab_amd.FMT_I16:
        rows = np.stack([np.round(m * 32768.0).astype(np.int16) for m in streams])
        streams = [(r.astype(np.float32) / np.float32(32768.0)).astype(np.float32) for r in rows]
    else:
        rows = np.stack(streams)

    rows = np.ascontiguousarray(rows)
    pitch = rows.strides[0]
    item = rows.itemsize
    others = np.ascontiguousarray(rows[:2, :n])  # rows of a submission over another stream range

    with nfclab_amd.NfcGpu(device=0, max_streams=64) as gpu:
        first = gpu.open(count=count)
        extra = gpu.open(count=2)
        log = []
        early = {}  # frames polled before the end, per stream

        for k in range(subs):
            gpu.submit_uniform(first, count, rows.ctypes.data + k * n * item, pitch, n, FS, stride=1, location=location, fmt=fmt)

            if between is None or k + 1 == subs:
                continue

            if between == "poll":
                polled = gpu.poll(first, capacity=65536)
                log.append(len(polled))
                early.setdefault(0, []).extend(polled)
            elif between == "flush":
                # (the flush completes the pending tail, collects the frames and queues a carrier frame of its own behind them: that
                # one is taken out here, so that what is left can be held against the reference)
                gpu.flush(first + 1)
                polled = gpu.poll(first + 1, capacity=65536)
                log.append(list(polled[-1][:5]))
                early.setdefault(1, []).extend(polled[:-1])
            elif between == "pending":
                cnt = nfclab_amd.ctypes.c_uint32()
                gpu._check(gpu.lib.nfcgpu_pending(gpu.ctx, first, nfclab_amd.ctypes.byref(cnt)), allow=())
                log.append(cnt.value)
            elif between == "stats":
                log.append(int(gpu.stats().windowed_streams))
            elif between == "reset":
                gpu.reset(first)
            elif between == "configure":
                p = nfclab_amd.default_params()
                p.corr_threshold[0] = 0.8
                p.min_modulation_depth[1] = 0.12
                gpu.configure(first + 1, p)
            elif between == "reopen":
                gpu.close_stream(first + count - 1)
                again = gpu.open(count=1)
                assert again == first + count - 1, (again, first, count)
            elif between == "other_range":
                gpu.submit_uniform(extra, 2, others.ctypes.data, others.strides[0], n, FS, stride=1, location=location, fmt=fmt)
            elif between == "sequential":
                # (shorter than the shortest submission the time-parallel path takes: the sequential kernels)
                short = np.ascontiguousarray(rows[:, k * n:k * n + 1024])
                gpu.submit_uniform(first, count, short.ctypes.data, short.strides[0], 1024, FS, stride=1, location=location, fmt=fmt)
            elif between == "sink_rewind":
                # (the synchronisation is what completes the pending tail here and collects the frames; the rewind then finds the
                # sink drained and nothing pending - called with frames in the sink it would discard them)
                gpu.sync()
                gpu.sink_rewind()
            else:
                raise SystemExit("unknown call between submissions: %r" % between)

        got = [early.get(i, []) + gpu.poll(first + i, capacity=65536) for i in range(count)]
        more = [gpu.poll(extra + i, capacity=65536) for i in range(2)]
        st = gpu.stats()

    out = {"frames": [[list(f) if isinstance(f, tuple) else f for f in g] for g in got + more], "log": log,
           "total": sum(len(g) for g in got),
           "stats": {"pipelined": int(st.pipelined_submissions), "refronts": int(st.pipeline_refronts), "windowed": int(st.windowed_streams),
                     "fallback": int(st.fallback_streams)}}

    if sc.get("reference"):
        # what the reference decoder is given: the samples each stream was really fed, in order
        fed = [m for m in streams]
        fed_more = []
        if between == "sequential":
            fed = [np.concatenate([np.concatenate([m[k * n:(k + 1) * n], m[k * n:k * n + 1024]]) if k + 1 < subs else m[k * n:(k + 1) * n] for k in range(subs)])
                   for m in streams]
        elif between == "reopen":
            fed[count - 1] = streams[count - 1][(subs - 1) * n:]  # closed and opened again before the last submission: a new decoder, its frames alone
        elif between == "other_range":
            fed_more = [np.concatenate([streams[i][:n]] * (subs - 1)) for i in range(2)]
        ref = lambda m: T.reference_decode(np.ascontiguousarray(m, dtype=np.float32), sample_rate=FS, keep_carrier=True, cap=65536, defined_storage=True)[0]
        want = [ref(m) for m in fed]
        out["mismatching"] = [i for i in range(count) if got[i] != want[i]]
        out["mismatching"] += [count + i for i, m in enumerate(fed_more) if more[i] != ref(m)]
        out["reference_frames"] = sum(len(w) for w in want)

    print(json.dumps(out, default=str))


if __name__ == "__main__":
    main()
