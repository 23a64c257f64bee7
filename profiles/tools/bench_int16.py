#!/usr/bin/env python3
"""Measurement of int16 input (NFCGPU_FMT_I16) against float input holding the same values, on one GPU.

  device   S streams of L I/Q samples resident in HBM (the synthetic streams of bench.py, synth.fill_iq_torch: the headline's
           data), once as float32 pairs and once as the int16 pairs they convert from (value * 32768, exact: the data is on the
           int16 grid). A step is one nfcgpu_submit_uniform[_fmt] of all streams plus the wait for it (nfcgpu_sync), wall time,
           the two formats alternately on stream sets of their own that have seen the same samples; median of --reps steps after
           --warmup. The default shape is the headline's, 4096 x 2^20; --streams / --samples make it smaller where that does not fit
           (the line says which shape was run).
  host     H streams of M I/Q samples in host memory, submitted with NFCGPU_LOC_HOST: the copy into pinned staging and the upload
           count. A replay host that holds a capture file starts from int16; for the float calls it first has to widen it,
           astype(float32) / 32768 (one numpy pass on one core, timed on its own: `widen_ms`), then submit twice the bytes.

Prints one JSON line and, with --out, writes it. The words of frame records the two formats leave in the sink are compared (the
frames themselves are compared by tests/test_int16_input.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
import nfclab_amd  # noqa: E402
import synth  # noqa: E402

FS = 10000000


def median(values):
    return sorted(values)[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--host-streams", type=int, default=256)
    ap.add_argument("--host-samples", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default="", help="commit the change is measured against (written into the result)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    S, L, H, M = args.streams, args.samples, args.host_streams, args.host_samples
    F32, I16 = nfclab_amd.FMT_F32, nfclab_amd.FMT_I16

    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    f32 = torch.empty((S, L, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(f32, template, first_stream=0, chunk_streams=max(1, min(1024, (1 << 27) // L)))
    i16 = torch.empty((S, L, 2), dtype=torch.int16, device=dev)
    for s in range(0, S, 256):
        i16[s:s + 256] = (f32[s:s + 256] * 32768.0).to(torch.int16)
        # the same values: the float data is on the int16 grid
        assert torch.equal(i16[s:s + 256].to(torch.float32) / 32768.0, f32[s:s + 256])
    torch.cuda.synchronize()
    print("filled %d streams of %d samples in both formats" % (S, L), file=sys.stderr, flush=True)

    steps = args.warmup + args.reps
    sink_words = max(16 << 20, 2 * steps * (1024 * S * max(1, L >> 20) + 65536))
    sink = torch.zeros(sink_words, dtype=torch.int32, device=dev)
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    result = {"op": "int16 input against float input, the same values", "parent": args.parent, "device": torch.cuda.get_device_name(0)}
    head = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    result["git"] = open(head).read().strip() if os.path.exists(head) else ""

    with nfclab_amd.NfcGpu(device=0, max_streams=2 * max(S, H), frame_sink_bytes=1 << 20) as gpu:
        gpu.sink_attach(sink.data_ptr(), sink_words, ctl.data_ptr())
        gpu.sink_hold(True)
        first = {F32: gpu.open(count=S), I16: gpu.open(count=S)}

        def device_step(fmt):
            data, size = (f32, 8) if fmt == F32 else (i16, 4)
            t0 = time.perf_counter()
            gpu.submit_uniform(first[fmt], S, data.data_ptr(), L * size, L, FS, stride=2, location=nfclab_amd.LOC_DEVICE, fmt=fmt)
            gpu.sync()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        times = {F32: [], I16: []}
        frames = {F32: 0, I16: 0}
        paths = {}
        for k in range(steps):
            for fmt in (F32, I16):
                gpu.stats_reset()
                before = int(ctl[0].item())
                ms = device_step(fmt)
                st = gpu.stats()
                if k >= args.warmup:
                    times[fmt].append(ms)
                    frames[fmt] += int(ctl[0].item()) - before  # words of frame records the step appended to the held sink
                paths[fmt] = [int(st.windowed_streams), int(st.fallback_streams)]
        dropped = int(ctl[1].item())
        shape = {"streams": S, "samples_per_stream": L, "stride": 2,
                 "shape": "the headline's (4096 x 2^20)" if (S, L) == (4096, 1 << 20) else "smaller than the headline's 4096 x 2^20",
                 "timing": "wall time of nfcgpu_submit_uniform[_fmt] + nfcgpu_sync, formats alternately, median of %d steps after %d" % (args.reps, args.warmup),
                 "frames_dropped": dropped}
        for fmt, name, size in ((F32, "f32", 8), (I16, "i16", 4)):
            ms = median(times[fmt])
            shape[name] = {"ms_per_step": round(ms, 3), "ms_all": [round(t, 3) for t in times[fmt]], "Msamples_per_s": round(S * L / ms / 1e3, 1),
                           "resident_bytes": S * L * size, "frame_record_words": frames[fmt], "windowed_fallback_streams_last_step": paths[fmt]}
        shape["i16_over_f32_throughput"] = round(median(times[F32]) / median(times[I16]), 4)
        shape["frame_record_words_equal"] = frames[F32] == frames[I16]
        result["device_resident"] = shape
        print("device: f32 %.2f ms, i16 %.2f ms per step" % (median(times[F32]), median(times[I16])), file=sys.stderr, flush=True)

        for fmt in (F32, I16):
            for s in range(S):
                gpu.close_stream(first[fmt] + s)
        gpu.sync()
        gpu.sink_rewind()

        # ---- host-resident: what a replay host holds is int16 ----
        host_i16 = np.ascontiguousarray(i16[:H, :M].cpu().numpy())
        first = {F32: gpu.open(count=H), I16: gpu.open(count=H)}
        widen, times = [], {F32: [], I16: []}
        for k in range(steps):
            t0 = time.perf_counter()
            host_f32 = host_i16.astype(np.float32) / np.float32(32768.0)
            widen_ms = (time.perf_counter() - t0) * 1e3
            for fmt in (F32, I16):
                data, size = (host_f32, 8) if fmt == F32 else (host_i16, 4)
                t0 = time.perf_counter()
                gpu.submit_uniform(first[fmt], H, data.ctypes.data, M * size, M, FS, stride=2, location=nfclab_amd.LOC_HOST, fmt=fmt)
                gpu.sync()
                ms = (time.perf_counter() - t0) * 1e3
                if k >= args.warmup:
                    times[fmt].append(ms)
            if k >= args.warmup:
                widen.append(widen_ms)
            gpu.sink_rewind()
        shape = {"streams": H, "samples_per_stream": M, "stride": 2,
                 "timing": "wall time of nfcgpu_submit_uniform[_fmt] with NFCGPU_LOC_HOST + nfcgpu_sync, formats alternately, median of %d steps after %d; "
                           "widen_ms: numpy astype(float32) / 32768 of the int16 rows on one core, what a host does before it can call the float entry" % (args.reps, args.warmup),
                 "widen_ms": round(median(widen), 3), "widen_ms_all": [round(t, 3) for t in widen]}
        for fmt, name, size in ((F32, "f32", 8), (I16, "i16", 4)):
            ms = median(times[fmt])
            shape[name] = {"ms_per_step": round(ms, 3), "ms_all": [round(t, 3) for t in times[fmt]], "Msamples_per_s": round(H * M / ms / 1e3, 1),
                           "bytes_uploaded": H * M * size}
        shape["f32_with_widening"] = {"ms_per_step": round(median(times[F32]) + median(widen), 3),
                                      "Msamples_per_s": round(H * M / (median(times[F32]) + median(widen)) / 1e3, 1)}
        shape["i16_over_f32_throughput"] = round(median(times[F32]) / median(times[I16]), 4)
        shape["i16_over_f32_with_widening_throughput"] = round((median(times[F32]) + median(widen)) / median(times[I16]), 4)
        result["host_resident"] = shape

    result["command"] = "python profiles/tools/bench_int16.py --streams %d --samples %d --host-streams %d --host-samples %d --reps %d --warmup %d" % (
        S, L, H, M, args.reps, args.warmup)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
