#!/usr/bin/env python3
"""Measurement of nfcgpu_signal_tap_reduce on one GPU.

  shapes   buffers resident in HBM (the synthetic streams of bench.py, as profiles/tools/bench_tap.py makes them), HIP-event time
           of the call on the context's stream, median of --reps after --warmup:
             many         256 x 2^16   float mono, all six channels, bins of 1024
             iq_i16       512 x 2^20   int16 I/Q, ENVELOPE | DEPTH, bins of 4096; scratch_bytes 0: all planes at once
             iq_i16_slabs the same with scratch_bytes = 1 GiB: four slabs of 128 buffers, each with the tap's rounds of its own
             frames       the input of iq_i16, 10^5 ranges of 900 ... 1100 samples anywhere in it, in device memory, in no order
           per shape: the whole call; nfcgpu_signal_tap with NFCGPU_LOC_DEVICE on the same input into planes of the caller (what the
           same caller runs today before reducing the planes itself); their difference, which is the reduce stage with whatever the
           slabs add to the tap; the bytes the reduce kernels read (4 bytes per sample of every range and channel) over that
           difference as a share of nfcgpu_read_bandwidth over the same input.
  host     `many` once more from host memory: the whole call against nfcgpu_signal_tap with NFCGPU_LOC_HOST, planes and all, which
           is what a caller whose samples are in host memory pays today (wall clock: the copies are the host's).

  kernels  the reduce stage alone. The difference above is a few hundred microseconds between two calls of tens or hundreds of
           milliseconds, so the kernels' own times come from a second, short run of this tool under a kernel trace
           (rocprofv3 --kernel-trace --output-format csv -- python bench_tap_reduce.py --reps 2 --warmup 1 --no-host --out TRACED.json)
           and are merged into the first run's file without a GPU: --merge-trace KERNEL_TRACE.csv --traced TRACED.json --out FILE.
           Per shape: the dispatches of nfc_tap_reduce_kernel and nfc_tap_reduce_finish_kernel of a call (one of each per slab)
           summed, the median over the traced calls, and the bytes the reduce kernels read over the reduce kernel's time as a share
           of the first run's nfcgpu_read_bandwidth.

Prints one JSON line and, with --out, writes it."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfclab_amd  # noqa: E402
import synth  # noqa: E402

FS = 10000000
ALL, ENV_DEPTH = nfclab_amd.TAP_ALL, nfclab_amd.TAP_ENVELOPE | nfclab_amd.TAP_DEPTH
SEGMENT = 16384


def median(values):
    return sorted(values)[len(values) // 2]


def merge_trace(trace_csv, traced_json, out_json):
    """the kernels' times of a traced run into the file of the measured one"""
    with open(out_json) as f:
        result = json.load(f)
    with open(traced_json) as f:
        traced = json.load(f)
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    spans = {kernel: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if r["Kernel_Name"].startswith(kernel + "(")]
             for kernel in ("nfc_tap_reduce_kernel", "nfc_tap_reduce_finish_kernel")}
    first = next(r for r in rows if r["Kernel_Name"].startswith("nfc_tap_reduce_kernel("))
    result["kernels"] = {"what": "rocprofv3 --kernel-trace of a run with %d calls per shape; microseconds per call, median" % traced["calls_per_shape"],
                         "nfc_tap_reduce_kernel": {"vgpr": int(first["VGPR_Count"]), "accum_vgpr": int(first["Accum_VGPR_Count"]), "sgpr": int(first["SGPR_Count"]),
                                                   "lds_bytes": int(first["LDS_Block_Size"]), "scratch_bytes": int(first["Scratch_Size"])}}
    at = 0
    for name, shape in traced["shapes"].items():
        calls, slabs = traced["calls_per_shape"], shape["slabs"]
        per_call = {kernel: [sum(v[at + c * slabs:at + (c + 1) * slabs]) for c in range(calls)] for kernel, v in spans.items()}
        at += calls * slabs
        us = median(per_call["nfc_tap_reduce_kernel"])
        into = result["shapes"][name]
        into["reduce_kernel_us"] = round(us, 1)
        into["finish_kernel_us"] = round(median(per_call["nfc_tap_reduce_finish_kernel"]), 1)
        into["reduce_kernel_GBps"] = round(into["bytes_reduced"] / us / 1e3, 1)
        into["reduce_kernel_frac_of_read_bandwidth"] = round(into["bytes_reduced"] / us / 1e3 / into["read_bandwidth_GBps"], 3)
    assert at == len(spans["nfc_tap_reduce_kernel"]) == len(spans["nfc_tap_reduce_finish_kernel"]), "the trace is not of that run"
    line = json.dumps(result)
    print(line)
    with open(out_json, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--ranges", type=int, default=100000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--traced", default=None)
    args = ap.parse_args()

    if args.merge_trace:
        return merge_trace(args.merge_trace, args.traced, args.out)

    import torch

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    S, N = args.streams, args.samples

    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    iq = torch.empty((S, N, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(iq, template, first_stream=0, chunk_streams=max(1, min(256, (1 << 27) // N)))
    iq16 = (iq * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    total_mono = min(1 << 24, S * N)
    rows = max(1, total_mono // N)
    mono = torch.linalg.vector_norm(iq[:rows], dim=2).reshape(-1)[:total_mono].contiguous()
    del iq
    planes = torch.empty(max(6 * total_mono, 2 * S * N), dtype=torch.float32, device=dev)
    states = torch.zeros((max(S, 256), 8), dtype=torch.int32, device=dev)

    rng = np.random.default_rng(1)
    frames = np.zeros(args.ranges, dtype=nfclab_amd.TAP_RANGE_DTYPE)
    frames["buffer"] = rng.integers(0, S, args.ranges)
    frames["count"] = rng.integers(900, 1101, args.ranges)
    frames["first"] = rng.integers(0, N - 1100, args.ranges)
    d_frames = torch.from_numpy(frames.view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    print("filled %d streams of %d samples" % (S, N), file=sys.stderr, flush=True)

    result = {"op": "nfcgpu_signal_tap_reduce", "device": torch.cuda.get_device_name(0)}
    head = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    result["git"] = open(head).read().strip() if os.path.exists(head) else ""

    nb_many = 256
    shapes = {"many": (mono, nb_many, total_mono // nb_many, 1, nfclab_amd.FMT_F32, ALL, 1024, None, 0),
              "iq_i16": (iq16, S, N, 2, nfclab_amd.FMT_I16, ENV_DEPTH, 4096, None, 0),
              "iq_i16_slabs": (iq16, S, N, 2, nfclab_amd.FMT_I16, ENV_DEPTH, 4096, None, 1 << 30),
              "frames": (iq16, S, N, 2, nfclab_amd.FMT_I16, ENV_DEPTH, 0, frames, 0)}
    most_records = max(6 * nb_many * -(-(total_mono // nb_many) // 1024), 2 * S * -(-N // 4096), 2 * args.ranges)
    records = torch.zeros(most_records * 32, dtype=torch.uint8, device=dev)

    with nfclab_amd.NfcGpu(device=0, max_streams=64) as gpu:
        stream = torch.cuda.ExternalStream(gpu.hip_stream(), device=dev)

        def timed(call):
            for _ in range(args.warmup):
                call()
            times, report = [], None
            for _ in range(args.reps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                report = call()
                end.record(stream)
                end.synchronize()
                times.append(start.elapsed_time(end))
            return median(times), [round(t, 3) for t in times], report

        def measure(name):
            data, nb, n, stride, fmt, mask, bin_samples, ranges, scratch = shapes[name]
            sample_bytes = stride * (2 if fmt == nfclab_amd.FMT_I16 else 4)
            k = bin(mask).count("1")

            def reduce():
                return gpu.signal_tap_reduce_device(data.data_ptr(), n * sample_bytes, nb, n, FS, records.data_ptr(), channels=mask,
                                                    ranges_ptr=None if ranges is None else d_frames.data_ptr(), n_ranges=0 if ranges is None else ranges.size,
                                                    bin_samples=bin_samples, stride=stride, fmt=fmt, state_out_ptr=states.data_ptr(), scratch_bytes=scratch)

            def tap():
                return gpu.signal_tap_device(data.data_ptr(), n * sample_bytes, nb, n, FS, planes.data_ptr(), k * n * 4, n * 4, channels=mask,
                                             stride=stride, fmt=fmt, state_out_ptr=states.data_ptr())

            ms, ms_all, report = timed(reduce)
            tap_ms, tap_all, tap_report = timed(tap)
            if ranges is None:
                n_ranges, reduced, segments = nb * -(-n // bin_samples), nb * n * k * 4, nb * -(-n // bin_samples) * -(-min(bin_samples, n) // SEGMENT)
            else:
                n_ranges, reduced = ranges.size, int(ranges["count"].astype(np.int64).sum()) * k * 4
                segments = int((-(-ranges["count"].astype(np.int64) // SEGMENT)).sum())
            read_gbs = gpu.read_bandwidth(data.data_ptr(), nb * n * sample_bytes, 5)
            stage = ms - tap_ms
            per_buffer = ((n * 4 + 255) & ~255) * k
            slabs = -(-nb // max(1, scratch // per_buffer)) if scratch else 1
            out = {"buffers": nb, "samples_per_buffer": n, "stride": stride, "format": "i16" if fmt == nfclab_amd.FMT_I16 else "f32", "channels": k,
                   "bin_samples": bin_samples, "ranges": n_ranges, "records": n_ranges * k, "units": segments * k, "scratch_bytes": scratch, "slabs": slabs,
                   "ms_per_call": round(ms, 3), "ms_all": ms_all, "tap_device_ms": round(tap_ms, 3), "tap_device_ms_all": tap_all,
                   "reduce_stage_ms_by_difference": round(stage, 3), "bytes_reduced": reduced,
                   "reduce_GBps_by_difference": round(reduced / stage / 1e6, 1) if stage > 0 else None, "read_bandwidth_GBps": round(read_gbs, 1),
                   "frac_of_read_bandwidth_by_difference": round(reduced / stage / 1e6 / read_gbs, 4) if stage > 0 else None,
                   "report": {"chunks": report.chunks, "rounds": report.rounds, "rewalked_chunks": report.rewalked_chunks},
                   "tap_report": {"chunks": tap_report.chunks, "rounds": tap_report.rounds, "rewalked_chunks": tap_report.rewalked_chunks}}
            print("%s: call %.3f ms, tap alone %.3f ms, difference %.3f ms" % (name, ms, tap_ms, stage), file=sys.stderr, flush=True)
            return out

        result["timing"] = ("HIP events on the context's stream around the call (which returns when the records are complete), median of %d after %d "
                            "warm-up calls; read_bandwidth: nfcgpu_read_bandwidth over the shape's input, 5 repeats" % (args.reps, args.warmup))
        result["calls_per_shape"] = args.warmup + args.reps
        result["shapes"] = {name: measure(name) for name in shapes}

        if not args.no_host:
            data, nb, n, stride, fmt, mask, bin_samples, _, _ = shapes["many"]
            host_rows = data.reshape(nb, n).cpu().numpy()

            def wall(call):
                for _ in range(args.warmup):
                    call()
                times = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    times.append((time.perf_counter() - t0) * 1e3)
                return round(median(times), 3), [round(t, 3) for t in times]

            plane = (n * 4 + 15) & ~15
            out_planes = np.zeros((nb, 6, plane // 4), dtype=np.float32)
            out_states = np.zeros(nb, dtype=nfclab_amd.TAP_STATE_DTYPE)
            out_records = np.zeros((nb * -(-n // bin_samples), 6), dtype=nfclab_amd.TAP_STAT_DTYPE)
            p, q = nfclab_amd.TapParams(FS, mask, 0, 0), nfclab_amd.TapReduceParams(bin_samples, 0, 0)

            def host_tap():
                gpu._check(gpu.lib.nfcgpu_signal_tap(gpu.ctx, host_rows.ctypes.data, n * 4, nb, n, 1, fmt, p, None, out_planes.ctypes.data, 6 * plane, plane,
                                                     out_states.ctypes.data, None, nfclab_amd.LOC_HOST))

            def host_reduce():
                gpu._check(gpu.lib.nfcgpu_signal_tap_reduce(gpu.ctx, host_rows.ctypes.data, n * 4, nb, n, 1, fmt, p, q, None, None, 0, out_records.ctypes.data,
                                                            out_states.ctypes.data, None, nfclab_amd.LOC_HOST))

            reduce_ms, reduce_all = wall(host_reduce)
            tap_ms, tap_all = wall(host_tap)
            result["host"] = {"shape": "many", "timing": "wall clock of the call, median of %d after %d" % (args.reps, args.warmup),
                              "reduce_ms": reduce_ms, "reduce_ms_all": reduce_all, "tap_host_ms": tap_ms, "tap_host_ms_all": tap_all,
                              "bytes_in": nb * n * 4, "bytes_out_reduce": int(out_records.nbytes), "bytes_out_tap": nb * n * 4 * 6}
            print("host: reduce %.3f ms, tap with its planes %.3f ms" % (reduce_ms, tap_ms), file=sys.stderr, flush=True)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
