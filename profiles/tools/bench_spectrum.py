#!/usr/bin/env python3
"""Measurement of nfcgpu_spectrum on one GPU: N IQ buffers of P pairs resident in HBM (the synthetic streams of bench.py,
synth.fill_iq_torch), HIP-event time of the call on the context's stream after a warm-up, for two shapes:

  waterfall   the defaults (L = 1024, "hamming", D = 16) with hop = L * D: every frame the reference's gather allows side by
              side, 64 frames per buffer of 2^20 pairs (the waterfall of BASELINE config 5's input). The gather reads 32
              contiguous bytes out of every 512.
  dense       D = 1, hop = L: every sample transformed once.

Bytes used = 8 L read + 4 L written per frame. Bytes moved come from the counters, which need runs of their own:

  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d DIR/pmc_FETCH_SIZE -o run --output-format csv -- python bench_spectrum.py --counter-run
  (the same with WRITE_SIZE, and both again around profiles/tools/calib_traffic.hip into DIR/calib_FETCH_SIZE, DIR/calib_WRITE_SIZE)
  python bench_spectrum.py --counters DIR

FETCH_SIZE / WRITE_SIZE are in KiB and are corrected by known / reported of the calibration kernels (dword-per-lane reads and
writes of 8 GiB), as profiles/tools/r04/make_traffic.py does. The counter runs may use fewer buffers (--counter-buffers): what is
written down is bytes per frame.

Beside it numpy.fft in complex64 on one host core over a sample of the same frames (gather, window, FFT, magnitude, swap), labelled
as what it is: the reference's task itself cannot be timed where no binary of it is. Prints one JSON line and, with --out, writes it."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
import nfclab_amd  # noqa: E402
import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # the figure bench.py's rooflines use
L = 1024
SHAPES = {"waterfall": {"decimation": 16, "hop": L * 16}, "dense": {"decimation": 1, "hop": L}}
KERNEL = "nfc_spectrum_kernel_1024"


def counters(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((r["Kernel_Name"].split("(")[0], int(r.get("Grid_Size", 0) or 0), r["Counter_Name"], float(r["Counter_Value"])))
    return rows


def moved_bytes(directory):
    """Per shape: calibrated HBM bytes per frame from the counter runs under `directory` (None where a run is missing)."""
    result = {"calibration": {}, "shapes": {}}
    for c, kern in (("FETCH_SIZE", "read_rows"), ("WRITE_SIZE", "write_rows")):
        vals = [v for (k, _, n, v) in counters(os.path.join(directory, "calib_" + c)) if n == c and kern in k]
        result["calibration"][c] = float(1 << 33) / (vals[-1] * 1024.0) if vals else None
    meta_path = os.path.join(directory, "counter_run.json")
    meta = json.load(open(meta_path)) if os.path.exists(meta_path) else None
    if meta is None:
        return result
    for i, name in enumerate(meta["order"]):
        entry = {"buffers": meta["buffers"], "frames": meta["frames"][name]}
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            # each counter run launches the kernel once per shape, in meta["order"]
            vals = [v for (k, _, n, v) in counters(os.path.join(directory, "pmc_" + c)) if n == c and KERNEL in k]
            factor = result["calibration"][c]
            if len(vals) == len(meta["order"]) and factor:
                entry[c + "_KiB"] = vals[i]
                entry[c.lower() + "_bytes_per_frame"] = vals[i] * 1024.0 * factor / entry["frames"]
        result["shapes"][name] = entry
    return result


def numpy_frames_per_s(iq_host, decimation, hop, frames):
    """numpy on one core: what FourierProcessTask::process() does per frame, vectorised over the sample."""
    n = np.arange(L)
    w = (np.sin((np.pi * n / L).astype(np.float32)).astype(np.float64) ** 2).astype(np.float32)
    src = 4 * decimation * (n >> 2) + (n & 3)
    z = np.ascontiguousarray(iq_host).view(np.complex64)[..., 0]
    assert z.dtype == np.complex64
    t0 = time.perf_counter()
    count = 0
    for b in range(z.shape[0]):
        idx = (np.arange(frames) * hop)[:, None] + src[None, :]
        x = z[b][idx] * w[None, :]
        spectrum = np.fft.fftshift(np.abs(np.fft.fft(x, axis=1)), axes=1)
        assert spectrum.dtype == np.float32
        count += frames
    return count / (time.perf_counter() - t0), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counter-run", action="store_true", help="one call per shape and nothing else (to be run under rocprofv3 --pmc)")
    ap.add_argument("--counter-buffers", type=int, default=1024)
    ap.add_argument("--counters", default=None, help="directory with the counter runs")
    ap.add_argument("--numpy-buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    buffers = args.counter_buffers if args.counter_run else args.buffers
    pairs = args.pairs

    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    iq = torch.empty((buffers, pairs, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(iq, template, first_stream=0, chunk_streams=256)
    torch.cuda.synchronize()
    print("filled %d buffers of %d pairs" % (buffers, pairs), file=sys.stderr, flush=True)

    shapes = {}
    with nfclab_amd.NfcGpu(device=0, max_streams=64) as gpu:
        stream = torch.cuda.ExternalStream(gpu.hip_stream(), device=dev)
        frames_of = {name: gpu.spectrum_frames(pairs, length=L, **p) for name, p in SHAPES.items()}
        out = torch.empty((buffers, max(frames_of.values()) * L), dtype=torch.float32, device=dev)

        if args.counter_run:
            for name, p in SHAPES.items():
                gpu.spectrum_device(iq.data_ptr(), pairs * 8, buffers, pairs, out.data_ptr(), frames_of[name] * L * 4, length=L, **p)
            directory = os.environ.get("SPECTRUM_COUNTER_DIR")
            if directory:
                with open(os.path.join(directory, "counter_run.json"), "w") as f:
                    json.dump({"order": list(SHAPES), "buffers": buffers, "frames": {k: v * buffers for k, v in frames_of.items()}}, f)
            return

        for name, p in SHAPES.items():
            frames = frames_of[name]
            pitch = frames * L * 4

            def call():
                gpu.spectrum_device(iq.data_ptr(), pairs * 8, buffers, pairs, out.data_ptr(), pitch, length=L, **p)

            for _ in range(args.warmup):
                call()
            times = []
            for _ in range(args.reps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                call()
                end.record(stream)
                end.synchronize()
                times.append(start.elapsed_time(end))
            ms = sorted(times)[len(times) // 2]
            total = frames * buffers
            used = total * L * 12
            shapes[name] = {"length": L, "window": "hamming", "decimation": p["decimation"], "hop": p["hop"], "buffers": buffers,
                            "pairs_per_buffer": pairs, "frames": total, "ms_per_call": round(ms, 3), "ms_all": [round(t, 3) for t in times],
                            "frames_per_s": round(total / ms * 1e3, 1), "bytes_used": used,
                            "used_gbs": round(used / ms / 1e6, 1), "used_frac_of_hbm_peak": round(used / ms / 1e6 / HBM_PEAK_GBS, 4)}
            print("%s: %.3f ms per call" % (name, ms), file=sys.stderr, flush=True)

            host = iq[:args.numpy_buffers].cpu().numpy()
            sample = min(frames, 256)
            rate, count = numpy_frames_per_s(host, p["decimation"], p["hop"], sample)
            shapes[name]["cpu_baseline"] = {"value": round(rate, 1), "unit": "frames/s", "cores": 1, "kind": "numpy",
                                            "sample": "numpy.fft.fft in complex64 with gather, window, abs and fftshift, %d frames of the same input" % count}

    if args.counters:
        moved = moved_bytes(args.counters)
        for name, entry in moved["shapes"].items():
            if name not in shapes:
                continue
            rd, wr = entry.get("fetch_size_bytes_per_frame"), entry.get("write_size_bytes_per_frame")
            shapes[name]["counters"] = entry
            if rd is not None and wr is not None:
                moved_per_frame = rd + wr
                shapes[name]["bytes_moved_per_frame"] = round(moved_per_frame, 1)
                shapes[name]["bytes_used_per_frame"] = L * 12
                shapes[name]["moved_over_used"] = round(moved_per_frame / (L * 12), 3)
                ms = shapes[name]["ms_per_call"]
                gbs = moved_per_frame * shapes[name]["frames"] / ms / 1e6
                shapes[name]["roofline"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4)}
        calibration = moved["calibration"]
    else:
        calibration = None

    head = ""
    stamp = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    if os.path.exists(stamp):
        head = open(stamp).read().strip()
    result = {"op": "nfcgpu_spectrum", "git": head, "command": "python profiles/tools/bench_spectrum.py --buffers %d --pairs %d --reps %d --warmup %d%s" % (
                  args.buffers, args.pairs, args.reps, args.warmup, " --counters DIR (counter runs on %d buffers, see the tool's text)" % args.counter_buffers if args.counters else ""),
              "timing": "HIP events on the context's stream around the call (which returns when the output is complete), median of %d after %d warm-up calls" % (args.reps, args.warmup),
              "counter_calibration": {"tool": "profiles/tools/calib_traffic.hip (8 GiB read, 8 GiB written, one dword per lane)", "factors": calibration},
              "device": torch.cuda.get_device_name(0), "shapes": shapes}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
