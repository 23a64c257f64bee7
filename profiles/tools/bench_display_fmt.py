#!/usr/bin/env python3
"""Measurement of the display calls on int16 input (nfcgpu_spectrum_fmt, nfcgpu_resample_radio_fmt with NFCGPU_FMT_I16)
against the float calls, on one GPU, everything resident in HBM (the synthetic streams of bench.py, synth.fill_iq_torch, on
the int16 grid: the int16 pairs and the float pairs hold the same values).

  spectrum    512 buffers x 2^20 I/Q pairs, the shipped parameters (L = 1024, "hamming", D = 16) with hop = L * D
  resampler   512 buffers x 2^16 samples: I/Q (stride 2), and the mono capture (stride 1)

Per shape three ways to the same output:
  float       the float call (nfcgpu_spectrum / nfcgpu_resample_radio) on float values that are already there - what the
              parent commit offers, measured with the parent's library and binding (--parent-pkg: its nfc-laboratory_amd/ directory
              with libnfcgpu.so built) and with this tree's;
  route       what a host holding int16 has to do with the parent: make the floats first - widen (torch, v / 32768) for the
              spectrum and the mono resampler, nfcgpu_magnitude_fmt for the I/Q resampler - then the float call;
  int16       the _fmt call on the int16 bytes where they lie (this tree's library only).

A library is measured in a process of its own; the libraries take turns, parent first, --rounds times. Timing: HIP events on
the context's stream around the calls (which return when the output is complete; the widening runs on the same stream), --reps timed repeats after --warmup; the result keeps every time, the
median and min - max per run, and over all runs of a library. Outputs of the three ways are compared once per run (counts and
bytes), so that the times are times of the same result. Prints one JSON line and, with --out, writes it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "nfc-laboratory_amd")
L, D = 1024, 16
FMT_F32, FMT_I16 = 0, 1


def summary(times):
    s = sorted(times)
    return {"ms": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4), "ms_all": [round(t, 4) for t in times]}


def worker(args):
    import torch
    sys.path.insert(0, args.pkg)
    import nfclab_amd
    import synth

    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    B, P, N = args.buffers, args.pairs, args.samples

    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    f32 = torch.empty((B, P, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(f32, template, first_stream=0, chunk_streams=max(1, min(1024, (1 << 27) // P)))
    i16 = torch.empty((B, P, 2), dtype=torch.int16, device=dev)
    for s in range(0, B, 64):
        i16[s:s + 64] = (f32[s:s + 64] * 32768.0).to(torch.int16)
        assert torch.equal(i16[s:s + 64].to(torch.float32) / 32768.0, f32[s:s + 64])
    wide = torch.empty_like(f32)  # where the route puts its floats

    # resampler input: the first N samples of every buffer
    rs_iq16 = i16[:, :N].contiguous()
    rs_iq32 = f32[:, :N].contiguous()
    rs_mag32 = rs_iq32.abs().sum(dim=-1).contiguous()  # (axis-aligned I/Q, one component is 0: the magnitude, exactly, and on the grid)
    rs_mono16 = (rs_mag32 * 32768.0).to(torch.int16).contiguous()
    assert torch.equal(rs_mono16.to(torch.float32) / 32768.0, rs_mag32)
    rs_wide = torch.empty_like(rs_mag32)
    cap = N + N // 255 + 2
    torch.cuda.synchronize()

    result = {}

    with nfclab_amd.NfcGpu(device=0, max_streams=64) as gpu:
        has_fmt = hasattr(gpu.lib, "nfcgpu_spectrum_fmt") and hasattr(gpu.lib, "nfcgpu_resample_radio_fmt")
        result["has_fmt_calls"] = has_fmt
        stream = torch.cuda.ExternalStream(gpu.hip_stream(), device=dev)

        def timed(call):
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
            return summary(times)

        # ---- spectrum ----
        frames = gpu.spectrum_frames(P, length=L, decimation=D, hop=L * D)
        pitch = frames * L * 4
        outs = {k: torch.zeros((B, frames * L), dtype=torch.float32, device=dev) for k in ("float", "route", "int16")}

        def spectrum_float(src, out):
            gpu.spectrum_device(src.data_ptr(), P * 8, B, P, out.data_ptr(), pitch, length=L, decimation=D, hop=L * D)

        def spectrum_route():
            with torch.cuda.stream(stream):
                torch.div(i16, 32768.0, out=wide)
            spectrum_float(wide, outs["route"])

        def spectrum_i16():
            gpu.spectrum_device(i16.data_ptr(), P * 4, B, P, outs["int16"].data_ptr(), pitch, length=L, decimation=D, hop=L * D, fmt=FMT_I16)

        sp = {"buffers": B, "pairs_per_buffer": P, "length": L, "window": "hamming", "decimation": D, "hop": L * D, "frames": frames * B,
              "input_bytes": {"float": B * P * 8, "int16": B * P * 4}}
        sp["float"] = timed(lambda: spectrum_float(f32, outs["float"]))
        sp["route"] = timed(spectrum_route)
        if has_fmt:
            sp["int16"] = timed(spectrum_i16)
        torch.cuda.synchronize()
        sp["outputs_equal"] = bool(torch.equal(outs["float"], outs["route"]) and (not has_fmt or torch.equal(outs["float"], outs["int16"])))
        result["spectrum"] = sp
        del outs

        # ---- resampler ----
        def buffers_of():
            return torch.zeros((B, 2 * cap), dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)

        def resample_float(src, out, counts):
            gpu.resample_radio_device(src.data_ptr(), N * 4, B, N, out.data_ptr(), 2 * cap * 4, cap, counts.data_ptr())

        rs = {"buffers": B, "samples_per_buffer": N}
        for shape, stride, raw in (("iq", 2, rs_iq16), ("mono", 1, rs_mono16)):
            o = {k: buffers_of() for k in ("float", "route", "int16")}

            def route():
                if stride == 2:
                    gpu._check(gpu.lib.nfcgpu_magnitude_fmt(gpu.ctx, raw.data_ptr(), B * N, rs_wide.data_ptr(), nfclab_amd.LOC_DEVICE, FMT_I16))
                else:
                    with torch.cuda.stream(stream):
                        torch.div(raw, 32768.0, out=rs_wide)
                resample_float(rs_wide, *o["route"])

            def fmt_call():
                gpu.resample_radio_device(raw.data_ptr(), N * 2 * stride, B, N, o["int16"][0].data_ptr(), 2 * cap * 4, cap, o["int16"][1].data_ptr(),
                                          stride=stride, fmt=FMT_I16)

            entry = {"stride": stride, "input_bytes": {"float_magnitudes": B * N * 4, "int16": B * N * 2 * stride},
                     "route_makes_floats_with": "nfcgpu_magnitude_fmt" if stride == 2 else "torch.div(int16, 32768)"}
            entry["float"] = timed(lambda: resample_float(rs_mag32, *o["float"]))
            entry["route"] = timed(route)
            if has_fmt:
                entry["int16"] = timed(fmt_call)
            torch.cuda.synchronize()
            same = torch.equal(o["float"][1], o["route"][1]) and (not has_fmt or torch.equal(o["float"][1], o["int16"][1]))
            # (beyond a buffer's pairs nothing is written: the rows were zero before)
            same = same and torch.equal(o["float"][0], o["route"][0]) and (not has_fmt or torch.equal(o["float"][0], o["int16"][0]))
            entry["outputs_equal"] = bool(same)
            entry["control_points"] = int(o["float"][1].sum().item())
            rs[shape] = entry
        result["resampler"] = rs
        result["device"] = torch.cuda.get_device_name(0)

    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-pkg", default="", help="nfc-laboratory_amd/ of a checkout of the parent commit, libnfcgpu.so built")
    ap.add_argument("--pkg", default=PKG, help=argparse.SUPPRESS)
    ap.add_argument("--parent", default="", help="the parent commit (written into the result)")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.worker:
        return worker(args)

    libs = ([("parent", args.parent_pkg)] if args.parent_pkg else []) + [("this", PKG)]
    runs = {name: [] for name, _ in libs}
    env = {k: v for k, v in os.environ.items() if k != "NFCGPU_LIB"}
    for _ in range(args.rounds):
        for name, pkg in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg", os.path.abspath(pkg), "--buffers", str(args.buffers),
                   "--pairs", str(args.pairs), "--samples", str(args.samples), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=420)
            if proc.returncode != 0:
                # (whatever ended the worker: nothing more is started on the device)
                sys.exit("worker for %s ended with %d" % (name, proc.returncode))
            line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print("%s: done" % name, file=sys.stderr, flush=True)

    def over_runs(name, path):
        times = []
        for run in runs.get(name, []):
            node = run
            for key in path:
                node = node.get(key) if isinstance(node, dict) else None
            if node:
                times += node["ms_all"]
        return summary(times) if times else None

    compare = {}
    for label, path in (("spectrum", ("spectrum",)), ("resampler_iq", ("resampler", "iq")), ("resampler_mono", ("resampler", "mono"))):
        parent_float = over_runs("parent", path + ("float",))
        this_float = over_runs("this", path + ("float",))
        parent_route = over_runs("parent", path + ("route",))
        this_i16 = over_runs("this", path + ("int16",))
        entry = {"parent_float": parent_float, "this_float": this_float, "parent_route": parent_route, "this_route": over_runs("this", path + ("route",)),
                 "this_int16": this_i16}
        base = parent_float or this_float
        if base and this_i16:
            spread = base["ms_max"] - base["ms_min"]
            entry["int16_minus_float_ms"] = round(this_i16["ms"] - base["ms"], 4)
            entry["float_spread_ms"] = round(spread, 4)
            entry["int16_no_slower_than_float_beyond_spread"] = bool(this_i16["ms"] <= base["ms"] + spread)
            route = parent_route or entry["this_route"]
            entry["int16_over_route_time"] = round(this_i16["ms"] / route["ms"], 4)
        compare[label] = entry

    head = ""
    stamp = os.path.join(PKG, "build", "git_head.txt")
    if os.path.exists(stamp):
        head = open(stamp).read().strip()
    result = {"op": "nfcgpu_spectrum_fmt / nfcgpu_resample_radio_fmt on int16 input against the float calls", "git": head, "parent": args.parent,
              "command": "python profiles/tools/bench_display_fmt.py --buffers %d --pairs %d --samples %d --reps %d --warmup %d --rounds %d%s" % (
                  args.buffers, args.pairs, args.samples, args.reps, args.warmup, args.rounds, " --parent-pkg PARENT/nfc-laboratory_amd" if args.parent_pkg else ""),
              "timing": "HIP events on the context's stream around the calls of one way, %d timed repeats after %d warm-up calls per run; the libraries "
                        "take turns in processes of their own, %d runs each; summaries: median, min, max over all repeats of all runs" % (args.reps, args.warmup, args.rounds),
              "summary": compare, "runs": runs}
    line = json.dumps(result, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
