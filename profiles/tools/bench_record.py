#!/usr/bin/env python3
"""Measurement of nfcgpu_record on one GPU, and of the live flow it opens.

  throughput  B buffers of N float I/Q samples resident in HBM (the synthetic streams of bench.py, synth.fill_iq_torch, times
              0.83 plus noise of sigma 0.002 per component, so that nothing lies on the int16 grid), HIP-event time of the
              call on the context's stream, median of --reps after --warmup, for MAGNITUDE with levels, MAGNITUDE without and
              SAME with levels. Bytes moved = 8 read + 2 (MAGNITUDE) or 4 (SAME) written per sample, over the time, as a
              fraction of nfcgpu_read_bandwidth over the same input on the same box and of the 8 TB/s the rooflines here use.
  live flow   S streams of N such samples: record (MAGNITUDE, with levels) + nfcgpu_submit_uniform_fmt (I16) of the recording
              against nfcgpu_submit_uniform of the floats, each with the wait for it (nfcgpu_sync), wall time, the two flows
              alternately on stream sets of their own that have seen the same samples; median of --reps steps after --warmup.
              Then eight streams of each flow, on fresh streams, against the reference decoder (oracle/_ref/libnfcref.so, when
              it is there) on that flow's own input: the recorded values / 32768 for the one, the magnitudes of the floats
              (nfcgpu_magnitude) for the other.

Prints one JSON line and, with --out, writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfclab_amd  # noqa: E402
import synth  # noqa: E402

FS = 10000000
HBM_PEAK_GBS = 8000.0  # the figure bench.py's rooflines use


def median(values):
    return sorted(values)[len(values) // 2]


def data_frames(frames):
    return [f for f in frames if f[1] in (0x102, 0x103)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compare", type=int, default=8, help="streams of each flow compared with the reference decoder")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    B, N, S = args.buffers, args.samples, args.streams
    assert S <= B
    SAME, MAGNITUDE = nfclab_amd.RECORD_SAME, nfclab_amd.RECORD_MAGNITUDE

    # S distinct streams, off the grid; the buffers beyond them repeat those (the record kernels do not care what they read)
    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    iq = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(iq[:S], template, first_stream=0, chunk_streams=max(1, min(256, (1 << 27) // N)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261017)
    for s in range(0, S, 64):
        block = iq[s:s + 64]
        block.mul_(0.83).add_(torch.randn(block.shape, generator=gen, device=dev, dtype=torch.float32), alpha=0.002)
    for s in range(S, B, S):
        iq[s:s + S] = iq[:min(S, B - s)]
    torch.cuda.synchronize()
    print("filled %d buffers of %d samples" % (B, N), file=sys.stderr, flush=True)

    pcm = torch.empty((B, 2 * N), dtype=torch.int16, device=dev)
    levels = torch.zeros((B, 4), dtype=torch.float32, device=dev)
    result = {"op": "nfcgpu_record", "device": torch.cuda.get_device_name(0)}
    head = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    result["git"] = open(head).read().strip() if os.path.exists(head) else ""

    steps = args.warmup + args.reps
    sink_words = max(16 << 20, 4 * steps * (1024 * S * max(1, N >> 20) + 65536))
    sink = torch.zeros(sink_words, dtype=torch.int32, device=dev)
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    with nfclab_amd.NfcGpu(device=0, max_streams=2 * S + 4 * args.compare, frame_sink_bytes=64 << 20) as gpu:
        stream = torch.cuda.ExternalStream(gpu.hip_stream(), device=dev)

        # ---- throughput ----
        read_gbs = gpu.read_bandwidth(iq.data_ptr(), iq.numel() * 4, 5)
        shapes = {}
        for name, mode, with_levels, out_bytes in (("magnitude_levels", MAGNITUDE, True, 2), ("magnitude", MAGNITUDE, False, 2),
                                                   ("same_levels", SAME, True, 4)):
            def call():
                gpu.record_device(iq.data_ptr(), N * 8, B, N, pcm.data_ptr(), N * out_bytes, stride=2, mode=mode,
                                  levels_ptr=levels.data_ptr() if with_levels else None)

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
            ms = median(times)
            moved = B * N * (8 + out_bytes)
            gbs = moved / ms / 1e6
            shapes[name] = {"ms_per_call": round(ms, 3), "ms_all": [round(t, 3) for t in times], "Gsamples_per_s": round(B * N / ms / 1e6, 2),
                            "bytes_moved": moved, "GBps": round(gbs, 1), "frac_of_read_bandwidth": round(gbs / read_gbs, 4),
                            "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            print("%s: %.3f ms per call, %.0f GB/s" % (name, ms, gbs), file=sys.stderr, flush=True)
        result["throughput"] = {"buffers": B, "samples_per_buffer": N, "stride": 2, "read_bandwidth_GBps": round(read_gbs, 1),
                                "read_bandwidth": "nfcgpu_read_bandwidth over the same input, 5 repeats", "hbm_peak_GBps": HBM_PEAK_GBS,
                                "timing": "HIP events on the context's stream around the call (which returns when the output is complete), "
                                          "median of %d after %d warm-up calls" % (args.reps, args.warmup),
                                "shapes": shapes}

        # ---- the live flow ----
        gpu.sink_attach(sink.data_ptr(), sink_words, ctl.data_ptr())
        gpu.sink_hold(True)
        first = {"recorded": gpu.open(count=S), "floats": gpu.open(count=S)}

        def flow_step(flow):
            t0 = time.perf_counter()
            if flow == "recorded":
                gpu.record_device(iq.data_ptr(), N * 8, S, N, pcm.data_ptr(), N * 2, stride=2, mode=MAGNITUDE, levels_ptr=levels.data_ptr())
                record_ms = (time.perf_counter() - t0) * 1e3
                gpu.submit_uniform(first[flow], S, pcm.data_ptr(), N * 2, N, FS, stride=1, location=nfclab_amd.LOC_DEVICE, fmt=nfclab_amd.FMT_I16)
            else:
                record_ms = 0.0
                gpu.submit_uniform(first[flow], S, iq.data_ptr(), N * 8, N, FS, stride=2, location=nfclab_amd.LOC_DEVICE)
            gpu.sync()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, record_ms

        times = {"recorded": [], "floats": []}
        record_part, words, paths = [], {"recorded": 0, "floats": 0}, {"recorded": [], "floats": []}
        for k in range(steps):
            for flow in ("recorded", "floats"):
                gpu.stats_reset()
                before = int(ctl[0].item())
                ms, rec = flow_step(flow)
                st = gpu.stats()
                if k >= args.warmup:
                    times[flow].append(ms)
                    words[flow] += int(ctl[0].item()) - before
                    if flow == "recorded":
                        record_part.append(rec)
                    paths[flow].append([int(st.windowed_streams), int(st.fallback_streams)])
        live = {"streams": S, "samples_per_stream": N, "frames_dropped": int(ctl[1].item()),
                "timing": "wall time of the flow's calls + nfcgpu_sync, flows alternately, median of %d steps after %d" % (args.reps, args.warmup)}
        for flow in ("recorded", "floats"):
            ms = median(times[flow])
            live[flow] = {"ms_per_step": round(ms, 3), "ms_all": [round(t, 3) for t in times[flow]], "Gsamples_per_s": round(S * N / ms / 1e6, 3),
                          "frame_record_words": words[flow], "windowed_fallback_streams_per_step": paths[flow]}
        live["recorded"]["record_ms_of_it"] = round(median(record_part), 3)
        live["recorded_over_floats_throughput"] = round(median(times["floats"]) / median(times["recorded"]), 3)
        print("live: recorded %.2f ms, floats %.2f ms per step" % (median(times["recorded"]), median(times["floats"])), file=sys.stderr, flush=True)

        for flow in first:
            for s in range(S):
                gpu.close_stream(first[flow] + s)
        gpu.sync()
        gpu.sink_rewind()
        gpu.sink_hold(False)
        gpu.sink_attach(None, 0, None)

        # ---- eight streams of each flow against the reference on that flow's own input ----
        import nfc_testlib as T
        C = min(args.compare, S)
        compare = {"streams": C, "reference": "oracle/_ref/libnfcref.so" if T.reference_lib() is not None else None}
        if T.reference_lib() is not None and C:
            gpu.record_device(iq.data_ptr(), N * 8, C, N, pcm.data_ptr(), N * 2, stride=2, mode=MAGNITUDE, levels_ptr=levels.data_ptr())
            sid = gpu.open(count=C)
            gpu.submit_uniform(sid, C, pcm.data_ptr(), N * 2, N, FS, stride=1, location=nfclab_amd.LOC_DEVICE, fmt=nfclab_amd.FMT_I16)
            recorded = [data_frames(gpu.poll(sid + s, capacity=16384)) for s in range(C)]
            fid = gpu.open(count=C)
            gpu.submit_uniform(fid, C, iq.data_ptr(), N * 8, N, FS, stride=2, location=nfclab_amd.LOC_DEVICE)
            floats = [data_frames(gpu.poll(fid + s, capacity=16384)) for s in range(C)]
            host_pcm = pcm.view(-1)[:C * N].view(C, N).cpu().numpy()  # (rows N samples apart)
            host_iq = iq[:C].cpu().numpy()
            equal = {"recorded": 0, "floats": 0}
            frames = {"recorded": 0, "floats": 0, "same_between_flows": 0}
            for s in range(C):
                want_r, _ = T.reference_decode(host_pcm[s].astype(np.float32) / np.float32(32768), cap=16384)
                want_f, _ = T.reference_decode(gpu.magnitude(host_iq[s].reshape(-1)), cap=16384)
                equal["recorded"] += recorded[s] == want_r
                equal["floats"] += floats[s] == want_f
                frames["recorded"] += len(recorded[s])
                frames["floats"] += len(floats[s])
                frames["same_between_flows"] += recorded[s] == floats[s]
            compare.update({"streams_equal_to_the_reference": equal, "frames": frames,
                            "levels_of_stream_0": [float(v) for v in levels[0, :3].cpu()] + [int(levels[0, 3:].view(torch.int32).item())]})
        live["against_the_reference"] = compare
        result["live_flow"] = live

    result["command"] = "python profiles/tools/bench_record.py --buffers %d --samples %d --streams %d --reps %d --warmup %d" % (
        B, N, S, args.reps, args.warmup)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
