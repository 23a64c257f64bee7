#!/usr/bin/env python3
"""Measurement of nfcgpu_signal_tap on one GPU.

  shapes   buffers resident in HBM (the synthetic streams of bench.py, synth.fill_iq_torch; mono shapes take their magnitudes),
           HIP-event time of the call on the context's stream, median of --reps after --warmup:
             long      1 x 2^24   float mono, all six channels
             many    256 x 2^16   float mono, all six channels (as many samples)
             iq_i16  512 x 2^20   int16 I/Q, ENVELOPE | DEPTH
             iq_f32  512 x 2^20   float I/Q, ENVELOPE | DEPTH
           per shape: ms, GS/s, bytes read (the samples) and written (the planes), their sum over the time as a share of
           nfcgpu_read_bandwidth over the same input on the same card, the call's report (chunks, rounds, chunks walked twice)
           and the chunk and warm-up the library chose.
  decoder  for comparison, the scan_ms nfcgpu_stats reports (profiling on) for a decoder submission of the iq_i16 shape on
           fresh streams: the existing front's walk over the same samples.
  sweep    with --sweep: `long`, `many` and `iq_i16` again with chunk_samples given (warm-up as the library's), what the
           library's choice was measured against.

Prints one JSON line and, with --out, writes it."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfclab_amd  # noqa: E402
import synth  # noqa: E402

FS = 10000000
ALL, ENV_DEPTH = nfclab_amd.TAP_ALL, nfclab_amd.TAP_ENVELOPE | nfclab_amd.TAP_DEPTH


def median(values):
    return sorted(values)[len(values) // 2]


def default_cut(n_buffers, n, rate=FS):
    """the chunk and warm-up nfcgpu_signal_tap chooses (nfcgpu.hip: tap_default_warm, tap_default_chunk), for the record"""
    warm = (rate * 4096 + 9999999) // 10000000
    warm = min(max((warm + 63) & ~63, 64), 8192)
    c = max(n_buffers * n // 65536, 256)
    if n_buffers >= 1024 and c < 2 * warm:
        c = 2 * warm
    c = min(c, (n + 63) & ~63)
    return (c + 63) & ~63, warm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-decoder", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    S, N = args.streams, args.samples

    template = torch.from_numpy(synth.load_template(os.path.join(ROOT, "tests", "golden")).astype(np.int16)).to(dev)
    iq = torch.empty((S, N, 2), dtype=torch.float32, device=dev)
    synth.fill_iq_torch(iq, template, first_stream=0, chunk_streams=max(1, min(256, (1 << 27) // N)))
    iq16 = (iq * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    total_mono = 1 << 24
    rows = max(1, total_mono // N)
    mono = torch.linalg.vector_norm(iq[:rows], dim=2).reshape(-1)[:total_mono].contiguous()
    assert mono.numel() == total_mono
    planes = torch.empty(max(6 * total_mono, 2 * S * N), dtype=torch.float32, device=dev)
    states = torch.zeros((max(S, 256), 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    print("filled %d streams of %d samples" % (S, N), file=sys.stderr, flush=True)

    result = {"op": "nfcgpu_signal_tap", "device": torch.cuda.get_device_name(0)}
    head = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    result["git"] = open(head).read().strip() if os.path.exists(head) else ""

    shapes = {"long": (mono, 1, total_mono, 1, nfclab_amd.FMT_F32, ALL),
              "many": (mono, 256, total_mono // 256, 1, nfclab_amd.FMT_F32, ALL),
              "iq_i16": (iq16, S, N, 2, nfclab_amd.FMT_I16, ENV_DEPTH),
              "iq_f32": (iq, S, N, 2, nfclab_amd.FMT_F32, ENV_DEPTH)}

    sink_words = 64 << 20
    sink = torch.zeros(sink_words, dtype=torch.int32, device=dev)
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)

    with nfclab_amd.NfcGpu(device=0, max_streams=S, frame_sink_bytes=64 << 20) as gpu:
        stream = torch.cuda.ExternalStream(gpu.hip_stream(), device=dev)

        def measure(name, chunk=0, warm=0):
            data, nb, n, stride, fmt, mask = shapes[name]
            sample_bytes = stride * (2 if fmt == nfclab_amd.FMT_I16 else 4)
            k = bin(mask).count("1")

            def call():
                return gpu.signal_tap_device(data.data_ptr(), n * sample_bytes, nb, n, FS, planes.data_ptr(), k * n * 4, n * 4, channels=mask,
                                             stride=stride, fmt=fmt, state_out_ptr=states.data_ptr(), chunk=chunk, warm=warm)

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
            ms = median(times)
            read, written = nb * n * sample_bytes, nb * n * 4 * k
            read_gbs = gpu.read_bandwidth(data.data_ptr(), read, 5)
            gbs = (read + written) / ms / 1e6
            cut = (chunk, warm) if chunk else default_cut(nb, n)
            out = {"buffers": nb, "samples_per_buffer": n, "stride": stride, "format": "i16" if fmt == nfclab_amd.FMT_I16 else "f32", "channels": k,
                   "ms_per_call": round(ms, 3), "ms_all": [round(t, 3) for t in times], "Gsamples_per_s": round(nb * n / ms / 1e6, 2),
                   "bytes_read": read, "bytes_written": written, "GBps": round(gbs, 1), "read_bandwidth_GBps": round(read_gbs, 1),
                   "frac_of_read_bandwidth": round(gbs / read_gbs, 4), "chunk_samples": cut[0], "warm_samples": cut[1],
                   "report": {"chunks": report.chunks, "rounds": report.rounds, "rewalked_chunks": report.rewalked_chunks}}
            print("%s chunk %d warm %d: %.3f ms, %.2f GS/s, %d chunks, %d rounds, %d walked twice" % (
                name, cut[0], cut[1], ms, out["Gsamples_per_s"], report.chunks, report.rounds, report.rewalked_chunks), file=sys.stderr, flush=True)
            return out

        result["timing"] = ("HIP events on the context's stream around the call (which returns when the planes are complete), median of %d "
                            "after %d warm-up calls; read_bandwidth: nfcgpu_read_bandwidth over the shape's input, 5 repeats" % (args.reps, args.warmup))
        result["shapes"] = {name: measure(name) for name in shapes}
        result["default"] = {"walkers_wanted": 65536, "min_chunk": 256, "warm_at_10MSps": 4096,
                             "many_buffers": "1024 buffers or more: chunks of twice the warm-up at least"}

        if args.sweep:
            keep_reps, keep_warm = args.reps, args.warmup
            args.reps, args.warmup = 5, 1
            sweep = {}
            for name, chunks in (("long", (256, 512, 1024, 2048, 4096)), ("many", (256, 512, 1024, 2048, 4096, 16384, 65536)),
                                 ("iq_i16", (4096, 8192, 16384, 65536))):
                sweep[name] = {str(c): {k: v for k, v in measure(name, c, 4096).items() if k in ("ms_per_call", "Gsamples_per_s", "report")} for c in chunks}
            result["sweep"] = sweep
            args.reps, args.warmup = keep_reps, keep_warm

        if not args.no_decoder:
            # the existing front's walk over the samples of iq_i16: a decoder submission on fresh streams, profiling on
            gpu.sink_attach(sink.data_ptr(), sink_words, ctl.data_ptr())
            gpu.sink_hold(True)
            gpu.profile(True)
            first = gpu.open(count=S)
            gpu.stats_reset()
            gpu.submit_uniform(first, S, iq16.data_ptr(), N * 4, N, FS, stride=2, location=nfclab_amd.LOC_DEVICE, fmt=nfclab_amd.FMT_I16)
            gpu.sync()
            st = gpu.stats()
            result["decoder_front"] = {"what": "nfcgpu_submit_uniform_fmt of the iq_i16 shape on fresh streams, profiling on: nfcgpu_stats",
                                       "scan_ms": round(st.scan_ms, 3), "scan_samples": int(st.scan_samples), "planes_ms": round(st.planes_ms, 3),
                                       "scan_repairs": int(st.scan_repairs), "windowed_streams": int(st.windowed_streams)}
            print("decoder front: scan %.3f ms over %d samples" % (st.scan_ms, st.scan_samples), file=sys.stderr, flush=True)
            gpu.profile(False)
            gpu.sink_hold(False)
            gpu.sink_attach(None, 0, None)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
