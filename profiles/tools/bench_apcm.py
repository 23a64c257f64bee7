#!/usr/bin/env python3
"""Measurement of nfcgpu_apcm_encode on one GPU.

Input: the output of nfcgpu_resample_radio, resident in HBM, for --streams x --samples samples in buffers of --buffer samples,
16 buffers to an entry, of three signals:
  flat     a constant: a point every 255 samples beside the run-in and run-out of every buffer
  dense    a signal whose every sample is a control point
  capture  the NFC-A capture of the test vectors, tiled
Per signal: HIP-event time of nfcgpu_apcm_encode (NFCGPU_LOC_DEVICE) on the context's stream, median of --reps after --warmup;
the same for the resampler call that made the input; the bytes the encoder moves (8 per pair and 4 per count read, the entries
written) over its time, as a share of nfcgpu_read_bandwidth over the pair rows on the same card.

Prints one JSON line and, with --out, writes it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nfc-laboratory_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfclab_amd  # noqa: E402
import nfc_testlib as T  # noqa: E402

FS = 10000000
GROUP = 16


def median(values):
    return sorted(values)[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--buffer", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    dev = torch.device("cuda:0")
    n = args.buffer
    nb = args.streams * args.samples // n
    assert nb % GROUP == 0
    n_entries = nb // GROUP
    cap = n + n // 255 + 2
    entry_pitch = (32 + 3 * GROUP * cap + 3) & ~3

    samples = torch.empty(nb * n, dtype=torch.float32, device=dev)
    pairs = torch.empty((nb, 2 * cap), dtype=torch.float32, device=dev)
    counts = torch.zeros(nb, dtype=torch.int32, device=dev)
    out = torch.zeros((n_entries, entry_pitch), dtype=torch.uint8, device=dev)
    info = torch.zeros((n_entries, 4), dtype=torch.int32, device=dev)

    def fill(kind):
        if kind == "flat":
            samples.fill_(0.5)
        elif kind == "dense":
            i = torch.arange(nb * n, device=dev)
            samples.copy_(torch.where(i % 2 == 0, 0.2, 0.8) + (i % 7).to(torch.float32) * 0.01)
        else:
            x = torch.from_numpy(T.load_fixture("test_NFC-A_106kbps_001")).to(dev)
            samples.copy_(x.repeat(-(-nb * n // x.numel()))[:nb * n])
        torch.cuda.synchronize()

    result = {"op": "nfcgpu_apcm_encode", "device": torch.cuda.get_device_name(0), "buffers": nb, "samples_per_buffer": n, "buffers_per_entry": GROUP,
              "entries": n_entries, "capacity_pairs": cap}
    head = os.path.join(ROOT, "nfc-laboratory_amd", "build", "git_head.txt")
    result["git"] = open(head).read().strip() if os.path.exists(head) else ""

    with nfclab_amd.NfcGpu(device=0, max_streams=64) as gpu:
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
            return median(times), [round(t, 3) for t in times]

        def resample():
            gpu.resample_radio_device(samples.data_ptr(), n * 4, nb, n, pairs.data_ptr(), 2 * cap * 4, cap, counts.data_ptr())

        def encode():
            gpu.apcm_encode_device(pairs.data_ptr(), 2 * cap * 4, counts.data_ptr(), nb, cap, FS, out.data_ptr(), entry_pitch, entry_pitch, info.data_ptr(),
                                   buffers_per_entry=GROUP, buffer_samples=n)

        result["timing"] = ("HIP events on the context's stream around the call (which returns when the entries are complete), median of %d after %d "
                            "warm-up calls; read_bandwidth: nfcgpu_read_bandwidth over the pair rows, 5 repeats" % (args.reps, args.warmup))
        result["signals"] = {}
        for kind in ("flat", "dense", "capture"):
            fill(kind)
            resample_ms, resample_all = timed(resample)
            ms, ms_all = timed(encode)
            got = info.cpu().numpy().view(np.uint32)
            total_pairs = int(counts.cpu().numpy().astype(np.int64).sum())
            assert int(got[:, 1].astype(np.int64).sum()) == total_pairs and not got[:, 2].any()
            moved = 8 * total_pairs + 4 * nb + int(got[:, 0].astype(np.int64).sum())
            read_gbs = gpu.read_bandwidth(pairs.data_ptr(), nb * 2 * cap * 4, 5)
            result["signals"][kind] = {"pairs": total_pairs, "entry_bytes": int(got[:, 0].astype(np.int64).sum()), "bytes_moved": moved,
                                       "encode_ms": round(ms, 3), "encode_ms_all": ms_all, "resample_ms": round(resample_ms, 3), "resample_ms_all": resample_all,
                                       "encode_GBps": round(moved / ms / 1e6, 1), "read_bandwidth_GBps": round(read_gbs, 1),
                                       "frac_of_read_bandwidth": round(moved / ms / 1e6 / read_gbs, 4)}
            print("%s: %d pairs, encode %.3f ms, resample %.3f ms" % (kind, total_pairs, ms, resample_ms), file=sys.stderr, flush=True)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
