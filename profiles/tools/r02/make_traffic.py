#!/usr/bin/env python3
"""HBM bytes per launch of the two roofline kernels from the rocprofv3 counter passes of round_profile.sh.
usage: make_traffic.py <gpurun_out/tag>   ->  <dir>/pmc_hbm_traffic.json and profiles/traffic.json

FETCH_SIZE / WRITE_SIZE are in KiB. The calibration kernels (profiles/tools/calib_traffic.hip) read and write 8 GiB with
known byte counts; the ratio known / reported is applied to the kernels' counters (on gfx950 FETCH_SIZE reports half the
bytes of dword-per-lane reads, WRITE_SIZE is exact: MI355X_MICROARCH.md, HBM section)."""
import collections
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def counters(d):
    """[(kernel, grid, counter, value)] in dispatch order"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r.get("Dispatch_Id", 0)), r["Kernel_Name"].split("(")[0], int(r.get("Grid_Size", 0) or 0), r["Counter_Name"], float(r["Counter_Value"])))
    rows.sort()
    return rows


def main():
    out = sys.argv[1]
    CAL_BYTES = float(1 << 33)
    calib = {}
    for c, kern in (("FETCH_SIZE", "read_rows"), ("WRITE_SIZE", "write_rows")):
        vals = [v for (_, k, _, n, v) in counters(os.path.join(out, "calib_" + c)) if n == c and kern in k]
        calib[c] = CAL_BYTES / (vals[-1] * 1024.0) if vals else None

    result = {"round": 2, "command": "profiles/tools/r02/round_profile.sh: rocprofv3 --kernel-trace --pmc FETCH_SIZE (and, separately, WRITE_SIZE) -- "
                                      "python bench.py --full --no-cpu --steps 2 --warmup 1 --points config5_idle; no other trace domains",
              "calibration": {"tool": "profiles/tools/calib_traffic.hip (8 GiB read, 8 GiB written)", "fetch_size_factor": calib["FETCH_SIZE"],
                              "write_size_factor": calib["WRITE_SIZE"]}, "kernels": {}}

    shapes = {"nfc_demod_fixed_kernel": (131072, 8192), "nfc_scan_kernel": (4096, 1 << 20)}
    per = collections.defaultdict(dict)
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        rows = counters(os.path.join(out, "pmc_" + c))
        for kern in shapes:
            mine = [(g, v) for (_, k, g, n, v) in rows if n == c and k == kern]
            if not mine:
                continue
            biggest = max(g for g, _ in mine)
            full = [v for g, v in mine if g == biggest]   # launches over the whole submission (not the re-walks of single chunks)
            per[kern][c] = {"dispatches": len(full), "grid": biggest, "last_KiB": full[-1], "mean_KiB": sum(full) / len(full)}

    try:
        git = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip() or None
    except Exception:
        git = None
    sys.path.insert(0, ROOT)
    import bench
    digest = bench.sources_digest()

    traffic = {}
    for kern, (streams, samples) in shapes.items():
        if "FETCH_SIZE" not in per[kern] or "WRITE_SIZE" not in per[kern] or not calib["FETCH_SIZE"] or not calib["WRITE_SIZE"]:
            continue
        rd = per[kern]["FETCH_SIZE"]["last_KiB"] * 1024.0 * calib["FETCH_SIZE"]
        wr = per[kern]["WRITE_SIZE"]["last_KiB"] * 1024.0 * calib["WRITE_SIZE"]
        alg = 8.0 * streams * samples
        result["kernels"][kern] = {"streams": streams, "samples": samples, "raw": per[kern], "hbm_read_bytes_per_launch": rd,
                                   "hbm_write_bytes_per_launch": wr, "hbm_bytes_per_launch": rd + wr, "algorithmic_bytes_per_launch": alg,
                                   "ratio_traffic_to_algorithmic": (rd + wr) / alg}
        traffic[kern] = {"streams": streams, "samples": samples, "hbm_bytes_per_launch": rd + wr, "sources_sha1": digest, "git": git,
                         "from": "profiles/r02/pmc_hbm_traffic.json"}

    json.dump(result, open(os.path.join(out, "pmc_hbm_traffic.json"), "w"), indent=1)
    json.dump(traffic, open(os.path.join(out, "traffic.json"), "w"), indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
