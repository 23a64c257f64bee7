"""Pipelined submissions (the front of a submission under the tail of the one before: front / join_front, csrc/nfcgpu.hip) against
the parent commit: bench.py of a built checkout of the parent and of this tree run alternately, parent first, for the default
command and for `--gpus 1 --steps 20 --warmup 5`; and, from rocprofv3 kernel traces of `bench.py --steps 4 --warmup 2`, the
front and the tail of a step and what runs between the end of a step's first decode pass and its nfc_finish_kernel.

  python profiles/tools/bench_pipeline.py --parent-tree DIR [--runs 3] [--commands default,steps20] [--outputs] [--points] [--trace-parent CSV] [--trace CSV] [--out FILE]

--commands: which of the two commands (a visit too short for both takes one at a time; the files are put together afterwards).

--outputs: `bench.py --dump-outputs` for both commands on both trees, frames.npy and frame_payload.npy held against each other
with numpy.array_equal, frames_decoded_rank0 and frames_dropped beside them, and the pipeline counters of this tree per step
(a run of the headline shape through the C ABI: pipelined_submissions, pipeline_refronts, pipeline_zeroed_edges).
--points: `bench.py --full --no-cpu` once on each tree, the points share_dense, single_dense, config5_sparse, s2_config5 and
fixtures_single side by side.

DIR: the parent commit checked out and built (make -C nfc-laboratory_amd). The traces are taken apart from the runs:
  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python bench.py --gpus 1 --steps 4 --warmup 2
Writes profiles/pipelined_submissions.json."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COMMANDS = {"default": [], "steps20": ["--gpus", "1", "--steps", "20", "--warmup", "5"]}


def bench(tree, extra):
    run = subprocess.run([sys.executable, "bench.py"] + extra, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if run.returncode != 0:
        raise SystemExit("bench.py failed in %s: %s" % (tree, run.stderr[-2000:]))
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    cfg = line.get("config", {})
    print("bench.py %s in %s: %s ms per step" % (" ".join(extra), tree, cfg.get("ms_per_step")), file=sys.stderr, flush=True)
    return {"value": line["value"], "ms_per_step": cfg.get("ms_per_step"), "time_parallel": cfg.get("time_parallel"),
            "frames_decoded_rank0": cfg.get("frames_decoded_rank0"), "frames_dropped": cfg.get("frames_dropped")}


def outputs(parent_tree, extra):
    """step 4: the frames of both trees, array for array"""
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "parent"), os.path.join(tmp, "this")
        ra, rb = bench(parent_tree, extra + ["--dump-outputs", a]), bench(ROOT, extra + ["--dump-outputs", b])
        same = {f: bool(np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f)))) for f in ("frames.npy", "frame_payload.npy")}
    return {"equal": same, "frames_decoded_rank0": [ra["frames_decoded_rank0"], rb["frames_decoded_rank0"]], "frames_dropped": [ra["frames_dropped"], rb["frames_dropped"]]}


COUNTERS = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(sys.argv[1], "nfc-laboratory_amd"))
import nfclab_amd, synth
S, L, K, FS = 4096, 1 << 20, int(sys.argv[2]), 10000000
dev = torch.device("cuda", 0)
template = synth.load_template(os.path.join(sys.argv[1], "tests", "golden"))
data = torch.empty((S, 2 * L, 2), dtype=torch.float32, device=dev)
synth.fill_iq_torch(data, torch.from_numpy(template.astype(np.int16)).to(dev), first_stream=0, chunk_streams=16)
words = 256 << 20
sink = torch.zeros(words, dtype=torch.int32, device=dev); ctl = torch.zeros(4, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
gpu = nfclab_amd.NfcGpu(device=0, max_streams=S, frame_sink_bytes=1 << 20)
gpu.sink_attach(sink.data_ptr(), words, ctl.data_ptr()); gpu.sink_hold(True)
first = gpu.open(nfclab_amd.default_params(), count=S)
for k in range(K):
    gpu.submit_uniform(first, S, data.data_ptr() + (k % 2) * L * 8, 2 * L * 8, L, FS, stride=2)
gpu.sync(); torch.cuda.synchronize()
st = gpu.stats()
print(json.dumps({"steps": K, "pipelined_submissions": int(st.pipelined_submissions), "pipeline_refronts": int(st.pipeline_refronts),
                  "pipeline_zeroed_edges": int(st.pipeline_zeroed_edges), "fallback_streams": int(st.fallback_streams)}))
gpu.close()
"""


def counters(steps=6):
    run = subprocess.run([sys.executable, "-c", COUNTERS, ROOT, str(steps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if run.returncode != 0:
        raise SystemExit("the counters run failed: %s" % run.stderr[-2000:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def points(tree):
    run = subprocess.run([sys.executable, "bench.py", "--full", "--no-cpu"], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=3000)
    if run.returncode != 0:
        raise SystemExit("bench.py --full failed in %s: %s" % (tree, run.stderr[-2000:]))
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    found = line.get("config", {}).get("points", line.get("points", {}))
    return {name: found.get(name) for name in ("share_dense", "single_dense", "config5_sparse", "s2_config5", "fixtures_single")}


def spread(runs, key):
    v = [r[key] for r in runs if r[key] is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)} if v else None


def steps_of_trace(path):
    """per step of a kernel trace (CSV of rocprofv3 --kernel-trace): the front (first front kernel to the first launch of the
    step's first decode pass), the tail (end of that pass's longest launch to the end of nfc_finish_kernel), and the front
    kernels of the NEXT step that start inside this tail - ms"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]))
    rows.sort()
    front_names = ("nfc_scan_kernel", "nfc_envelope_kernel", "nfc_scan_planes_kernel", "nfc_seams_kernel", "nfc_tiles_kernel")
    finishes = [r for r in rows if r[2].startswith("nfc_finish_kernel")]
    out, after = [], 0
    for fin in finishes:
        # the step's launches of the wave decoder lie between the finish before and this one; the first pass holds the longest
        waves = [r for r in rows if r[2].startswith("nfc_wave_kernel") and after <= r[0] < fin[0]]
        if not waves:
            continue
        longest = max(waves, key=lambda r: r[1] - r[0])
        first_wave = min(r[0] for r in waves)
        fronts = [r for r in rows if r[2].startswith(front_names) and r[0] < first_wave and r[0] >= (out[-1]["_pass0_end"] if out else 0)]
        inside = [r for r in rows if r[2].startswith(front_names) and longest[1] <= r[0] < fin[1]]
        out.append({"front_ms": (first_wave - min(r[0] for r in fronts)) / 1e6 if fronts else None,
                    "pass0_ms": (longest[1] - longest[0]) / 1e6, "tail_ms": (fin[1] - longest[1]) / 1e6,
                    "next_front_kernels_inside_tail": sorted({r[2] for r in inside}),
                    "next_front_ms_inside_tail": (max(r[1] for r in inside) - min(r[0] for r in inside)) / 1e6 if inside else 0.0,
                    "_pass0_end": longest[1]})
        after = fin[1]
    for o in out:
        del o["_pass0_end"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commands", default=",".join(COMMANDS))
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--trace-parent", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipelined_submissions.json"))
    args = ap.parse_args()

    commands = {name: COMMANDS[name] for name in args.commands.split(",")}
    result = {"op": "front of submission k+1 under the tail of submission k (pipelined submissions) against the parent commit"}

    if args.parent_tree:
        for name, extra in commands.items():
            runs = {"parent": [], "this": []}
            for _ in range(args.runs):
                runs["parent"].append(bench(args.parent_tree, extra))
                runs["this"].append(bench(ROOT, extra))
            result[name] = {"command": "python bench.py " + " ".join(extra), "runs": runs,
                            "parent": {k: spread(runs["parent"], k) for k in ("value", "ms_per_step")},
                            "this": {k: spread(runs["this"], k) for k in ("value", "ms_per_step")}}

    if args.parent_tree and args.outputs:
        result["outputs"] = {name: outputs(args.parent_tree, extra) for name, extra in commands.items()}
        result["counters_headline_shape"] = counters()

    if args.parent_tree and args.points:
        result["points"] = {"parent": points(args.parent_tree), "this": points(ROOT)}

    for key, path in (("trace_parent", args.trace_parent), ("trace_this", args.trace)):
        if path:
            result[key] = steps_of_trace(path)

    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
