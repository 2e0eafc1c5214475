"""Condense the profiler output of tools/two_part_profile.py runs:  python tools/two_part_summary.py DIR [--drop 10]

DIR holds one sub-directory per run (any name), each with the files rocprofv3 wrote (-d) and the run's own JSON line as run.json.
Per run: mean and standard deviation of the query_kernel_r launches in the kernel trace (the first --drop launches left out), or the
counters per read (summed over a dispatch's rows, averaged over the dispatches)."""
import argparse
import collections
import csv
import glob
import json
import os
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--drop", type=int, default=10)
    a = ap.parse_args()
    out = {}
    for run in sorted(glob.glob(os.path.join(a.dir, "*", ""))):
        tag = os.path.basename(os.path.dirname(run))
        line = {}
        try:
            line = json.load(open(os.path.join(run, "run.json")))
        except (OSError, ValueError):
            pass
        d = {"set": line.get("set"), "reads": line.get("reads"), "hip_events_ms": line.get("hip_events_ms"), "rows_sha256_16": line.get("rows_sha256_16"),
             "library_sha256_16": line.get("library_sha256_16")}
        for f in glob.glob(os.path.join(run, "**", "*_kernel_trace.csv"), recursive=True):
            rows = [r for r in csv.DictReader(open(f)) if "query_kernel_r<" in r["Kernel_Name"]]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows][a.drop:]
            if ms:
                d["kernel_trace_ms"] = {"launches": len(ms), "mean": round(statistics.mean(ms), 4), "sd": round(statistics.stdev(ms), 4) if len(ms) > 1 else 0.0,
                                        "min": round(min(ms), 4), "max": round(max(ms), 4)}
        for f in glob.glob(os.path.join(run, "**", "*_counter_collection.csv"), recursive=True):
            per = collections.defaultdict(lambda: collections.defaultdict(float))
            for r in csv.DictReader(open(f)):
                if "query_kernel_r<" in r["Kernel_Name"]:
                    per[r["Counter_Name"]][r["Dispatch_Id"]] += float(r["Counter_Value"])
            if per and line.get("reads"):
                d["pmc_per_read"] = {c: round(statistics.mean(v.values()) / line["reads"], 2) for c, v in sorted(per.items())}
                d["pmc_dispatches"] = len(next(iter(per.values())))
        out[tag] = d
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
