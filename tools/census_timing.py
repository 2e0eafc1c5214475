#!/usr/bin/env python3
"""What the table census costs: a synthetic database generated in HBM (mic_synth_db_device, the benchmark's
generator and seed), loaded with mic_db_load_device - census off, then census on - several times each.

    python tools/census_timing.py [--workload full|light] [--reps 3] [--layout auto|direct|minimizer|super|super2]

Prints one JSON line: the wall time of every load, the build report of the first load of each kind (line for line what the library
reports), the `census:` seconds of every load with the option on, their median and the k-mers per second.  Works on a build without
the census too (the parent commit): the loads with the option on are then left out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {   # bench.py's "full" and "light" tables
    "full": dict(htsize=1610612741, genome_nt=5_730_000_000, n_genomes=8192, n_targets=4096, k=31, key_bytes=4),
    "light": dict(htsize=57777779, genome_nt=54_000_000, n_genomes=512, n_targets=512, k=31, key_bytes=8),
}
LAYOUTS = {"auto": 0, "direct": 1, "minimizer": 2, "super": 3, "super2": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="full", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layout", default="auto", choices=sorted(LAYOUTS))
    args = ap.parse_args()
    import torch
    from cuclark_amd import MiClarkDB, _lib
    # (a library of the parent commit lacks the census symbols: bind what it exports)
    _lib._share_hip_runtime_with_torch()
    exported = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(exported, s[0])]
    L = _lib.load()
    w = WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    spec = _lib.MicSynthSpec(seed=4, htsize=w["htsize"], genome_nt=w["genome_nt"], n_targets=w["n_targets"], n_genomes=w["n_genomes"], k=w["k"],
                             key_bytes=w["key_bytes"], keep_ppm=0, run_len=0, repeat_ppm=0, mosaic_ppm=0)
    cap = int(w["genome_nt"]) + 1024
    d_sizes = torch.empty(w["htsize"], dtype=torch.uint8, device=dev)
    d_keys = torch.empty(cap, dtype=torch.int32 if w["key_bytes"] == 4 else torch.int64, device=dev)
    d_labels = torch.empty(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    rc = L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None)
    assert rc == 0, f"mic_synth_db_device failed ({rc})"
    os.environ.setdefault("MIC_SUPER2_MAY_FALL_BACK", "1")
    has_census = hasattr(L, "mic_db_census_enable")
    out = {"workload": args.workload, "device": torch.cuda.get_device_name(0), "elements": n_el.value, "has_census": has_census}
    for on in ([False, True] if has_census else [False]):
        walls, census_s, report, info, stats = [], [], None, None, None
        for _ in range(args.reps):
            with MiClarkDB(w["k"], w["n_targets"], layout=LAYOUTS[args.layout]) as e:
                if on:
                    e.census_enable()
                torch.cuda.synchronize()
                t0 = time.time()
                e.read_device(d_sizes.data_ptr(), w["htsize"], d_keys.data_ptr(), w["key_bytes"], d_labels.data_ptr())
                e.sync()
                walls.append(round(time.time() - t0, 4))
                rep = L.mic_db_last_build_report().decode()
                report = report or rep
                info = e.info()
                if on:
                    census_s += [float(ln.split(":")[1]) for ln in rep.splitlines() if ln.startswith("census:")]
                    counts, st = e.census_fetch()
                    stats = [int(v) for v in st]
                    assert stats[3] == 0 and int(counts.sum()) == stats[0] - stats[4] and stats[0] == info["n_elems"]
        key = "census_on" if on else "census_off"
        out[key] = {"load_wall_s": walls, "load_wall_median_s": statistics.median(walls), "build_report": report.splitlines(), "kmers": info["n_elems"],
                    "layout": info["layout"]}
        if on:
            med = statistics.median(census_s)
            out[key].update({"census_s": census_s, "census_median_s": med, "kmers_per_s": round(info["n_elems"] / med) if med > 0 else None, "stats": stats})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
