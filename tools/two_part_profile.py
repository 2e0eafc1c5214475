"""The headline launch on three read sets, to be run plain (HIP events) or under a profiler:

    python tools/two_part_profile.py --set n001|n0|two [--launches 50] [--warmup 10] [--layout auto|super2] [--out FILE]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/two_part_profile.py --set n001
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_BRANCH SQ_INSTS_LDS -d <dir> -- python tools/two_part_profile.py --set two --launches 4 --warmup 0

bench.py's `full` table and its 10 M x 150 bp reads (same seeds, the packer's format), generated
  n001  as bench.py generates them: 0.1 % N per base,
  n0    without N: every read is one part,
  two   the reads of n001 that keep exactly two parts of at least k nucleotides and at most 128 k-mer positions when joined - the
        reads that leave the pipelined road of query_kernel_r and no others.
One process per read set: every query_kernel_r launch of a trace then belongs to that set.  Prints one JSON line: the reads' part
statistics, the kernel's name, mean and standard deviation of the launches by HIP events, and a digest of all result rows."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk_parts(torch, d_rp, d_cont, n_reads, k):
    """per read: containers used, number of parts kept, lengths of the first two parts (the generator's layout: a 0 ends a read)"""
    dev = d_rp.device
    rp64 = d_rp.to(torch.int64) & 0xFFFFFFFF
    cu16 = d_cont.view(torch.int16).to(torch.int32) & 0xFFFF
    pos, end = rp64[:-1].clone(), rp64[1:]
    live = torch.ones(n_reads, dtype=torch.bool, device=dev)
    n_parts = torch.zeros(n_reads, dtype=torch.int64, device=dev)
    n_short = torch.zeros_like(n_parts)
    len1, len2 = torch.zeros_like(n_parts), torch.zeros_like(n_parts)
    for _ in range(64):
        live &= pos < end
        plen = torch.where(live, cu16[torch.clamp(pos, max=cu16.numel() - 1)].to(torch.int64), torch.zeros_like(pos))
        live &= plen > 0
        if not bool(live.any()):
            break
        len2 = torch.where(live & (n_parts == 1), plen, len2)
        len1 = torch.where(live & (n_parts == 0), plen, len1)
        n_parts += live.to(torch.int64)
        n_short += (live & (plen < k)).to(torch.int64)
        pos = torch.where(live, pos + 1 + (plen + 7) // 8, pos)
    return rp64, pos - rp64[:-1], n_parts, n_short, len1, len2


def compact(torch, d_cont, rp64, used, keep=None):
    """the kept reads back to back, readsPointer[r + 1] = the end of read r, no terminator (what bench.py times)"""
    dev = d_cont.device
    start = rp64[:-1]
    if keep is not None:
        start, used = start[keep], used[keep]
    n = start.numel()
    rp_c = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(used, 0, out=rp_c[1:])
    total = int(rp_c[-1].item())
    src = torch.repeat_interleave(start - rp_c[:-1], used, output_size=total) + torch.arange(total, dtype=torch.int64, device=dev)
    out = torch.zeros(total + 64, dtype=torch.int16, device=dev)          # (the kernel's read-ahead looks past the last read)
    out[:total] = d_cont[src]
    return rp_c.to(torch.int32), out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", required=True, choices=["n001", "n0", "two"])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--layout", default="auto", choices=["auto", "super2"])
    ap.add_argument("--workload", default="full")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from cuclark_amd import MiClarkDB, _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    w = dict(bench.WORKLOADS[a.workload])
    k, T, n_reads, read_len = w["k"], w["n_targets"], w["n_reads"], w["read_len"]
    spec = _lib.MicSynthSpec(seed=4, htsize=w["htsize"], genome_nt=w["genome_nt"], n_targets=T, n_genomes=w["n_genomes"], k=k, key_bytes=w["key_bytes"])
    cap = int(w["genome_nt"]) + 1024
    d_sizes = torch.empty(w["htsize"], dtype=torch.uint8, device=dev)
    d_keys = torch.empty(cap, dtype=torch.int32 if w["key_bytes"] == 4 else torch.int64, device=dev)
    d_labels = torch.empty(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    assert L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None) == 0
    os.environ.setdefault("MIC_SUPER2_MAY_FALL_BACK", "1")
    eng = MiClarkDB(k, T, num_batches=16, device=0, row_words=16, layout={"auto": 0, "super2": 4}[a.layout])
    eng.read_device(d_sizes.data_ptr(), w["htsize"], d_keys.data_ptr(), w["key_bytes"], d_labels.data_ptr())
    del d_sizes, d_keys, d_labels
    torch.cuda.empty_cache()
    name = C.create_string_buffer(256)
    L.mic_db_kernel_name(eng.h, name, 256)

    pitch = L.mic_synth_read_pitch(read_len, k)
    d_rp = torch.empty(n_reads + 1, dtype=torch.int32, device=dev)
    d_cont = torch.zeros(n_reads * pitch + 64, dtype=torch.int16, device=dev)
    n_rate = 0.0 if a.set == "n0" else 0.001
    assert L.mic_synth_reads_device2(C.byref(spec), 5, n_reads, read_len, 0, 0.2, 0.01, n_rate, d_rp.data_ptr(), d_cont.data_ptr(), d_cont.numel(),
                                     None, None) == 0
    torch.cuda.synchronize()
    rp64, used, n_parts, n_short, len1, len2 = walk_parts(torch, d_rp, d_cont, n_reads, k)
    two = (n_parts == 2) & (n_short == 0) & (len1 + len2 - k + 1 <= 128)
    stats = {"reads_generated": n_reads, "n_rate": n_rate,
             "reads_of_one_part": int((n_parts == 1).sum()), "reads_of_two_parts": int((n_parts == 2).sum()),
             "reads_of_more_parts": int((n_parts > 2).sum()), "reads_without_part": int((n_parts == 0).sum()),
             "reads_with_a_part_shorter_than_k": int((n_short > 0).sum()), "two_part_reads_that_fit_one_chunk": int(two.sum())}
    d_rp, d_cont, n = compact(torch, d_cont, rp64, used, two if a.set == "two" else None)
    del rp64, used, n_parts, n_short, len1, len2, two
    torch.cuda.empty_cache()
    d_res = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    ms = []
    for i in range(a.warmup + a.launches):
        eng.query_device(d_rp.data_ptr(), d_cont.data_ptr(), n, d_res.data_ptr(), 0, 0)
        eng.resolve_flagged_device(d_rp.data_ptr(), d_cont.data_ptr(), d_res.data_ptr(), 0, 0)
        if i >= a.warmup:
            ms.append(eng.last_query_ms())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    out = {"set": a.set, "layout": a.layout, "kernel": name.value.decode(), "reads": n, "parts": stats, "warmup": a.warmup, "launches": a.launches,
           "hip_events_ms": {"mean": round(float(np.mean(ms)), 4), "sd": round(float(np.std(ms, ddof=1)) if len(ms) > 1 else 0.0, 4),
                             "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)},
           "reads_with_hits": int(np.count_nonzero(res[:, 0])), "rows_sha256_16": hashlib.sha256(res.tobytes()).hexdigest()[:16],
           "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
