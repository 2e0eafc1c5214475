"""The workload behind DESIGN.md 4.7's table, to be run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/density_profile.py ingest [--mosaic-ppm 150000] [--off]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/density_profile.py crafted same|spread

ingest   mic_ingest_classify(MIC_INGEST_NO_CSV) of 2 M synthetic 150-bp reads, twice, in 38 batches of 106 k reads, T = 4096, a 128 M-nucleotide
         database (4.5's setup), with abundance and density counting started (--off: neither), so that one trace holds query_kernel_r,
         abund_kernel and density_kernel on the same batches.
crafted  38 launches of mic_density_device on 106 k crafted rows: `same` = every read in one cell (the most a wave can contend for an
         LDS address), `spread` = the cells drawn uniformly (the least).
MIC_DENSITY_AGG=0|1|2 picks the aggregation the density kernel is built with (csrc/mic_density.hip).  Prints the counters' totals."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_READS, BATCH, T, K = 2_000_000, 106_000, 4096, 31


def ingest(mosaic_ppm, off):
    import torch
    from cuclark_amd import MiClarkDB, _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    genome_nt, htsize = 128_000_000, 57777779
    spec = _lib.MicSynthSpec(seed=11, htsize=htsize, genome_nt=genome_nt, n_targets=T, n_genomes=T, k=K, key_bytes=8, mosaic_ppm=mosaic_ppm)
    cap = genome_nt + 1024
    d_sizes = torch.empty(htsize, dtype=torch.uint8, device=dev)
    d_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    d_labels = torch.empty(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    assert L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None) == 0
    rb = int(L.mic_synth_text_record_bytes(150, 0))
    d_text = torch.empty(N_READS * rb + 64, dtype=torch.uint8, device=dev)
    assert L.mic_synth_reads_text_device(C.byref(spec), 5, N_READS, 150, 0.2, 0.01, 0.002, 0, -1, d_text.data_ptr(), d_text.numel(), None) == 0
    torch.cuda.synchronize()
    text = d_text[: N_READS * rb].cpu().numpy().tobytes()
    del d_text
    with MiClarkDB(K, T) as e:
        e.read_device(d_sizes.data_ptr(), htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, BATCH * rb + 4096, [f"L{i}" for i in range(T)])
        if not off:
            e.abundance_start()
            e.density_start()
        ok = back = 0
        for _ in range(2):                  # two passes over the 19 batches: 38 launches of every kernel
            for r0 in range(0, N_READS, BATCH):
                out = e.ingest_classify(0, text[r0 * rb:min(N_READS, r0 + BATCH) * rb], csv=False)
                ok += out["status"] == 0
                back += out["status"] != 0
        print(f"ingest: {ok} batches counted on the device, {back} handed back, mosaic_ppm {mosaic_ppm}, counting {'off' if off else 'on'}")
        if not off:
            a, d = e.abundance_fetch(), e.density_fetch()
            print(f"abundance: {int(a.sum())} reads; density: {int(d[0])} reads, {int(d[1])} unassigned, {int(np.count_nonzero(d[2:]))} cells, "
                  f"largest cell {int(d[2:].max())}")


def crafted(kind):
    import torch
    from cuclark_amd import MiClarkDB, host
    rng = np.random.default_rng(1)
    res = np.zeros((BATCH, 8), np.uint32)
    res[:, 1] = 1 + rng.integers(0, T, BATCH)
    if kind == "same":
        res[:, 0], res[:, 2] = 90, 90
    else:
        c = rng.integers(50, 101, BATCH)
        res[:, 0], res[:, 2], res[:, 4] = rng.integers(0, 121, BATCH), c, 100 - c
    norm = np.full(BATCH, 150, np.uint32)
    dev = torch.device("cuda:0")
    d_res = torch.from_numpy(res.view(np.int32)).to(dev)
    d_norm = torch.from_numpy(norm.view(np.int32)).to(dev)
    d_counts = torch.zeros(5153, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with MiClarkDB(K, T) as e:
        for _ in range(38):
            e.density_device(d_res.data_ptr(), d_norm.data_ptr(), BATCH, d_counts.data_ptr())
        e.sync()
    got = d_counts.cpu().numpy().view(np.uint64)
    assert (got == 38 * host.density_host(res, norm, K, T)).all()
    print(f"crafted {kind}: {int(np.count_nonzero(got[2:]))} cells, counters as the host rule's")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ingest", "crafted"])
    ap.add_argument("kind", nargs="?", default="same", choices=["same", "spread"])
    ap.add_argument("--mosaic-ppm", type=int, default=0)
    ap.add_argument("--off", action="store_true")
    a = ap.parse_args()
    ingest(a.mosaic_ppm, a.off) if a.what == "ingest" else crafted(a.kind)
