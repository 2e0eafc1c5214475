"""The workload behind DESIGN.md 4.8's figures, to be run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lowc_profile.py [--level 20] [--off] [--write reads.fq]

mic_ingest_classify(MIC_INGEST_NO_CSV) of 1 M synthetic 150-bp reads (four-line FASTQ), twice, in 10 batches of 100 k reads,
against a 32 M-nucleotide synthetic database of 1024 targets; every tenth read carries a planted 40-nt tract of a unit of 1 .. 6
nucleotides.  With a level set, one trace holds lowc_kernel and pack_kernel<false, true> on the same batches; --off: pack_kernel
<false, false> alone, the launch sequence of a run without the option.  Prints the wall time of each pass (host clock around calls
that end in a device wait) and how many reads the mask touches.  --write: the same reads as a four-line FASTQ file, for exe/cuCLARK."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_READS, BATCH, T, K, LEN = 1_000_000, 100_000, 1024, 31, 150
UNITS = [b"A", b"T", b"C", b"AC", b"GA", b"ACG", b"TTC", b"ACGT", b"AACGT", b"AACGTC"]


def main(level, off, write):
    import torch
    from cuclark_amd import MiClarkDB, _lib, host
    L = _lib.load()
    dev = torch.device("cuda:0")
    genome_nt, htsize = 32_000_000, 14444443
    spec = _lib.MicSynthSpec(seed=11, htsize=htsize, genome_nt=genome_nt, n_targets=T, n_genomes=T, k=K, key_bytes=8, mosaic_ppm=0)
    cap = genome_nt + 1024
    d_sizes = torch.empty(htsize, dtype=torch.uint8, device=dev)
    d_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    d_labels = torch.empty(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    assert L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None) == 0
    rb = int(L.mic_synth_text_record_bytes(LEN, 0))
    d_text = torch.empty(N_READS * rb + 64, dtype=torch.uint8, device=dev)
    assert L.mic_synth_reads_text_device(C.byref(spec), 5, N_READS, LEN, 0.2, 0.01, 0.002, 0, -1, d_text.data_ptr(), d_text.numel(), None) == 0
    torch.cuda.synchronize()
    rows = d_text[: N_READS * rb].cpu().numpy().reshape(N_READS, rb).copy()
    del d_text
    # records of one size ("@r<9 digits>\n" SEQ "\n+\n" QUAL "\n"): the sequence starts behind the first line end of a record
    s0 = int(np.flatnonzero(rows[0] == 10)[0]) + 1
    assert (rows[:, s0 - 1] == 10).all() and (rows[:, s0 + LEN] == 10).all()
    rng = np.random.default_rng(3)
    sel = np.arange(0, N_READS, 10)
    at = rng.integers(0, LEN - 40 + 1, sel.size)
    unit = rng.integers(0, len(UNITS), sel.size)
    for u, pat in enumerate(UNITS):
        tract = np.frombuffer((pat * 40)[:40], np.uint8)
        for r, p in zip(sel[unit == u], at[unit == u]):
            rows[r, s0 + p:s0 + p + 40] = tract
    text = rows.tobytes()
    if write:
        with open(write, "wb") as f:
            f.write(text)
        print(f"wrote {write}")
    masked = host.mask_low_complexity(text[:BATCH * rb], level)
    n_touched = sum(b"N" in s for s in masked.split(b"\n")[1::4])
    print(f"level {level}: the host rule masks bases in {n_touched} of the first {BATCH} reads ({BATCH // 10} planted)")
    with MiClarkDB(K, T) as e:
        e.read_device(d_sizes.data_ptr(), htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, BATCH * rb + 4096, [f"L{i}" for i in range(T)])
        e.ingest_set_low_complexity(0 if off else level)
        for p in range(2):                  # two passes over the 10 batches: 20 launches of every kernel
            ok = back = 0
            t0 = time.time()
            for r0 in range(0, N_READS, BATCH):
                out = e.ingest_classify(0, text[r0 * rb:min(N_READS, r0 + BATCH) * rb], csv=False)
                ok += out["status"] == 0
                back += out["status"] != 0
            print(f"pass {p}: {ok} batches on the device, {back} handed back, {(time.time() - t0) * 1e3:.1f} ms, level {0 if off else level}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--write", default="")
    a = ap.parse_args()
    main(a.level, a.off, a.write)
