"""The workload behind DESIGN.md 4.9's device-time table, to be run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/split_profile.py [--which 1|2|3] [--off]

mic_ingest_classify of 2 M synthetic 150-bp reads as four-line FASTQ, twice, in 38 batches of 106 k reads, T = 4096, a 128 M-nucleotide
database (4.5's setup), with read splitting started under CLARK's default filter (--off: not started), so that one trace holds
query_kernel_r, pack_kernel, split_class_kernel, the scan and split_copy_kernel on the same batches.  Afterwards the bytes of one batch
are copied device to device 38 times in the same process (torch.Tensor.copy_ between two device tensors - the runtime's device-to-device
copy -, timed with events): the floor for the copy kernel.
Prints the classes' sizes and the copy's mean."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_READS, BATCH, T, K = 2_000_000, 106_000, 4096, 31


def main(which, off):
    import torch
    from cuclark_amd import MiClarkDB, _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    genome_nt, htsize = 128_000_000, 57777779
    spec = _lib.MicSynthSpec(seed=11, htsize=htsize, genome_nt=genome_nt, n_targets=T, n_genomes=T, k=K, key_bytes=8)
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
    with MiClarkDB(K, T) as e:
        e.read_device(d_sizes.data_ptr(), htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, BATCH * rb + 4096, [f"L{i}" for i in range(T)])
        if not off:
            e.split_start(None, which)
        ok = back = n_c = n_u = b_c = b_u = 0
        for _ in range(2):                  # two passes over the 19 batches: 38 launches of every kernel
            for r0 in range(0, N_READS, BATCH):
                out = e.ingest_classify(0, text[r0 * rb:min(N_READS, r0 + BATCH) * rb])
                ok += out["status"] == 0
                back += out["status"] != 0
                if not off and out["status"] == 0:
                    s = e.ingest_split_text(0)
                    n_c += s["n_classified"]; n_u += s["n_unclassified"]
                    b_c += len(s["classified"] or b""); b_u += len(s["unclassified"] or b"")
        print(f"ingest: {ok} batches, {back} handed back, {rb} bytes per record, splitting {'off' if off else 'which = %d' % which}")
        if not off:
            print(f"split: {n_c} classified records ({b_c} bytes), {n_u} unclassified records ({b_u} bytes)")
    nbytes = BATCH * rb
    d_dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(38)]
    d_dst.copy_(d_text[:nbytes])            # (warm)
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        d_dst.copy_(d_text[:nbytes])
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print(f"device-to-device copy of one batch ({nbytes} bytes): mean {sum(ms) / len(ms) * 1e3:.1f} us, median {ms[len(ms) // 2] * 1e3:.1f} us, "
          f"{nbytes / (sum(ms) / len(ms) * 1e-3) / 1e9:.0f} GB/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", type=int, default=3, choices=[1, 2, 3])
    ap.add_argument("--off", action="store_true")
    a = ap.parse_args()
    main(a.which, a.off)
