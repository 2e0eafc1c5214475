"""The workload behind DESIGN.md 4.11's device-time figures, to be run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/hitmap_profile.py [--off | --kraken | --both]

mic_ingest_classify of 2 M synthetic 150-bp reads as four-line FASTQ, twice, in 38 batches of 106 k reads, T = 4096, a 128 M-nucleotide
database (4.10's setup), with the hit maps started (--off: not started), so that one trace holds query_kernel_r, pack_kernel, the two
instantiations of hitmap_kernel, hitmap_len_kernel and hitmap_fmt_kernel on the same batches.  Prints the number of batches, the bytes
of hit-map text and the tokens in it.  --kraken: the product in Kraken format (kraken_len_kernel / kraken_fmt_kernel in
place of the two hit-map text kernels); --both: the passes with hit maps, then the same passes in Kraken format, so that one trace
holds both pairs of text kernels on the same batches."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_READS, BATCH, T, K = 2_000_000, 106_000, 4096, 31


def main(off, formats=("hitmap",)):
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
        for fmt in formats:
            if not off:                     # (in front of the slots: their hit-map buffers come with them)
                e.kraken_start() if fmt == "kraken" else e.hitmap_start()
            e.ingest_alloc(1, BATCH * rb + 4096, [f"L{i}" for i in range(T)])
            ok = back = n_bytes = n_tokens = n_seps = 0
            for _ in range(2):                  # two passes over the 19 batches: 38 launches of every kernel
                for r0 in range(0, N_READS, BATCH):
                    out = e.ingest_classify(0, text[r0 * rb:min(N_READS, r0 + BATCH) * rb])
                    ok += out["status"] == 0
                    back += out["status"] != 0
                    if not off and out["status"] == 0:
                        hm = e.ingest_kraken_text(0) if fmt == "kraken" else e.ingest_hitmap_text(0)
                        n_bytes += len(hm)
                        n_tokens += hm.count(b":")
                        n_seps += hm.count(b"|")
            print(f"ingest: {ok} batches, {back} handed back, {rb} bytes per record, {fmt} text {'off' if off else 'on'}")
            if not off:
                print(f"{fmt}: {n_bytes} bytes of text, {n_tokens} runs, {n_seps} separators, {n_tokens / max(1, 2 * N_READS):.2f} runs per read")
                e.kraken_stop() if fmt == "kraken" else e.hitmap_stop()
            e.ingest_free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--kraken", action="store_true")
    ap.add_argument("--both", action="store_true")
    a = ap.parse_args()
    main(a.off, ("hitmap", "kraken") if a.both else ("kraken",) if a.kraken else ("hitmap",))
