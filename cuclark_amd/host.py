"""Host-side pieces of the path exposed by the C ABI: key-width rule, read indexer, packer, CSV.

These wrap the C++ implementations in cuclark_amd/csrc/mic_host.cpp (the same code the cuCLARK CLI uses);
nothing here touches the GPU.
"""
import ctypes as C

import numpy as np

from . import _lib


def key_bytes_rule(htsize, k):
    """main.cc:274-316."""
    return int(_lib.load().mic_key_bytes_rule(int(htsize), int(k)))


def index_reads(data, threads=1):
    """CuCLARK_hh.hh:1339-1534 (one batch).  Returns dict of u64 arrays or None for an unknown format."""
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    cap = max(16, buf.size // 64)
    while True:
        arrs = [np.zeros(cap, np.uint64) for _ in range(5)]
        if threads > 1:
            n = L.mic_index_reads_parallel(buf.ctypes.data, buf.size, threads, cap, *[a.ctypes.data for a in arrs])
        else:
            n = L.mic_index_reads(buf.ctypes.data, buf.size, cap, *[a.ctypes.data for a in arrs])
        if n < 0:
            return None
        if n <= cap:
            return dict(zip(("name_s", "name_e", "seq_s", "seq_e", "length"), [a[:n].copy() for a in arrs]))
        cap = n


def pack_reads(data, seq_s, seq_e, length, k):
    """CuCLARK_hh.hh:1616-1716.  Returns (reads_pointer u32[n+1], containers u16[m])."""
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    seq_s = np.ascontiguousarray(seq_s, np.uint64)
    seq_e = np.ascontiguousarray(seq_e, np.uint64)
    length = np.ascontiguousarray(length, np.uint64)
    n = seq_s.size
    cap = int(L.mic_pack_bound(seq_s.ctypes.data, seq_e.ctypes.data, n, k))
    rp = np.zeros(n + 1, np.uint32)
    cont = np.zeros(cap, np.uint16)
    m = L.mic_pack_reads(buf.ctypes.data, seq_s.ctypes.data, seq_e.ctypes.data, length.ctypes.data, n, k, rp.ctypes.data,
                         cont.ctypes.data, cap)
    if m == C.c_size_t(-1).value:
        raise RuntimeError("mic_pack_reads: bound too small")
    return rp, cont[:m].copy()


def format_csv(data, idx, results, target_names, k, paired=False, extended=False, rows=None, dense=None):
    """CuCLARK_hh.hh:1951-2139: header + one line per read.  dense: optional dict read index -> u32[T] counts."""
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    names = (C.c_char_p * len(target_names))(*[t.encode() for t in target_names])
    T = len(target_names)
    cap = 512 + (T * 48 if extended else 0) + sum(len(t) + 1 for t in target_names)
    line = C.create_string_buffer(cap)
    out = []
    n = L.mic_csv_header(line, cap, int(extended), names, T)
    out.append(line.raw[:n])
    results = np.ascontiguousarray(results, np.uint32)
    for r in range(results.shape[0]):
        row_p = rows[r].ctypes.data if (extended and rows is not None) else None
        dn = None
        if extended and dense is not None and r in dense:
            dn = np.ascontiguousarray(dense[r], np.uint32)
        ns, ne = int(idx["name_s"][r]), int(idx["name_e"][r])
        n = L.mic_csv_line(line, cap, buf.ctypes.data + ns, ne - ns, int(idx["length"][r]), int(paired), k,
                           results[r].ctypes.data, names, T, int(extended), row_p, dn.ctypes.data if dn is not None else None)
        assert n >= 0
        out.append(line.raw[:n])
    return b"".join(out)


def build_db(target_files, target_labels, k, htsize, out_prefix, key_bytes=0, min_count=0, device=-1, threads=4, parts=0,
             light_gap=0):
    """GPU database builder (mic_db_build): target_labels[i] is the label index of target_files[i].  Returns #k-mers.
    light_gap > 0 builds cuCLARK-l's light database (non-overlapping k-blocks, every light_gap-th one)."""
    L = _lib.load()
    files = (C.c_char_p * len(target_files))(*[f.encode() for f in target_files])
    labels = np.ascontiguousarray(target_labels, np.uint16)
    n = C.c_uint64(0)
    rc = L.mic_db_build(files, labels.ctypes.data, len(target_files), int(k), int(htsize), int(key_bytes), int(min_count),
                        int(light_gap), out_prefix.encode(), int(device), int(threads), int(parts), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"mic_db_build failed ({rc}): {L.mic_db_build_error().decode(errors='replace')}")
    return int(n.value)


def parse_threshold(text, max_int=1):
    """A threshold as the command lines take it (mic_abund_parse): (num, den) with den = 10^d, d <= 9; ValueError otherwise."""
    num, den = C.c_uint64(0), C.c_uint64(0)
    if _lib.load().mic_abund_parse(text.encode() if isinstance(text, str) else text, int(max_int), C.byref(num), C.byref(den)) != 0:
        raise ValueError(f"not a threshold in [0, {max_int}] with at most 9 decimals: {text!r}")
    return int(num.value), int(den.value)


def mask_quality(data, q, offset=33, threshold_byte=None):
    """mic_fastq_mask_quality: the bytes of four-line FASTQ text with every base whose Phred quality is below q (quality characters
    at `offset`) replaced by 'N' - csrc/mic_qmask.h's rule on the CPU; q = 0: a plain copy.  threshold_byte overrides offset + q.
    ValueError when the text does not start with '@' or its line count is no multiple of four."""
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.empty(max(src.size, 1), np.uint8)
    c0 = int(threshold_byte) if threshold_byte is not None else ((int(offset) + int(q)) if q else 0)
    rc = _lib.load().mic_fastq_mask_quality(src.ctypes.data if src.size else None, src.size, c0, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_fastq_mask_quality: not four-line FASTQ text, or a threshold byte above 255 ({rc})")
    return out[: src.size].tobytes()


def mask_low_complexity(data, level):
    """mic_text_mask_low_complexity: the bytes of FASTA or four-line FASTQ text with every base whose 32-nucleotide window has a DUST
    score above level / 10 replaced by 'N' - csrc/mic_lowc.h's rule on the CPU; level 0: a plain copy.
    ValueError when the text does not start with '>' or '@', or the level is above 149."""
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.empty(max(src.size, 1), np.uint8)
    rc = _lib.load().mic_text_mask_low_complexity(src.ctypes.data if src.size else None, src.size, int(level), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_text_mask_low_complexity: not FASTA / FASTQ text, or a level above 149 ({rc})")
    return out[: src.size].tobytes()


def abund_filter(confidence="0.5", gamma="0"):
    """mic_abund_filter from decimal strings (CLARK's defaults: -c 0.5 -g 0)."""
    cn, cd = parse_threshold(confidence)
    gn, gd = parse_threshold(gamma)
    return _lib.MicAbundFilter(cn, cd, gn, gd)


def abundance_host(results, norm, k, n_targets, filt=None):
    """mic_abundance_host: u64[n_targets + 2] counts of the result rows (u32[n, 8]) by the rule of csrc/mic_abund.h
    ([0] unassigned, [1] filtered out, [t + 2] target t).  norm: the CSV's Length column per read, or None (no gamma filter)."""
    L = _lib.load()
    results = np.ascontiguousarray(results, np.uint32).reshape(-1, 8)
    n = results.shape[0]
    nm = np.ascontiguousarray(norm, np.uint32) if norm is not None else None
    counts = np.zeros(int(n_targets) + 2, np.uint64)
    f = filt if filt is not None else abund_filter()
    rc = L.mic_abundance_host(results.ctypes.data, nm.ctypes.data if nm is not None else None, n, int(k), int(n_targets), C.byref(f),
                              counts.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_abundance_host: invalid argument ({rc})")
    return counts


def split_host(data, rec_start, results, norm, k, n_targets, filt=None, which=3):
    """mic_split_host: the text's records (rec_start: u64 byte offsets, [0] = 0) partitioned by the rule of csrc/mic_split.h.
    Returns (out u8[len(data) + 1], (a, b, n_classified, n_unclassified)): classified records at out[:a], unclassified at
    out[a:a + b]; a class `which` (1 classified, 2 unclassified, 3 both) does not name is not written."""
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    results = np.ascontiguousarray(results, np.uint32).reshape(-1, 8)
    starts = np.ascontiguousarray(rec_start, np.uint64)
    nm = np.ascontiguousarray(norm, np.uint32) if norm is not None else None
    out = np.full(buf.size + 1, 0xA5, np.uint8)
    tot = np.zeros(4, np.uint64)
    f = filt if filt is not None else abund_filter()
    rc = L.mic_split_host(buf.ctypes.data, buf.size, starts.ctypes.data, starts.size, results.ctypes.data,
                          nm.ctypes.data if nm is not None else None, int(k), int(n_targets), C.byref(f), int(which), out.ctypes.data,
                          tot.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_split_host: invalid argument ({rc})")
    return out, tuple(int(x) for x in tot)


def density_host(results, norm, k, n_targets, counts=None):
    """mic_density_host: u64[5153] score-density counters of the result rows (u32[n, 8]) by the rule of csrc/mic_density.h
    ([0] reads, [1] unassigned, [2 + (c - 50) * 101 + g]).  norm: the CSV's Length column per read, or None (gamma bin 0).
    counts: an array to ADD to (returned), else a fresh one."""
    L = _lib.load()
    results = np.ascontiguousarray(results, np.uint32).reshape(-1, 8)
    nm = np.ascontiguousarray(norm, np.uint32) if norm is not None else None
    assert nm is None or nm.size == results.shape[0], "norm: one entry per result row"
    if counts is None:
        counts = np.zeros(_lib.MIC_DENSITY_WORDS, np.uint64)
    assert counts.dtype == np.uint64 and counts.size == _lib.MIC_DENSITY_WORDS and counts.flags.c_contiguous
    rc = L.mic_density_host(results.ctypes.data, nm.ctypes.data if nm is not None else None, results.shape[0], int(k), int(n_targets),
                            counts.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_density_host: invalid argument ({rc})")
    return counts


def density_report(counts, which=0):
    """mic_density_format: the report of exe/cuCLARK --density / exe/evaluate_density (csrc/density_report.hpp) as str.
    which: 0 all four blocks, 1 totals + confidence, 2 totals + gamma."""
    L = _lib.load()
    c = np.ascontiguousarray(counts, np.uint64)
    n = L.mic_density_format(c.ctypes.data, c.size, int(which), None, 0)
    if n < 0:
        raise ValueError(f"mic_density_format: invalid argument ({n})")
    buf = C.create_string_buffer(n + 1)
    assert L.mic_density_format(c.ctypes.data, c.size, int(which), buf, n + 1) == n
    return buf.raw[:n].decode()


def ksketch_add(kmers, labels, k, n_targets, regs=None, hits=None):
    """mic_ksketch_add_host: the sketch rule of csrc/mic_ksketch.h on (k-mer as it reads, label) pairs; label 0 or above n_targets adds
    nothing, label l adds to target l - 1.  regs (u8[n_targets, 16384]) / hits (u64[n_targets]): arrays to ADD to, else fresh ones.
    Returns (regs, hits)."""
    L = _lib.load()
    km = np.ascontiguousarray(kmers, np.uint64).reshape(-1)
    lb = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    assert km.size == lb.size, "one label per k-mer"
    if regs is None:
        regs = np.zeros((int(n_targets), _lib.MIC_KSKETCH_REGS), np.uint8)
    if hits is None:
        hits = np.zeros(int(n_targets), np.uint64)
    assert regs.dtype == np.uint8 and regs.size == int(n_targets) * _lib.MIC_KSKETCH_REGS and regs.flags.c_contiguous
    assert hits.dtype == np.uint64 and hits.size == int(n_targets) and hits.flags.c_contiguous
    rc = L.mic_ksketch_add_host(km.ctypes.data, lb.ctypes.data, km.size, int(k), int(n_targets), regs.ctypes.data, hits.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_ksketch_add_host: invalid argument ({rc})")
    return regs, hits


def ksketch_estimate(regs):
    """mic_ksketch_estimate: the number of distinct k-mers behind one target's 16384 registers (float; all zero: 0.0)."""
    L = _lib.load()
    r = np.ascontiguousarray(regs, np.uint8).reshape(-1)
    assert r.size == _lib.MIC_KSKETCH_REGS, "the registers of one target"
    return float(L.mic_ksketch_estimate(r.ctypes.data))


def ksketch_report(names, reads, regs, hits):
    """mic_ksketch_format: the report of exe/cuCLARK --kmer-report (csrc/kmer_report.hpp) as str.  names: one per target; reads: u64 per
    target (what --abundance counts for it); regs, hits: the sketches."""
    L = _lib.load()
    n = len(names)
    rd = np.ascontiguousarray(reads, np.uint64).reshape(-1)
    rg = np.ascontiguousarray(regs, np.uint8).reshape(-1)
    ht = np.ascontiguousarray(hits, np.uint64).reshape(-1)
    assert rd.size == n and ht.size == n and rg.size == n * _lib.MIC_KSKETCH_REGS
    arr = (C.c_char_p * max(n, 1))(*[s.encode() if isinstance(s, str) else bytes(s) for s in names])
    ln = L.mic_ksketch_format(arr, rd.ctypes.data, rg.ctypes.data, ht.ctypes.data, n, None, 0)
    if ln < 0:
        raise ValueError(f"mic_ksketch_format: invalid argument ({ln})")
    buf = C.create_string_buffer(ln + 1)
    assert L.mic_ksketch_format(arr, rd.ctypes.data, rg.ctypes.data, ht.ctypes.data, n, buf, ln + 1) == ln
    return buf.raw[:ln].decode()


def hitmap_runs(labels, part_nk, n_targets):
    """mic_hitmap_runs_host: the hit-map rule of csrc/mic_hitmap.h on the labels of one read's k-mer positions, part after part (label 0
    or above n_targets: no target); part_nk: positions per part.  Returns the words (u32): (label << 16) | len per run, 0 between parts."""
    L = _lib.load()
    lb = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    nk = np.ascontiguousarray(part_nk, np.uint32).reshape(-1)
    assert int(nk.astype(np.int64).sum()) == lb.size, "one label per k-mer position"
    args = (lb.ctypes.data if lb.size else None, nk.ctypes.data if nk.size else None, nk.size, int(n_targets))
    n = L.mic_hitmap_runs_host(*args, None, 0)
    if n < 0:
        raise ValueError(f"mic_hitmap_runs_host: invalid argument ({n})")
    words = np.zeros(max(n, 1), np.uint32)
    assert L.mic_hitmap_runs_host(*args, words.ctypes.data, words.size) == n
    return words[:n]


def hitmap_format(read_names, offsets, words, target_names):
    """mic_hitmap_format: the text of exe/cuCLARK --hit-maps without its header line, as bytes.  read_names: one per read (bytes or
    str, as the indexers cut them); offsets u32[n + 1], words u32; target_names: one per target."""
    L = _lib.load()
    enc = lambda s: s.encode() if isinstance(s, str) else bytes(s)
    n, T = len(read_names), len(target_names)
    off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
    wd = np.ascontiguousarray(words, np.uint32).reshape(-1)
    assert off.size == n + 1 and (n == 0 or int(off[-1]) <= wd.size)
    rn = (C.c_char_p * max(n, 1))(*[enc(s) for s in read_names])
    tn = (C.c_char_p * max(T, 1))(*[enc(s) for s in target_names])
    args = (rn, n, off.ctypes.data, wd.ctypes.data if wd.size else None, tn, T)
    ln = L.mic_hitmap_format(*args, None, 0)
    if ln < 0:
        raise ValueError(f"mic_hitmap_format: invalid argument ({ln})")
    buf = C.create_string_buffer(ln + 1)
    assert L.mic_hitmap_format(*args, buf, ln + 1) == ln
    return buf.raw[:ln]


def kraken_format(read_names, results, norm, k, offsets, words, target_names, filt=None):
    """mic_kraken_format: the text of exe/cuCLARK --kraken-out (csrc/mic_kraken.h), as bytes.  read_names, offsets, words and
    target_names as for hitmap_format; results u32[n, 8]; norm: the CSV's Length column per read, or None; filt as for abundance_host."""
    L = _lib.load()
    enc = lambda s: s.encode() if isinstance(s, str) else bytes(s)
    n, T = len(read_names), len(target_names)
    f = filt if filt is not None else abund_filter()
    res = np.ascontiguousarray(results, np.uint32).reshape(-1, 8)
    nm = None if norm is None else np.ascontiguousarray(norm, np.uint32).reshape(-1)
    off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
    wd = np.ascontiguousarray(words, np.uint32).reshape(-1)
    assert res.shape[0] == n and (nm is None or nm.size == n) and off.size == n + 1 and (n == 0 or int(off[-1]) <= wd.size)
    rn = (C.c_char_p * max(n, 1))(*[enc(s) for s in read_names])
    tn = (C.c_char_p * max(T, 1))(*[enc(s) for s in target_names])
    args = (rn, n, res.ctypes.data if n else None, None if nm is None else nm.ctypes.data, int(k), T, C.byref(f), off.ctypes.data,
            wd.ctypes.data if wd.size else None, tn)
    ln = L.mic_kraken_format(*args, None, 0)
    if ln < 0:
        raise ValueError(f"mic_kraken_format: invalid argument ({ln})")
    buf = C.create_string_buffer(ln + 1)
    assert L.mic_kraken_format(*args, buf, ln + 1) == ln
    return buf.raw[:ln]


def db_census(sizes, keys, labels, k, n_targets, sampling=1):
    """mic_db_census_host: the census rule of csrc/mic_census.h on the arrays a table is loaded from (bucket sizes u8[htsize], keys,
    0-based labels), without a table: every canonical k-mer the builders enumerate counts under its file label - what a healthy whole
    table returns.  Returns (counts u64[n_targets], stats u64[8])."""
    L = _lib.load()
    sz = np.ascontiguousarray(sizes, np.uint8).reshape(-1)
    ky = np.ascontiguousarray(keys).reshape(-1)
    lb = np.ascontiguousarray(labels, np.uint16).reshape(-1)
    assert ky.dtype.itemsize in (2, 4, 8) and ky.dtype.kind == "u" and ky.size == lb.size
    assert int(sz.sum(dtype=np.uint64)) == ky.size, "one key per element"
    counts = np.zeros(int(n_targets), np.uint64)
    stats = np.zeros(8, np.uint64)
    rc = L.mic_db_census_host(sz.ctypes.data if sz.size else None, sz.size, ky.ctypes.data if ky.size else None, ky.dtype.itemsize,
                              lb.ctypes.data if lb.size else None, int(sampling), int(k), int(n_targets),
                              counts.ctypes.data if counts.size else None, stats.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_db_census_host: invalid argument ({rc})")
    return counts, stats


def kcoverage_report(names, reads, regs, hits, target_kmers):
    """mic_kcoverage_format: the report of exe/cuCLARK --kmer-coverage (csrc/kmer_report.hpp) as str: ksketch_report's arguments and
    target_kmers, u64 per target (the census counts).  ValueError for a target with hits and no k-mers in the table."""
    L = _lib.load()
    n = len(names)
    rd = np.ascontiguousarray(reads, np.uint64).reshape(-1)
    rg = np.ascontiguousarray(regs, np.uint8).reshape(-1)
    ht = np.ascontiguousarray(hits, np.uint64).reshape(-1)
    tk = np.ascontiguousarray(target_kmers, np.uint64).reshape(-1)
    assert rd.size == n and ht.size == n and tk.size == n and rg.size == n * _lib.MIC_KSKETCH_REGS
    arr = (C.c_char_p * max(n, 1))(*[s.encode() if isinstance(s, str) else bytes(s) for s in names])
    args = (C.cast(arr, C.c_void_p), rd.ctypes.data, rg.ctypes.data, ht.ctypes.data, tk.ctypes.data, n)
    ln = L.mic_kcoverage_format(*args, None, 0)
    if ln < 0:
        raise ValueError(f"mic_kcoverage_format: invalid argument ({ln})")
    buf = C.create_string_buffer(ln + 1)
    assert L.mic_kcoverage_format(*args, buf, ln + 1) == ln
    return buf.raw[:ln].decode()


def rollup_check(n_targets, group_of):
    """mic_rollup_check: raises ValueError (with the library's message) unless group_of (u16[n_levels, n_targets], level 1 first) has
    1 .. 7 levels, ids numbered by first appearance at every level, and every level a coarsening of the one below."""
    L = _lib.load()
    g = np.ascontiguousarray(group_of, np.uint16)
    n_levels = g.size // int(n_targets) if int(n_targets) and g.size % int(n_targets) == 0 else 0
    if L.mic_rollup_check(int(n_targets), n_levels, g.ctypes.data if g.size else None) != 0:
        raise ValueError(L.mic_last_error().decode(errors="replace"))


def rollup_host(rows, norm, k, n_targets, group_of, filt=None, dense=None, want_levels=False):
    """mic_rollup_host: the roll-up rule of csrc/mic_rollup.h on the CPU.  rows: u32[n, row_words] sparse rows or None; dense:
    u32[n, n_targets] counts or None (used for the reads whose row is invalid; for all reads when rows is None).
    Returns (rollup u32[n, 8], levels u32[n, n_levels + 1, 4] or None, counts u64[2 + T + G_1 + .. + G_L])."""
    L = _lib.load()
    T = int(n_targets)
    g = np.ascontiguousarray(group_of, np.uint16).reshape(-1, T)
    nl = g.shape[0]
    rw = 0
    if rows is not None:
        rows = np.ascontiguousarray(rows, np.uint32)
        rw = rows.shape[1]
        n = rows.shape[0]
    if dense is not None:
        dense = np.ascontiguousarray(dense, np.uint32).reshape(-1, T)
        n = dense.shape[0]
    nm = np.ascontiguousarray(norm, np.uint32) if norm is not None else None
    n_counters = 2 + T + sum(int(g[l].max()) + 1 for l in range(nl))
    rollup = np.zeros((n, _lib.MIC_ROLLUP_WORDS), np.uint32)
    levels = np.zeros((n, nl + 1, 4), np.uint32) if want_levels else None
    counts = np.zeros(n_counters, np.uint64)
    f = filt if filt is not None else abund_filter()
    rc = L.mic_rollup_host(rows.ctypes.data if rows is not None else None, rw, dense.ctypes.data if dense is not None else None,
                           nm.ctypes.data if nm is not None else None, n, int(k), T, nl, g.ctypes.data, C.byref(f),
                           rollup.ctypes.data, levels.ctypes.data if levels is not None else None, counts.ctypes.data)
    if rc != 0:
        raise ValueError(f"mic_rollup_host: invalid argument ({rc})")
    return rollup, levels, counts
