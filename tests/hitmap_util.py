"""A restatement in Python of the hit-map rule (csrc/mic_hitmap.h): per maximal nucleotide run of at least k nucleotides the labels of
its k-mers from a dict of the database, runs above 65 528 nucleotides cut the way the packer's emit_run cuts them, itertools.groupby
over each part's labels, then the words and the text.  Shared by tests/test_hit_maps.py (which pins the library's host functions to
it) and tests/test_hit_maps_gpu.py (whose expected values all come from here)."""
import itertools

import numpy as np

import ksketch_util as ku

MAX_PART = 65528
HEADER = b"Object_ID,Hit_map\n"


def _kmers(codes, k):
    """k-mer values (as they read) of every position of a stretch of 2-bit codes"""
    n = codes.size - k + 1
    v = np.zeros(n, np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | codes[j:j + n].astype(np.uint64)
    return v


def parts_of(seq, k):
    """the parts of a read as arrays of 2-bit codes: maximal nucleotide runs of >= k, a run above MAX_PART as overlapping sub-parts"""
    codes = ku._LUT[np.frombuffer(bytes(seq), np.uint8)]
    out = []
    edges = np.flatnonzero(np.diff(np.concatenate(([True], codes == 255, [True])).astype(np.int8)))
    for a, b in zip(edges[::2], edges[1::2]):
        run = codes[a:b]
        if run.size < k:
            continue
        start = 0
        while True:                       # emit_run (csrc/mic_host.cpp)
            plen = min(run.size - start, MAX_PART)
            out.append(run[start:start + plen])
            if start + plen >= run.size:
                break
            start += plen - (k - 1)
    return out


def part_labels(dct, seq, k, n_targets):
    """per part the labels of its k-mer positions: 1-based, 0 = in no target or above n_targets"""
    out = []
    for p in parts_of(seq, k):
        lab = np.asarray(ku.lookup(dct, _kmers(p, k), k), np.int64)
        out.append(np.where((lab >= 1) & (lab <= n_targets), lab, 0))
    return out


def rle_words(label_parts, n_targets):
    """the words of one read from its labels per part (any integers: 0 or above n_targets is no target)"""
    words = []
    first = True
    for lab in label_parts:
        lab = [int(x) if 1 <= int(x) <= n_targets else 0 for x in lab]
        if not lab:
            continue
        if not first:
            words.append(0)
        first = False
        for l, grp in itertools.groupby(lab):
            n = len(list(grp))
            assert 1 <= n <= 65535
            words.append((l << 16) | n)
    return words


def read_words(dct, seq, k, n_targets):
    return rle_words(part_labels(dct, seq, k, n_targets), n_targets)


def batch(dct, seqs, k, n_targets):
    """(offsets u32[n + 1], words u32) of the sequences"""
    per = [read_words(dct, s, k, n_targets) for s in seqs]
    off = np.zeros(len(per) + 1, np.uint32)
    off[1:] = np.cumsum([len(w) for w in per])
    return off, np.asarray([w for ws in per for w in ws], np.uint32)


def shown_name(name):
    name = bytes(name)
    return name[:39] if len(name) >= 40 else name


def names_of(text):
    """the reads' names as the result CSV prints them: from the byte behind the marker to the first blank or tab strictly behind the
    first byte, at most 39 bytes"""
    lines = text.split(b"\n")
    hdrs = [ln for ln in lines if ln[:1] == b">"] if text[:1] == b">" else [lines[i] for i in range(0, len(lines) - 1, 4) if lines[i]]
    out = []
    for h in hdrs:
        nm = h[1:]
        cut = min([i for i in (nm.find(b" ", 1), nm.find(b"\t", 1)) if i > 0] + [len(nm)])
        out.append(shown_name(nm[:cut]))
    return out


def format_text(read_names, offsets, words, target_names):
    """the text without its header line (bytes)"""
    out = []
    for r, nm in enumerate(read_names):
        toks = []
        for w in words[int(offsets[r]):int(offsets[r + 1])]:
            w = int(w)
            if w == 0:
                toks.append(b"|")
            else:
                l, n = w >> 16, w & 0xFFFF
                tn = target_names[l - 1] if l else "0"
                toks.append((tn.encode() if isinstance(tn, str) else bytes(tn)) + b":" + str(n).encode())
        out.append(shown_name(nm.encode() if isinstance(nm, str) else nm) + b"," + b" ".join(toks) + b"\n")
    return b"".join(out)


def text_of(dct, text, k, target_names):
    """the hit-map text (no header) of FASTA / FASTQ text against the database"""
    off, words = batch(dct, ku.sequences(text), k, len(target_names))
    return format_text(names_of(text), off, words, target_names)


def sums(offsets, words, n_targets):
    """per read: (sum of len over words with a label, per-target sums u64[n_targets], sum of all len)"""
    n = offsets.size - 1
    hit, per, tot = np.zeros(n, np.int64), np.zeros((n, n_targets), np.int64), np.zeros(n, np.int64)
    for r in range(n):
        for w in words[int(offsets[r]):int(offsets[r + 1])]:
            l, c = int(w) >> 16, int(w) & 0xFFFF
            tot[r] += c
            if l:
                hit[r] += c
                per[r, l - 1] += c
    return hit, per, tot
