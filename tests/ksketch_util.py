"""A restatement in Python of the k-mer sketch rule (csrc/mic_ksketch.h), the estimator and the report (csrc/kmer_report.hpp), and a
walk over the text of reads that gives the k-mers the query counts.  Shared by tests/test_kmer_report.py (which pins the library's
host functions to it) and tests/test_kmer_report_gpu.py (whose expected values all come from here)."""
import math
import os

import numpy as np

import golden_util as gu

P, M, Q = 14, 16384, 50
SEED = 0x9E3779B97F4A7C15
U64 = (1 << 64) - 1
CODE = {c: v for v, cs in enumerate(("Tt Uu", "Gg", "Cc", "Aa")) for c in cs.replace(" ", "").encode()}      # the packer's 2-bit codes


# ---- scalar form: plain Python integers ----------------------------------------------------------------------------------------
def fmix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & U64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & U64
    x ^= x >> 33
    return x


def revcomp(v, k):
    """digit by digit: nucleotide i of the reverse complement is the complement (3 - code) of nucleotide k - 1 - i"""
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (v & 3))
        v >>= 2
    return out


def canonical(v, k):
    return min(v, revcomp(v, k))


def index_rank(c):
    """(register, rank) of canonical k-mer c"""
    h = fmix64(c ^ SEED)
    w = (h << P) & U64
    return h >> Q, (64 - w.bit_length() + 1) if w else Q + 1


def kmer_of(seq):
    """value of a k-mer given as text"""
    v = 0
    for ch in seq if isinstance(seq, bytes) else seq.encode():
        v = (v << 2) | CODE[ch]
    return v


def sketch_scalar(kmers, labels, k, n_targets):
    regs, hits = np.zeros((n_targets, M), np.uint8), np.zeros(n_targets, np.uint64)
    for v, l in zip(kmers, labels):
        if 1 <= l <= n_targets:
            i, r = index_rank(canonical(int(v), k))
            regs[l - 1, i] = max(int(regs[l - 1, i]), r)
            hits[l - 1] += np.uint64(1)
    return regs, hits


# ---- the same on numpy arrays ----------------------------------------------------------------------------------------------------
def _u(x):
    return np.uint64(x)


def canonical_np(v, k):
    v = np.ascontiguousarray(v, np.uint64)
    x = ~v
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> _u(s)) & _u(m)) | ((x & _u(m)) << _u(s))
    x = (x >> _u(32)) | (x << _u(32))
    return np.minimum(v, x >> _u(64 - 2 * k))


def index_rank_np(c):
    x = np.ascontiguousarray(c, np.uint64) ^ _u(SEED)
    x = x ^ (x >> _u(33))
    x = x * _u(0xff51afd7ed558ccd)
    x = x ^ (x >> _u(33))
    x = x * _u(0xc4ceb9fe1a85ec53)
    h = x ^ (x >> _u(33))
    w = h << _u(P)
    bl = np.zeros(w.shape, np.int64)                  # bit length of w
    t = w.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = (t >> _u(s)) != 0
        bl += big * s
        t = np.where(big, t >> _u(s), t)
    bl += t != 0
    return (h >> _u(Q)).astype(np.int64), np.where(w != 0, 64 - bl + 1, Q + 1).astype(np.uint8)


def sketch(kmers, labels, k, n_targets, regs=None, hits=None):
    """labels: 1-based, 0 = no target.  Returns (regs u8[n_targets, M], hits u64[n_targets]); given ones are merged into (copies)."""
    regs = np.zeros((n_targets, M), np.uint8) if regs is None else regs.copy()
    hits = np.zeros(n_targets, np.uint64) if hits is None else hits.copy()
    kmers, labels = np.ascontiguousarray(kmers, np.uint64), np.ascontiguousarray(labels, np.int64)
    keep = (labels >= 1) & (labels <= n_targets)
    if keep.any():
        idx, rank = index_rank_np(canonical_np(kmers[keep], k))
        np.maximum.at(regs, (labels[keep] - 1, idx), rank)
        hits += np.bincount(labels[keep] - 1, minlength=n_targets).astype(np.uint64)
    return regs, hits


def merge(a, b):
    return np.maximum(a[0], b[0]), a[1] + b[1]


# ---- estimator and report ------------------------------------------------------------------------------------------------------
def _sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        zp = z
        z += x * y
        y += y
        if zp == z:
            return z


def _tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        zp = z
        y *= 0.5
        z -= (1.0 - x) ** 2 * y
        if zp == z:
            return z / 3.0


def estimate(regs):
    """Ertl's improved raw estimator on the M registers of one target"""
    c = [int(x) for x in np.bincount(np.minimum(np.asarray(regs, np.int64).reshape(-1), Q + 1), minlength=Q + 2)]
    assert sum(c) == M
    z = M * _tau(1.0 - c[Q + 1] / M)
    for v in range(Q, 0, -1):
        z = 0.5 * (z + float(c[v]))
    z += M * _sigma(c[0] / M)
    return M * M / (2.0 * math.log(2.0) * z) if z > 0.0 else math.inf       # (every register at rank 51: no finite estimate)


def distinct(regs, hits):
    e = estimate(regs)
    v = int(math.floor(e + 0.5)) if e < 9.0e18 else (1 << 63) - 1
    return max(v, 1 if hits else 0)


def ratio_text(num, den):
    q = (num * 100 + den // 2) // den
    return f"{q // 100}.{q % 100:02d}"


def report(names, reads, regs, hits, distinct_of=None):
    out = "Name,Reads,Kmers,DistinctKmers,Duplication\n"
    for t, name in enumerate(names):
        if int(hits[t]):
            d = distinct_of[t] if distinct_of is not None else distinct(regs[t], int(hits[t]))
            out += f"{name},{int(reads[t])},{int(hits[t])},{d},{ratio_text(int(hits[t]), d)}\n"
    return out


# ---- the k-mers of reads, from their text ------------------------------------------------------------------------------------------
def sequences(text):
    """the sequences of FASTA (lines joined) or four-line FASTQ text"""
    lines = text.split(b"\n")
    if text[:1] == b">":
        out = []
        for ln in lines:
            if ln[:1] == b">":
                out.append(b"")
            elif out:
                out[-1] += ln.rstrip(b"\r")
        return out
    return [lines[i].rstrip(b"\r") for i in range(1, len(lines), 4)]


_LUT = np.full(256, 255, np.uint8)
for _c, _v in CODE.items():
    _LUT[_c] = _v


def seq_kmers(seq, k):
    """k-mers (as they read) of every maximal run of nucleotides: anything else ('N', a masked base) belongs to no k-mer"""
    codes = _LUT[np.frombuffer(seq, np.uint8)]
    out = []
    edges = np.flatnonzero(np.diff(np.concatenate(([True], codes == 255, [True])).astype(np.int8)))
    for a, b in zip(edges[::2], edges[1::2]):
        if b - a >= k:
            n = b - a - k + 1
            v = np.zeros(n, np.uint64)
            for j in range(k):
                v = (v << _u(2)) | codes[a + j:a + j + n].astype(np.uint64)
            out.append(v)
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def db_dict_arrays(sizes_idx, sizes_val, keys, labels, htsize):
    """(sorted canonical k-mers u64, their 1-based labels) of a database given as non-empty buckets, keys and 0-based labels"""
    bucket = np.repeat(np.asarray(sizes_idx, np.uint64), np.asarray(sizes_val, np.int64))
    canon = np.asarray(keys, np.uint64) * _u(htsize) + bucket
    order = np.argsort(canon)
    return canon[order], np.asarray(labels, np.int64)[order] + 1


def golden_dict(name):
    db = gu.load_golden_db(name)
    return db_dict_arrays(db["sz_idx"], db["sz_val"], db["ky"], db["lb"], db["htsize"]), db


def lookup(dct, kmers, k):
    """1-based labels (0: not in the database) of k-mers as they read"""
    canon, lab = dct
    c = canonical_np(kmers, k)
    if canon.size == 0 or c.size == 0:
        return np.zeros(c.size, np.int64)
    pos = np.minimum(np.searchsorted(canon, c), canon.size - 1)
    return np.where(canon[pos] == c, lab[pos], 0)


def reads_sketch(dct, seqs, k, n_targets):
    """(regs, hits, hits per read) of the sequences against the database"""
    kms = [seq_kmers(s, k) for s in seqs]
    lbs = [lookup(dct, km, k) for km in kms]
    per_read = np.array([int(np.count_nonzero((lb >= 1) & (lb <= n_targets))) for lb in lbs], np.int64)
    regs, hits = sketch(np.concatenate(kms) if kms else [], np.concatenate(lbs) if lbs else [], k, n_targets)
    return regs, hits, per_read


GOLDEN_READS = {20: "reads_k27.fa", 27: "reads_k27.fq", 31: "reads_k31.fq", 32: "reads_k31.fa"}


def golden_reads(k):
    return open(os.path.join(gu.GOLDEN, GOLDEN_READS[k]), "rb").read()
