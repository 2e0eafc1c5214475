"""A restatement in Python of the table census rule (csrc/mic_census.h) without a table, of the count the census must give - every
k-mer of the file looked up in the oracle's database and counted by the label found - and of the coverage report
(csrc/kmer_report.hpp: format_coverage).  Shared by tests/test_kmer_coverage.py and tests/test_kmer_coverage_gpu.py."""
import numpy as np

import golden_util as gu
import ksketch_util as ku

HEADER = "Name,Reads,Kmers,DistinctKmers,Duplication,TargetKmers,Coverage"
# (found, answered elsewhere, not canonical, lost, found with a label at or above n_targets)
FOUND, ELSEWHERE, NONCANONICAL, LOST, BEYOND = 0, 1, 2, 3, 4


def census(sizes, keys, labels, k, n_targets, sampling=1):
    """the rule entry by entry, in plain integers: (counts, stats) as lists"""
    htsize = len(sizes)
    counts, stats = [0] * n_targets, [0] * 8
    off = rank = 0
    for b, sz in enumerate(int(s) for s in sizes):
        if not sz:
            continue
        rank += 1
        if sampling <= 1 or rank % sampling == 0:
            last, run = int(keys[off + sz - 1]), None
            for e in range(sz):
                kv = int(keys[off + e])
                rising = run is None or kv > run
                reach = rising and kv <= last
                if rising:
                    run = kv
                if not reach:
                    continue
                c = (kv * htsize + b) & ku.U64
                if c > ku.revcomp(c, k):
                    stats[NONCANONICAL] += 1
                    continue
                stats[FOUND] += 1
                lab = int(labels[off + e])
                if lab < n_targets:
                    counts[lab] += 1
                else:
                    stats[BEYOND] += 1
        off += sz
    return counts, stats


def oracle_counts(sizes, keys, labels, k, n_targets, sampling=1):
    """(counts by the label found, k-mers found, the oracle database's n_elems): every distinct canonical c = key * htsize + bucket of
    the file looked up in the oracle's database at this sampling"""
    sizes = np.ascontiguousarray(sizes, np.uint8)
    htsize = sizes.size
    bucket = np.repeat(np.arange(htsize, dtype=np.uint64), sizes.astype(np.int64))
    c = np.unique(np.asarray(keys, np.uint64) * np.uint64(htsize) + bucket)
    c = c[ku.canonical_np(c, k) == c]
    odb = gu.oracle().db_from_arrays(sizes, keys, labels, sampling)
    found, lab = odb.find_many(c, k)
    lab = lab[found == 1].astype(np.int64)
    counts = np.bincount(lab[lab < n_targets], minlength=n_targets).astype(np.uint64)
    return counts, int(found.sum()), odb.n_elems


def ratio6(num, den):
    q = (num * 1000000 + den // 2) // den
    return f"{q // 1000000}.{q % 1000000:06d}"


def report(names, reads, regs, hits, target_kmers, distinct_of=None):
    """the k-mer report's lines (ksketch_util.report) with TargetKmers and Coverage behind them"""
    out = HEADER + "\n"
    for t, name in enumerate(names):
        if int(hits[t]):
            d = distinct_of[t] if distinct_of is not None else ku.distinct(regs[t], int(hits[t]))
            tk = int(target_kmers[t])
            assert tk > 0, name
            out += f"{name},{int(reads[t])},{int(hits[t])},{d},{ku.ratio_text(int(hits[t]), d)},{tk},{ratio6(min(d, tk), tk)}\n"
    return out
