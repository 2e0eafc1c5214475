"""Shared by test_rollup.py and test_rollup_gpu.py: a restatement of the rank roll-up rule in plain Python (written from the
rule's text, not from csrc/mic_rollup.h), the report's text from counters, random lineages, and the seeded chimeric reads over the
golden genomes.  Expected values come from here and from the CPU oracle's per-target counts, never from the code under test."""
import os
from fractions import Fraction

import numpy as np

import golden_util as gu

UNRESOLVED, PENDING = 0xFFFFFFFF, 0xFFFFFFFE
ROW_INVALID = 0xFFFFFFFF
FILTERS = [("0.5", "0"), ("0.75", "0.03"), ("0.9", "0.5")]
GOLDEN_LINEAGE = np.array([[0, 0, 1, 1, 2, 2], [0, 0, 0, 0, 1, 1]], np.uint16)

GOLDEN_RANKS = ["target", "genus", "family"]
GOLDEN_GROUPS = [None, ["G_ab", "G_cd", "G_es"], ["F_abcd", "F_es"]]


def golden_lineage_file(path, header=True):
    names = gu.target_names()
    with open(path, "w") as f:
        if header:
            f.write("#label\tgenus\tfamily\n")
        for t in reversed(range(len(names))):            # (any order of lines)
            f.write(f"{names[t]}\t{GOLDEN_GROUPS[1][GOLDEN_LINEAGE[0][t]]}\t{GOLDEN_GROUPS[2][GOLDEN_LINEAGE[1][t]]}\n")


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def scan(pairs):
    """best / second-best over (id, count) pairs in ascending id: strictly greater replaces best, else strictly greater replaces
    second.  Returns (idxBest, best, idxSecond, second), indices id + 1, 0 = none."""
    ib = best = isec = second = 0
    for g, c in pairs:
        if c > best:
            isec, second = ib, best
            ib, best = g + 1, c
        elif c > second:
            isec, second = g + 1, c
    return ib, best, isec, second


def layout(T, group_of):
    group_of = np.asarray(group_of).reshape(-1, T)
    n_groups = [T] + [int(group_of[l].max()) + 1 for l in range(group_of.shape[0])]
    off = [0]
    for l in range(1, len(n_groups)):
        off.append(off[-1] + n_groups[l - 1])
    return n_groups, off, 2 + sum(n_groups)


def restate(reads, norm, k, T, group_of, c, g):
    """reads: per read None (row not available) or a list of (target, count) in ascending target order.
    Returns (rollup u32[n, 8], levels u32[n, L + 1, 4], counters u64)."""
    group_of = np.asarray(group_of).reshape(-1, T)
    L = group_of.shape[0]
    n_groups, off, n_counters = layout(T, group_of)
    C, G = Fraction(c), Fraction(g)
    rollup = np.zeros((len(reads), 8), np.uint32)
    levels = np.zeros((len(reads), L + 1, 4), np.uint32)
    counters = np.zeros(n_counters, np.uint64)
    for r, pairs in enumerate(reads):
        if pairs is None:
            rollup[r, 5], rollup[r, 6] = PENDING, 1
            continue
        pairs = [(int(t), int(cn)) for t, cn in pairs if cn > 0]
        total = sum(cn for _, cn in pairs)
        if total == 0:
            counters[0] += 1
            continue
        per_level, hit = [], []
        for l in range(L + 1):
            if l == 0:
                grp = dict(pairs)
            else:
                grp = {}
                for t, cn in pairs:
                    gid = int(group_of[l - 1][t])
                    grp[gid] = grp.get(gid, 0) + cn
            per_level.append(scan(sorted(grp.items())))
            hit.append(len(grp))
            levels[r, l] = per_level[-1]
        den = (int(norm[r]) if norm is not None else 0) - k + 1
        gamma = G == 0 or (den > 0 and Fraction(total, den) >= G)
        level = UNRESOLVED
        if gamma:
            for l in range(L + 1):
                ib, best, _, second = per_level[l]
                if Fraction(best, best + second) >= C:
                    level = l
                    break
        at = 0 if level == UNRESOLVED else level
        rollup[r] = (total,) + per_level[at] + (level, 0, hit[at])
        counters[1 if level == UNRESOLVED else 2 + off[level] + per_level[level][0] - 1] += 1
    return rollup, levels, counters


def pairs_of_dense(counts):
    return [[(int(t), int(row[t])) for t in np.flatnonzero(row)] for row in counts]


def pairs_of_rows(rows):
    out = []
    for row in rows:
        n = int(row[0])
        out.append(None if n == ROW_INVALID else [(int(v) & 0xFFFF, int(v) >> 16) for v in row[1:1 + n]])
    return out


# ---- the report ----------------------------------------------------------------------------------------------------------------
def pct(count, den):
    return "0" if den == 0 else "%g" % (100.0 * count / den)


def report(counters, T, group_of, ranks, names, taxids=None):
    """names[l][g] / taxids[l][g] for l = 0 .. L; ranks[l]."""
    group_of = np.asarray(group_of).reshape(-1, T)
    L = group_of.shape[0]
    n_groups, off, _ = layout(T, group_of)
    total = int(counters.sum())
    reads = [[int(counters[2 + off[l] + g]) for g in range(n_groups[l])] for l in range(L + 1)]
    clade = [list(reads[0])]
    for l in range(1, L + 1):
        cl = list(reads[l])
        below = {}                                  # group of level l - 1 -> its group at level l
        for t in range(T):
            below[t if l == 1 else int(group_of[l - 2][t])] = int(group_of[l - 1][t])
        for lo, hi in below.items():
            cl[hi] += clade[l - 1][lo]
        clade.append(cl)
    out = ["Level,Rank,Name,TaxID,Reads,CladeReads,Proportion_All(%)"]
    for l in range(L, -1, -1):
        rows = [g for g in range(n_groups[l]) if clade[l][g]]
        rows.sort(key=lambda g: (-clade[l][g], names[l][g].encode(), g))
        for g in rows:
            tid = taxids[l][g] if taxids else "UNKNOWN"
            out.append(f"{l},{ranks[l]},{names[l][g]},{tid},{reads[l][g]},{clade[l][g]},{pct(clade[l][g], total)}")
    out.append(f"-,-,UNRESOLVED,UNKNOWN,{int(counters[1])},{int(counters[1])},{pct(int(counters[1]), total)}")
    out.append(f"-,-,UNKNOWN,UNKNOWN,{int(counters[0])},{int(counters[0])},{pct(int(counters[0]), total)}")
    return "\n".join(out) + "\n"


# ---- lineages ------------------------------------------------------------------------------------------------------------------
def first_appearance(a):
    ids, out = {}, np.zeros(len(a), np.uint16)
    for i, v in enumerate(a):
        out[i] = ids.setdefault(int(v), len(ids))
    return out


def random_lineage(rng, T, L):
    """u16[L, T]: every level a coarsening of the one below, ids by first appearance."""
    out = np.zeros((L, T), np.uint16)
    cur = np.arange(T)
    n = T
    for l in range(L):
        n_next = max(1, int(n // rng.integers(2, 5)))
        parent = rng.integers(0, n_next, n)
        cur = first_appearance(parent[cur])
        out[l] = cur
        n = int(cur.max()) + 1
    return out


# ---- chimeric reads over the golden genomes ------------------------------------------------------------------------------------
def golden_genomes():
    out = []
    for fn, _ in gu.target_files_and_labels():
        lines = open(fn).read().split("\n")
        out.append("".join(l.strip() for l in lines if l and not l.startswith(">")))
    return out


def chimeric_reads(n=4000, seed=2026, length=150):
    """n reads of `length` nt: 1-3 pieces (cut points uniform in [20, 130]) taken at uniform places from the genome files chosen
    uniformly; every 50th read random nucleotides.  Returns the list of sequences."""
    rng = np.random.default_rng(seed)
    genomes = golden_genomes()
    seqs = []
    for i in range(n):
        if i % 50 == 49:
            seqs.append("".join("ACGT"[j] for j in rng.integers(0, 4, length)))
            continue
        pieces = int(rng.integers(1, 4))
        cuts = [0] + sorted(int(x) for x in rng.integers(20, 131, pieces - 1)) + [length]
        s = ""
        for a, b in zip(cuts[:-1], cuts[1:]):
            gen = genomes[int(rng.integers(0, len(genomes)))]
            at = int(rng.integers(0, len(gen) - (b - a) + 1))
            s += gen[at:at + (b - a)]
        seqs.append(s)
    return seqs


def fasta(seqs):
    return "".join(f">c{i}\n{s}\n" for i, s in enumerate(seqs)).encode()


def fastq(seqs, tag=""):
    return "".join(f"@c{i}{tag}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(seqs)).encode()


def oracle_counts(dbname, data, paired=False):
    """(per-target counts u32[n, T], Length column, k, extended CSV text) of the CPU oracle for the bytes of a FASTA / FASTQ file."""
    odb, db = gu.oracle_db_from_golden(dbname)
    orc = gu.oracle()
    names = gu.target_names()
    k = db["k"]
    idx = orc.index_reads(data)
    rp, cont = orc.pack_batch(data, idx["seq_s"], idx["seq_e"], idx["length"], k)
    counts, bad = odb.query_batch(k, rp, cont, len(names))
    assert bad == 0
    norm = idx["length"].astype(np.int64) - (1 if paired else 0)
    text, _ = odb.classify_file(k, data, names, paired, True)
    return counts, norm.astype(np.uint32), k, text


def outcome_shares(rollup):
    n = rollup.shape[0]
    lv = rollup[:, 5]
    nohit = int(((rollup[:, 0] == 0)).sum())
    out = {"nohit": nohit, "unresolved": int((lv == UNRESOLVED).sum())}
    for l in range(3):
        out[f"level{l}"] = int(((lv == l) & (rollup[:, 0] > 0)).sum())
    return {k: v / n for k, v in out.items()}
