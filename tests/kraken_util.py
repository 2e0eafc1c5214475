"""A restatement in Python of the Kraken per-read line (csrc/mic_kraken.h) and of the Kraken sample report (csrc/kraken_report.hpp).
Result rows come from per-target k-mer counts (hitmap_util.sums) through the top-2 rule: an ascending scan over the targets, best by
strict >, second by else-if >.  Shared by tests/test_kraken_out.py (which pins the library's host function and exe/estimate_abundance
to it) and tests/test_kraken_out_gpu.py (whose expected bytes all come from here)."""
import numpy as np

import hitmap_util as hu
import ksketch_util as ku

DEFAULT = (5, 10, 0, 1)            # -c 0.5 -g 0 as (conf_num, conf_den, gamma_num, gamma_den)


def filt(conf="0.5", gamma="0"):
    """a filter as exact integers from decimal strings"""
    def frac(s):
        whole, _, dec = s.partition(".")
        return int(whole + dec), 10 ** len(dec)
    return frac(conf) + frac(gamma)


def rows_from_counts(per):
    """result rows u32[n, 8] {sum, idxBest, best, idxSecond, second, targets hit, 0, 0} from per-target counts [n, T]"""
    per = np.asarray(per, np.int64)
    out = np.zeros((per.shape[0], 8), np.uint32)
    for r, row in enumerate(per):
        best = ib = second = i2 = hit = 0
        for t, c in enumerate(row.tolist()):
            if not c:
                continue
            hit += 1
            if c > best:
                second, i2, best, ib = best, ib, c, t + 1
            elif c > second:
                second, i2 = c, t + 1
        out[r, :6] = (int(row.sum()), ib, best, i2, second, hit)
    return out


def classified(res, norm, k, n_targets, f=DEFAULT):
    """bucket >= 2 of the abundance rule (csrc/mic_abund.h): the predicate of --classified-out"""
    total, ib, best, second = int(res[0]), int(res[1]), int(res[2]), int(res[4])
    if ib == 0 or ib > n_targets:
        return False
    cn, cd, gn, gd = f
    den = int(norm) - k + 1
    return best * cd >= cn * (best + second) and (gn == 0 or (den > 0 and total * gd >= gn * den))


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def map_field(words, target_names):
    n_targets = len(target_names)
    toks = []
    for w in words:
        w = int(w)
        if w == 0:
            toks.append(b"|:|")
            continue
        l, n = w >> 16, w & 0xFFFF
        toks.append((b"0" if l == 0 else b"NA" if l > n_targets else _b(target_names[l - 1])) + b":" + str(n).encode())
    return b" ".join(toks) if toks else b"0:0"


def format_text(read_names, res, norm, k, f, offsets, words, target_names):
    out = []
    T = len(target_names)
    for r, nm in enumerate(read_names):
        cls = classified(res[r], norm[r], k, T, f)
        out.append(b"\t".join([b"C" if cls else b"U", hu.shown_name(_b(nm)), _b(target_names[int(res[r][1]) - 1]) if cls else b"0", str(int(norm[r])).encode(),
                               map_field(words[int(offsets[r]):int(offsets[r + 1])], target_names)]) + b"\n")
    return b"".join(out)


def rows_of(dct, text, k, n_targets, paired=False):
    """(names, result rows, norm, offsets, words) of FASTA / FASTQ text against the database; paired: the text is merged mates"""
    seqs = ku.sequences(text)
    off, words = hu.batch(dct, seqs, k, n_targets)
    _, per, _ = hu.sums(off, words, n_targets)
    norm = np.array([len(s) - (1 if paired else 0) for s in seqs], np.int64)
    return hu.names_of(text), rows_from_counts(per), norm, off, words


def text_of(dct, text, k, target_names, f=DEFAULT, paired=False):
    names, res, norm, off, words = rows_of(dct, text, k, len(target_names), paired)
    return format_text(names, res, norm, k, f, off, words, target_names)


# ---- the sample report -------------------------------------------------------------------------------------------------------------
CODES = {"superkingdom": "D", "domain": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G", "species": "S"}


def pct(clade, total):
    h = (20000 * clade + total) // (2 * total) if total else 0
    return "%3d.%02d" % (h // 100, h % 100)


def report(unassigned, filtered, per_target, targets, levels=(), ranks=(), target_rank="species"):
    """targets: [(name, taxid)] per target; levels: per level 1 .. L a list of (name, taxid) per target (the target's group at that
    level: equal pairs = one group, numbered by first appearance); ranks: the levels' rank names; taxid "UNKNOWN" prints 0"""
    T, L = len(targets), len(levels)
    groups, group_of = [list(targets)], [list(range(T))]
    for lv in levels:
        ids = {}
        for key in lv:
            ids.setdefault(key, len(ids))
        groups.append(list(ids))
        group_of.append([ids[key] for key in lv])
    clade = [[0] * len(g) for g in groups]
    kids = [[[] for _ in g] for g in groups]
    for t in range(T):
        for l in range(L + 1):
            clade[l][group_of[l][t]] += int(per_target[t])
            if l and group_of[l - 1][t] not in kids[l][group_of[l][t]]:
                kids[l][group_of[l][t]].append(group_of[l - 1][t])
    unclassified, n_classified = int(unassigned) + int(filtered), sum(int(x) for x in per_target)
    total = unclassified + n_classified
    out = []

    def line(cl, tx, code, taxid, depth, name):
        out.append("%s\t%d\t%d\t%s\t%s\t%s%s\n" % (pct(cl, total), cl, tx, code, "0" if taxid == "UNKNOWN" else taxid, "  " * depth, name))

    def siblings(nodes):
        flat = []
        for l, g in nodes:
            if l and any(groups[l - 1][c] == groups[l][g] for c in kids[l][g]):
                flat += siblings([(l - 1, c) for c in kids[l][g]])      # an inherited rank: its children take its place
            else:
                flat.append((l, g))
        return flat

    def walk(nodes, depth):
        keep = [n for n in siblings(nodes) if clade[n[0]][n[1]]]
        for l, g in sorted(keep, key=lambda n: (-clade[n[0]][n[1]], groups[n[0]][n[1]][0].encode(), n[0], n[1])):
            name, taxid = groups[l][g]
            line(clade[l][g], clade[0][g] if l == 0 else 0, CODES.get(target_rank if l == 0 else ranks[l - 1], "-"), taxid, depth, name)
            if l:
                walk([(l - 1, c) for c in kids[l][g]], depth + 1)

    if unclassified:
        line(unclassified, unclassified, "U", "0", 0, "unclassified")
    if n_classified:
        line(n_classified, 0, "R", "1", 0, "root")
    walk([(L, g) for g in range(len(groups[L]))], 1)
    return "".join(out)
