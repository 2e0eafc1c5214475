"""Rank roll-up on the CPU: the library's host rule (mic_rollup_host, mic_rollup_check) and exe/estimate_abundance --rank-report
against the plain-Python restatement of the rule in rollup_util.py, on random rows and on chimeric reads over the golden databases
(per-target counts from the CPU oracle).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import rollup_util as ru
from test_targets_tools import make_taxonomy

EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")


def _est(*args):
    assert os.path.exists(EST), "exe/estimate_abundance is not built (build() makes it)"
    return subprocess.run([EST, *args], capture_output=True, text=True, timeout=300)


def random_rows(rng, n, T, rw, tie_heavy):
    """u32[n, rw] sparse rows (ascending targets): 0 / 1 / full rows, ties, counts of 65535, and invalid rows."""
    rows = np.zeros((n, rw), np.uint32)
    cap = min(rw - 1, T)
    for r in range(n):
        u = rng.random()
        if u < 0.08:
            rows[r, 0] = ru.ROW_INVALID
            rows[r, 1:] = rng.integers(0, 2 ** 32, rw - 1, dtype=np.uint64)      # (what an overflowed row leaves behind)
            continue
        ne = 0 if u < 0.18 else 1 if u < 0.35 else cap if u < 0.45 else int(rng.integers(1, cap + 1))
        tg = np.sort(rng.choice(T, ne, replace=False))
        if tie_heavy:
            cn = rng.integers(1, 4, ne)
        else:
            cn = rng.integers(1, 300, ne)
            cn[rng.random(ne) < 0.05] = 65535
        rows[r, 0] = ne
        rows[r, 1:1 + ne] = (cn.astype(np.uint32) << 16) | tg.astype(np.uint32)
    return rows


def dense_of(pairs, T):
    d = np.zeros((len(pairs), T), np.uint32)
    for r, p in enumerate(pairs):
        for t, c in (p or []):
            d[r, t] = c
    return d


@pytest.mark.parametrize("T", [2, 6, 4096, 65535])
@pytest.mark.parametrize("L", [1, 3, 7])
def test_host_rule_equals_the_restatement(lib, T, L):
    from cuclark_amd import host
    rng = np.random.default_rng(1000 * L + T)
    gof = ru.random_lineage(rng, T, L)
    host.rollup_check(T, gof)
    k = 31
    for rw in (16, 65):
        n = 400 if T > 4096 else 1500
        rows = random_rows(rng, n, T, rw, tie_heavy=(rw == 16))
        pairs = ru.pairs_of_rows(rows)
        norm = rng.integers(20, 400, n).astype(np.uint32)
        # dense counts for the invalid rows: more targets than any row holds (when T allows), or a count above 65535
        full = []
        for r, p in enumerate(pairs):
            if p is None:
                m = min(T, int(rng.integers(1, 130)))
                tg = np.sort(rng.choice(T, m, replace=False))
                cn = rng.integers(1, 5, m)
                if m <= rw - 1:
                    cn[0] = 70000
                full.append(list(zip(tg.tolist(), cn.tolist())))
            else:
                full.append(p)
        dense = dense_of(full, T)
        for c, g in ru.FILTERS:
            f = host.abund_filter(c, g)
            # rows only: invalid rows come back pending and uncounted
            want = ru.restate(pairs, norm, k, T, gof, c, g)
            got = host.rollup_host(rows, norm, k, T, gof, f, want_levels=True)
            for a, b, what in zip(got, want, ("rollup", "levels", "counters")):
                assert (a == b).all(), (what, T, L, rw, c, g)
            assert int(got[2].sum()) == sum(p is not None for p in pairs)
            # rows + dense counts for the invalid ones: complete, every read in exactly one counter
            want = ru.restate(full, norm, k, T, gof, c, g)
            want[0][[p is None for p in pairs], 6] = 2          # MIC_FLAG_DENSE_PATH
            got = host.rollup_host(rows, norm, k, T, gof, f, dense=dense, want_levels=True)
            for a, b, what in zip(got, want, ("rollup", "levels", "counters")):
                assert (a == b).all(), (what, T, L, rw, c, g, "with dense")
            assert int(got[2].sum()) == n
            # the dense form alone agrees with the rows form
            alone = host.rollup_host(None, norm, k, T, gof, f, dense=dense, want_levels=True)
            assert (alone[0][:, [0, 1, 2, 3, 4, 5, 7]] == got[0][:, [0, 1, 2, 3, 4, 5, 7]]).all()
            assert (alone[1] == got[1]).all() and (alone[2] == got[2]).all()
    with pytest.raises(ValueError):
        host.rollup_host(rows, None, k, T, gof, host.abund_filter("0.5", "0.1"))         # gamma without lengths


def test_walks_up_only_as_far_as_needed(lib):
    """A hand-made read: species split 5 / 5 inside one genus, 2 in another genus of the same family."""
    from cuclark_amd import host
    gof = np.array([[0, 0, 1, 1], [0, 0, 0, 0]], np.uint16)
    rows = np.zeros((1, 16), np.uint32)
    rows[0, :4] = [3, (5 << 16) | 0, (5 << 16) | 1, (2 << 16) | 2]
    r, lv, cnt = host.rollup_host(rows, None, 31, 4, gof, host.abund_filter("0.5", "0"), want_levels=True)
    assert r[0].tolist() == [12, 1, 5, 2, 5, 0, 0, 3] and cnt[2 + 0] == 1                       # 0.5 passes at level 0 (tie: lowest id)
    assert lv[0].tolist() == [[1, 5, 2, 5], [1, 10, 2, 2], [1, 12, 0, 0]]
    r, _, cnt = host.rollup_host(rows, None, 31, 4, gof, host.abund_filter("0.75", "0"))
    assert r[0].tolist() == [12, 1, 10, 2, 2, 1, 0, 2] and cnt[2 + 4 + 0] == 1                   # 10 / 12 at the genus
    r, _, cnt = host.rollup_host(rows, None, 31, 4, gof, host.abund_filter("0.9", "0"))
    assert r[0].tolist() == [12, 1, 12, 0, 0, 2, 0, 1] and cnt[2 + 4 + 2 + 0] == 1               # only the family
    r, _, cnt = host.rollup_host(rows, np.array([150], np.uint32), 31, 4, gof, host.abund_filter("0.5", "0.5"))
    assert r[0].tolist() == [12, 1, 5, 2, 5, ru.UNRESOLVED, 0, 3] and cnt[1] == 1                # gamma 12 / 120 fails everywhere


def test_check_refuses_bad_lineages(lib):
    from cuclark_amd import host
    host.rollup_check(6, ru.GOLDEN_LINEAGE)
    host.rollup_check(4, [[0, 1, 0, 2]])
    bad = {
        "not first appearance (starts at 1)": (4, [[1, 0, 0, 2]]),
        "not first appearance (skips an id)": (4, [[0, 0, 2, 1]]),
        "not a coarsening": (4, [[0, 0, 1, 1], [0, 1, 1, 1]]),
        "not a coarsening at the top": (6, [[0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 2, 2], [0, 1, 1, 1, 1, 1]]),
        "no level": (4, np.zeros((0, 4), np.uint16)),
        "eight levels": (4, np.zeros((8, 4), np.uint16)),
    }
    for what, (T, g) in bad.items():
        with pytest.raises(ValueError):
            host.rollup_check(T, g)
        assert lib.mic_rollup_host(None, 0, None, None, 0, 31, T, len(g), np.ascontiguousarray(g, np.uint16).ctypes.data if len(g) else None,
                                   ctypes.byref(host.abund_filter()), None, None, None) != 0, what
    with pytest.raises(ValueError) as ei:
        host.rollup_check(4, [[0, 0, 1, 1], [0, 1, 1, 1]])
    assert "level 2" in str(ei.value) and "target 1" in str(ei.value)


# ---- chimeric reads on the golden databases ----------------------------------------------------------------------------------------
GOLDEN_RANKS, GOLDEN_GROUPS, golden_lineage_file = ru.GOLDEN_RANKS, ru.GOLDEN_GROUPS, ru.golden_lineage_file


@pytest.mark.parametrize("dbname", ["full_k31_u32", "light_k27_u32"])
def test_chimeric_reads_report_equals_the_restatement(tmp_path, dbname):
    names = gu.target_names()
    T = len(names)
    seqs = ru.chimeric_reads()
    data = ru.fasta(seqs)
    counts, norm, k, ext_csv = ru.oracle_counts(dbname, data)
    pairs = ru.pairs_of_dense(counts)
    rollup, _, _ = ru.restate(pairs, norm, k, T, ru.GOLDEN_LINEAGE, "0.75", "0")
    shares = ru.outcome_shares(rollup)
    print(dbname, {a: round(100 * b, 2) for a, b in shares.items()})
    for what, share in shares.items():
        assert share >= 0.01, (what, shares)                   # every outcome holds at least 1 % of the reads
    csv = os.path.join(str(tmp_path), "ext.csv")
    open(csv, "wb").write(ext_csv)
    lin = os.path.join(str(tmp_path), "lineage.tsv")
    golden_lineage_file(lin)
    group_names = [names] + GOLDEN_GROUPS[1:]
    for c, flags in [("0.75", ["-c", "0.75"]), ("0.5", []), ("0.9", ["-c", "0.9"]), ("1", ["-c", "1"])]:
        out = os.path.join(str(tmp_path), f"report_{c}.csv")
        r = _est("-F", csv, "--rank-report", out, "--lineage", lin, *flags)
        assert r.returncode == 0, r.stderr
        _, _, counters = ru.restate(pairs, norm, k, T, ru.GOLDEN_LINEAGE, c, "0")
        want = ru.report(counters, T, ru.GOLDEN_LINEAGE, GOLDEN_RANKS, group_names)
        got = open(out).read()
        assert got == want, (dbname, c)
        body = [l.split(",") for l in got.splitlines()[1:]]
        assert sum(int(l[4]) for l in body) == len(seqs)                                   # Reads + UNRESOLVED + UNKNOWN
        assert sum(int(l[5]) for l in body if l[0] in ("2", "-")) == len(seqs)             # top-level clades likewise
        # the abundance table on stdout is what it is without the flag
        assert r.stdout == _est("-F", csv, *flags).stdout
    # with CLARK's default filter every read with a hit resolves at level 0
    assert "-,-,UNRESOLVED,UNKNOWN,0,0,0\n" in open(os.path.join(str(tmp_path), "report_0.5.csv")).read()
    # --highconfidence: the gamma test is level-independent
    out = os.path.join(str(tmp_path), "hc.csv")
    assert _est("-F", csv, "--rank-report", out, "--lineage", lin, "--highconfidence").returncode == 0
    _, _, counters = ru.restate(pairs, norm, k, T, ru.GOLDEN_LINEAGE, "0.75", "0.03")
    assert open(out).read() == ru.report(counters, T, ru.GOLDEN_LINEAGE, GOLDEN_RANKS, group_names)


def test_rank_report_refusals(tmp_path):
    tmp = str(tmp_path)
    ext = os.path.join(gu.GOLDEN, "expected_k31_fa_ext.csv")
    plain = os.path.join(gu.GOLDEN, "expected_k31_fa.csv")
    lin = os.path.join(tmp, "lineage.tsv")
    golden_lineage_file(lin, header=False)
    out = os.path.join(tmp, "o.csv")
    r = _est("-F", ext, "--rank-report", out, "--lineage", lin)
    assert r.returncode == 0, r.stderr
    assert ",level1," in open(out).read() and ",target," in open(out).read()
    r = _est("-F", plain, "--rank-report", out, "--lineage", lin)
    assert r.returncode != 0 and "extended" in r.stderr
    r = _est("-F", ext, "--rank-report", out)
    assert r.returncode != 0                                         # neither --lineage nor -D
    r = _est("-F", ext, "--lineage", lin)
    assert r.returncode != 0
    names = gu.target_names()
    cases = {
        "T_beta": [f"{n}\t{'X' if n in ('T_alpha', 'T_beta') else 'Y'}\t{'P' if n != 'T_beta' else 'Q'}" for n in names],    # not nested
        "T_gamma": [f"{n}\tX\tP" for n in names if n != "T_gamma"],                                                       # a label missing
        "nobody": [f"{n}\tX\tP" for n in names] + ["nobody\tX\tP"],                                                        # an unknown label
        "S6": [f"{n}\tX\tP" for n in names] + ["S6\tX\tP"],                                                                # twice
        "T_delta": [f"{n}\tX\tP" if n != "T_delta" else f"{n}\tX" for n in names],                                          # another L
    }
    for label, lines in cases.items():
        open(lin, "w").write("\n".join(lines) + "\n")
        r = _est("-F", ext, "--rank-report", out, "--lineage", lin)
        assert r.returncode != 0 and label in r.stderr, (label, r.stderr)


# ---- the lineage from a taxonomy -----------------------------------------------------------------------------------------------
def test_lineage_from_a_taxonomy(tmp_path):
    """test_targets_tools' taxonomy: 562 and 1001 (under a 'species group') in genus 561, 573 in genus 570, both genera in family
    543; 83333 is a strain of 562.  The family 543 as a label of its own keeps only the ranks above it; a custom label stays alone;
    9999 is not a node."""
    tmp = str(tmp_path)
    make_taxonomy(os.path.join(tmp, "DB", "taxonomy"))
    dbdir = os.path.join(tmp, "DB", "custom_0")
    os.makedirs(dbdir)
    labels = ["562", "573", "custom_x", "1001", "543", "83333", "9999"]
    csv = os.path.join(tmp, "e.csv")
    with open(csv, "w") as f:
        f.write("Object_ID," + ",".join(labels) + ",Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\n")
        f.write("a,5,0,0,5,0,0,0,150,0.1,562,5,1001,5,0.5\n")          # split inside genus 561
        f.write("b,5,5,0,0,0,0,0,150,0.1,562,5,573,5,0.5\n")           # split between the genera of family 543
        f.write("c,0,0,5,0,0,0,5,150,0.1,custom_x,5,9999,5,0.5\n")     # two labels the taxonomy does not know: never resolved
        f.write("d,5,0,0,0,5,0,0,150,0.1,562,5,543,5,0.5\n")           # a species and its family as a label: the family level
        f.write("e,0,0,0,0,0,9,0,150,0.1,83333,9,NA,0,1\n")
        f.write("f,0,0,0,0,0,0,0,150,0,NA,0,NA,0,0\n")
    out = os.path.join(tmp, "r.csv")
    r = _est("-F", csv, "--rank-report", out, "-D", dbdir, "-c", "0.75")
    assert r.returncode == 0, r.stderr
    got = open(out).read().splitlines()
    # expected lineage, by hand: level 1 genus .. 6 superkingdom; a missing rank inherits the group below
    #          562   573   custom 1001  543   83333 9999
    genus = [0, 1, 2, 0, 3, 0, 4]
    family = [0, 0, 1, 0, 0, 0, 2]                      # 543 itself joins its family's group only ABOVE the family level ...
    # ... so at the family level the label 543 is alone (ranks above the label's own only)
    family = [0, 0, 1, 0, 2, 0, 3]
    order = [0, 0, 1, 0, 0, 0, 2]
    gof = np.array([genus, family, order, order, order, order], np.uint16)
    from cuclark_amd import host
    host.rollup_check(len(labels), gof)
    dense = np.array([[5, 0, 0, 5, 0, 0, 0], [5, 5, 0, 0, 0, 0, 0], [0, 0, 5, 0, 0, 0, 5], [5, 0, 0, 0, 5, 0, 0], [0, 0, 0, 0, 0, 9, 0],
                      [0, 0, 0, 0, 0, 0, 0]], np.uint32)
    rollup, _, counters = ru.restate(ru.pairs_of_dense(dense), None, 31, len(labels), gof, "0.75", "0")
    assert rollup[:, 5].tolist() == [1, 2, ru.UNRESOLVED, 3, 0, 0]
    ranks = ["target", "genus", "family", "order", "class", "phylum", "superkingdom"]
    names = [labels,
             ["561", "570", "custom_x", "543", "9999"],
             ["543", "custom_x", "543", "9999"],
             ["91347", "custom_x", "9999"], ["1236", "custom_x", "9999"], ["1224", "custom_x", "9999"], ["2", "custom_x", "9999"]]
    taxids = [["562", "573", "UNKNOWN", "1001", "543", "83333", "UNKNOWN"],
              ["561", "570", "UNKNOWN", "543", "UNKNOWN"],
              ["543", "UNKNOWN", "543", "UNKNOWN"],
              ["91347", "UNKNOWN", "UNKNOWN"], ["1236", "UNKNOWN", "UNKNOWN"], ["1224", "UNKNOWN", "UNKNOWN"], ["2", "UNKNOWN", "UNKNOWN"]]
    assert "\n".join(got) + "\n" == ru.report(counters, len(labels), gof, ranks, names, taxids)
    assert "1,genus,561,561,1,2,33.3333" in got and "2,family,543,543,1,3,50" in got and "3,order,91347,91347,1,4,66.6667" in got
    assert got[-2:] == ["-,-,UNRESOLVED,UNKNOWN,1,1,16.6667", "-,-,UNKNOWN,UNKNOWN,1,1,16.6667"]
    # no taxonomy next to the database and no --lineage: an error, not a one-level report
    other = os.path.join(tmp, "elsewhere", "db")
    os.makedirs(other)
    r = _est("-F", csv, "--rank-report", out, "-D", other)
    assert r.returncode != 0 and "taxonomy" in r.stderr
