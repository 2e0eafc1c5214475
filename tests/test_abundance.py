"""Abundance profile on the CPU: exe/estimate_abundance (CLARK's third step) against a Python restatement of the counting rule
(csrc/mic_abund.h) and of the table (csrc/abundance_table.hpp), names and lineages from a synthetic taxonomy, and the library's
host rule (mic_abundance_host) and threshold parser through ctypes.  No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import golden_util as gu

EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")
CSVS = ["expected_k27_fa.csv", "expected_k31_fa.csv", "expected_k27_fq.csv", "expected_k31_fq.csv", "expected_k27_pairs.csv",
        "expected_k31_pairs.csv"]
RANKS = ["superkingdom", "phylum", "class", "order", "family", "genus"]


def _need_tool():
    assert os.path.exists(EST), "exe/estimate_abundance is not built (build() makes it)"


def _est(*args, **kw):
    return subprocess.run([EST, *args], capture_output=True, text=True, timeout=120, **kw)


# ---- the Python restatement ----------------------------------------------------------------------------------------------------
def _rows(path):
    """(label or None, score1, score2, gamma text) per read of a plain or extended result CSV."""
    out = []
    for i, line in enumerate(open(path).read().splitlines()):
        if i == 0 and line.startswith("Object_ID,"):
            continue
        f = line.split(",")[-7:]
        out.append((None if f[2] == "NA" else f[2], int(f[3]), int(f[5]), f[1]))
    return out


def _passes(s1, s2, gtext, c, g):
    if Fraction(s1, s1 + s2) < Fraction(c):
        return False
    if Fraction(g) == 0:
        return True
    try:
        return Fraction(gtext) >= Fraction(g)
    except ValueError:          # "-nan"
        return False


def _pct(count, den):
    return "0" if den == 0 else "%g" % (100.0 * count / den)


def _table(rows, c="0.5", g="0", a="0", describe=None):
    unassigned = filtered = 0
    per = {}
    for lab, s1, s2, gt in rows:
        if lab is None:
            unassigned += 1
        elif _passes(s1, s2, gt, c, g):
            per[lab] = per.get(lab, 0) + 1
        else:
            filtered += 1
    total = unassigned + filtered + sum(per.values())
    unknown = unassigned + filtered
    classified = total - unknown
    keep = [(lab, n) for lab, n in per.items() if Fraction(100 * n, classified) >= Fraction(a)]
    keep.sort(key=lambda x: (-x[1], x[0].encode()))
    out = ["Name,TaxID,Lineage,Count,Proportion_All(%),Proportion_Classified(%)"]
    for lab, n in keep:
        name, tid, lin = describe(lab) if describe else (lab, "UNKNOWN", "UNKNOWN")
        out.append(f"{name},{tid},{lin},{n},{_pct(n, total)},{_pct(n, classified)}")
    out.append(f"UNKNOWN,UNKNOWN,UNKNOWN,{unknown},{_pct(unknown, total)},-")
    return "\n".join(out) + "\n"


GRID = [("0.5", "0", "0"), ("0.75", "0", "0"), ("0.6", "0.5", "0"), ("0.5", "0.7", "12.5"), ("1", "0", "0"), ("0", "0", "20"),
        ("0.999", "0.03", "0"), ("0.5", "1", "0"), ("0.538462", "0.588235", "1.5")]


@pytest.mark.parametrize("csv", CSVS)
def test_estimate_abundance_equals_the_python_rule(csv):
    _need_tool()
    path = os.path.join(gu.GOLDEN, csv)
    rows = _rows(path)
    for c, g, a in GRID:
        r = _est("-F", path, "-c", c, "-g", g, "-a", a)
        assert r.returncode == 0, r.stderr
        assert r.stdout == _table(rows, c, g, a), (csv, c, g, a)
    r = _est("-F", path, "--highconfidence")
    assert r.returncode == 0 and r.stdout == _table(rows, "0.75", "0.03")


@pytest.mark.parametrize("k", [27, 31])
def test_plain_and_extended_csv_give_the_same_table_and_files_add_up(k):
    _need_tool()
    plain, ext = (os.path.join(gu.GOLDEN, f"expected_k{k}_fa{s}.csv") for s in ("", "_ext"))
    for c, g, a in GRID[:4]:
        a1, a2 = _est("-F", plain, "-c", c, "-g", g, "-a", a), _est("-F", ext, "-c", c, "-g", g, "-a", a)
        assert a1.returncode == 0 and a1.stdout == a2.stdout
    fq = os.path.join(gu.GOLDEN, f"expected_k{k}_fq.csv")
    r = _est("-F", plain, fq, "-c", "0.6")
    assert r.returncode == 0 and r.stdout == _table(_rows(plain) + _rows(fq), "0.6")


def test_exact_boundaries_and_the_default_counts_every_assigned_read(tmp_path):
    """Confidence exactly 0.75 passes -c 0.75, 2/3 does not; gamma exactly at the threshold passes; CLARK's defaults count every
    assigned read (its README's 20 / 70 / 10 example)."""
    _need_tool()
    p = os.path.join(str(tmp_path), "r.csv")
    lines = ["Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence"]
    lines += [f"a{i},100,0.3,A,3,B,1,0.75" for i in range(20)]            # confidence 3/4
    lines += [f"b{i},100,0.03,B,2,A,1,0.666667" for i in range(70)]       # confidence 2/3, gamma 0.03
    lines += [f"c{i},100,5e-05,C,1,NA,0,1" for i in range(10)]            # gamma 0.00005
    lines += ["n0,20,-0,NA,0,NA,0,0", "n1,30,-nan,NA,0,NA,0,0"]
    open(p, "w").write("\n".join(lines) + "\n")
    r = _est("-F", p)
    assert r.returncode == 0
    assert r.stdout.splitlines()[1:] == ["B,UNKNOWN,UNKNOWN,70,68.6275,70", "A,UNKNOWN,UNKNOWN,20,19.6078,20",
                                         "C,UNKNOWN,UNKNOWN,10,9.80392,10", "UNKNOWN,UNKNOWN,UNKNOWN,2,1.96078,-"]
    out = _est("-F", p, "-c", "0.75").stdout.splitlines()
    assert [l.split(",")[0] for l in out[1:]] == ["A", "C", "UNKNOWN"] and out[-1].startswith("UNKNOWN,UNKNOWN,UNKNOWN,72,")
    out = _est("-F", p, "-g", "0.03").stdout.splitlines()
    assert [l.split(",")[:4] for l in out[1:3]] == [["B", "UNKNOWN", "UNKNOWN", "70"], ["A", "UNKNOWN", "UNKNOWN", "20"]]
    out = _est("-F", p, "-g", "0.00005").stdout.splitlines()
    assert len(out) == 5
    out = _est("-F", p, "-g", "0.000051").stdout.splitlines()
    assert [l.split(",")[0] for l in out[1:]] == ["B", "A", "UNKNOWN"]
    # -a compares the classified share exactly: A has 20 %, so -a 20 keeps it and -a 20.000000001 drops it
    assert "A,UNKNOWN" in _est("-F", p, "-a", "20").stdout
    assert "A,UNKNOWN" not in _est("-F", p, "-a", "20.000000001").stdout
    for bad in (["-c", "1.5"], ["-c", "-0.1"], ["-g", "1e-3"], ["-a", "100.5"], ["-c", "0.1234567891"], ["-a", "x"], ["--bogus"], []):
        r = _est(*(["-F", p] if bad != [] else []), *bad)
        assert r.returncode != 0, bad


def test_all_reads_unassigned_prints_zero_fields(tmp_path):
    _need_tool()
    p = os.path.join(str(tmp_path), "r.csv")
    open(p, "w").write("Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\nx,10,-0,NA,0,NA,0,0\n")
    assert _est("-F", p).stdout == ("Name,TaxID,Lineage,Count,Proportion_All(%),Proportion_Classified(%)\n"
                                    "UNKNOWN,UNKNOWN,UNKNOWN,1,100,-\n")
    e = os.path.join(str(tmp_path), "e.csv")
    open(e, "w").write("Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\n")
    assert _est("-F", e).stdout.splitlines()[-1] == "UNKNOWN,UNKNOWN,UNKNOWN,0,0,-"


# ---- names and lineages from a taxonomy ---------------------------------------------------------------------------------------
NODES = [  # id, parent, rank, scientific name
    (1, 1, "no rank", "root"), (2, 1, "superkingdom", "Bacteria"), (1224, 2, "phylum", "Pseudomonadota"),
    (1236, 1224, "class", "Gammaproteobacteria"), (91347, 1236, "order", "Enterobacterales"), (543, 91347, "family", "Enterobacteriaceae"),
    (561, 543, "genus", "Escherichia"), (562, 561, "species", "Escherichia coli"),
    (3, 1, "domain", "Archaea"), (28890, 3, "phylum", "Euryarchaeota"), (2235, 28890, "order", "Halobacteriales"),     # no class
    (1963, 2235, "family", "Halobacteriaceae"), (2239, 1963, "genus", "Halobacterium"), (2242, 2239, "species", "Halobacterium salinarum"),
    (7000, 543, "genus", "Shigella"),
]


def _write_taxonomy(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for i, p, r, _ in NODES:
            f.write(f"{i}\t|\t{p}\t|\t{r}\t|\tXX\t|\t0\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for i, _, _, n in NODES:
            f.write(f"{i}\t|\t{n} (synonym)\t|\t\t|\tsynonym\t|\n")
            f.write(f"{i}\t|\t{n}\t|\t\t|\tscientific name\t|\n")


def _describe(label):
    by = {str(i): (p, r, n) for i, p, r, n in NODES}
    if label not in by:
        return label, "UNKNOWN", "UNKNOWN"
    p, r, n = by[label]
    own = RANKS.index(r) if r in RANKS else (0 if r == "domain" else 6)
    at = {}
    cur = str(p)
    while cur in by and cur != "1":
        pp, rr, nn = by[cur]
        lv = 0 if rr == "domain" else (RANKS.index(rr) if rr in RANKS else None)
        if lv is not None:
            at.setdefault(lv, nn)
        cur = str(pp)
    return n, label, ";".join(at.get(i, "UNKNOWN") for i in range(own)) or "UNKNOWN"


def test_names_lineages_fallback_and_order(tmp_path):
    _need_tool()
    tmp = str(tmp_path)
    _write_taxonomy(os.path.join(tmp, "DB", "taxonomy"))
    dbdir = os.path.join(tmp, "DB", "custom_0_canonical")
    os.makedirs(dbdir)
    labels = ["562"] * 5 + ["2242"] * 5 + ["7000"] * 3 + ["T_alpha"] * 3 + ["99999"] * 2 + ["561"]
    p = os.path.join(tmp, "r.csv")
    with open(p, "w") as f:
        f.write("Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\n")
        for i, lab in enumerate(labels):
            f.write(f"r{i},150,0.5,{lab},60,NA,0,1\n")
        f.write("u,150,0,NA,0,NA,0,0\n")
    r = _est("-F", p, "-D", dbdir)
    assert r.returncode == 0, r.stderr
    rows = _rows(p)
    assert r.stdout == _table(rows, describe=_describe)
    lines = r.stdout.splitlines()
    assert lines[1] == "Halobacterium salinarum,2242,Archaea;Euryarchaeota;UNKNOWN;Halobacteriales;Halobacteriaceae;Halobacterium,5,25,26.3158"
    assert lines[2] == "Escherichia coli,562,Bacteria;Pseudomonadota;Gammaproteobacteria;Enterobacterales;Enterobacteriaceae;Escherichia,5,25,26.3158"
    assert lines[3] == "Shigella,7000,Bacteria;Pseudomonadota;Gammaproteobacteria;Enterobacterales;Enterobacteriaceae,3,15,15.7895"
    assert lines[4].startswith("T_alpha,UNKNOWN,UNKNOWN,3,")
    assert lines[5].startswith("99999,UNKNOWN,UNKNOWN,2,")
    assert lines[6].startswith("Escherichia,561,Bacteria;Pseudomonadota;Gammaproteobacteria;Enterobacterales;Enterobacteriaceae,1,")
    # without the taxonomy files every label falls back to itself
    r = _est("-F", p)
    assert r.stdout == _table(rows)


# ---- the library's host rule and parser ---------------------------------------------------------------------------------------
def _rule(res, norm, k, T, c, g):
    out = np.zeros(T + 2, np.uint64)
    cn, cd = Fraction(c).numerator, Fraction(c).denominator
    for r, n in zip(res, norm):
        s, ib, b, _, s2 = (int(x) for x in r[:5])
        if ib == 0 or ib > T:
            out[0] += 1
            continue
        ok = Fraction(b, b + s2) >= Fraction(c) if b + s2 else cn == 0
        den = int(n) - k + 1
        ok = ok and (Fraction(g) == 0 or (den > 0 and Fraction(s, den) >= Fraction(g)))
        out[ib + 1 if ok else 1] += 1
    return out


def test_host_rule_through_ctypes_equals_the_python_rule(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(3)
    T, k, n = 300, 31, 20000
    res = np.zeros((n, 8), np.uint32)
    res[:, 2] = rng.integers(1, 200, n)
    res[:, 4] = np.minimum(res[:, 2], rng.integers(0, 200, n))
    res[:, 0] = res[:, 2] + res[:, 4] + rng.integers(0, 50, n)
    res[:, 1] = rng.integers(0, T + 1, n)
    res[rng.random(n) < 0.2, 1] = 0
    res[:, 2][res[:, 1] == 0] = 0
    norm = rng.integers(1, 400, n).astype(np.uint32)
    res[:5, 2], res[:5, 4], res[:5, 1] = 3, 1, 7                # confidence exactly 0.75
    res[5:10, 2], res[5:10, 4], res[5:10, 1] = 2, 1, 8          # 2/3
    for c, g in [("0.5", "0"), ("0.75", "0"), ("0.75", "0.03"), ("0.9", "0.5"), ("0", "1"), ("0.123456789", "0.000000001")]:
        got = host.abundance_host(res, norm, k, T, host.abund_filter(c, g))
        assert (got == _rule(res, norm, k, T, c, g)).all(), (c, g)
        assert int(got.sum()) == n
    got = host.abundance_host(res[:10], norm[:10], k, T, host.abund_filter("0.75", "0"))
    assert got[8] == 5 and got[9] == 0 and got[1] == 5
    with pytest.raises(ValueError):
        host.abundance_host(res, None, k, T, host.abund_filter("0.5", "0.1"))          # gamma without lengths
    assert (host.abundance_host(res, None, k, T) == _rule(res, norm, k, T, "0.5", "0")).all()


def test_threshold_parser(lib):
    from cuclark_amd import host
    good = {"0.5": (5, 10), "0.75": (75, 100), "1": (1, 1), "0": (0, 1), ".5": (5, 10), "1.": (1, 1), "0.000000001": (1, 10 ** 9),
            "1.000000000": (10 ** 9, 10 ** 9), "0.50": (50, 100)}
    for t, v in good.items():
        assert host.parse_threshold(t) == v, t
    assert host.parse_threshold("100", 100) == (100, 1) and host.parse_threshold("12.5", 100) == (125, 10)
    for t in ["", ".", "-0.5", "+0.5", "1e-3", "0.5 ", " 0.5", "1.5", "1.0000000001", "0.1234567891", "abc", "0,5", "1..0", "nan",
              "0x1", "99999999999999999999999"]:
        with pytest.raises(ValueError):
            host.parse_threshold(t)
    with pytest.raises(ValueError):
        host.parse_threshold("100.000000001", 100)
