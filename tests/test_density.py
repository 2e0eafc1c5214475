"""Score densities on the CPU: the rule of csrc/mic_density.h (host.density_host) against a restatement in exact fractions, the
survival property that ties the joint table to the abundance filter, the report text, exe/evaluate_density on the golden result CSVs,
the wrapper scripts and the command line's argument check.  (--density in list-of-files mode is refused after the database is loaded,
which needs a device: tests/test_density_gpu.py has that test.)"""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import golden_util as gu

EVAL = os.path.join(gu.ROOT, "exe", "evaluate_density")
EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
WORDS, CONF_BINS, GAMMA_BINS = 5153, 51, 101
T = 300


def _cell(c, g):
    return 2 + (c - 50) * GAMMA_BINS + g


def restate_bins(row, norm, k, n_targets):
    """(c, g) of a result row by the rule's definition in exact fractions, or None for an unassigned read"""
    total, ib, best, _, second = (int(x) for x in row[:5])
    if ib == 0 or ib > n_targets:
        return None
    c = 100 if best + second == 0 else max(50, min(100, math.floor(Fraction(100 * best, best + second))))
    den = int(norm) - k + 1
    g = 0 if den <= 0 else min(100, math.floor(Fraction(100 * total, den)))
    return c, g


def restate(rows, norm, k, n_targets):
    counts = np.zeros(WORDS, np.uint64)
    for r in range(rows.shape[0]):
        b = restate_bins(rows[r], norm[r], k, n_targets)
        counts[0] += 1
        counts[1 if b is None else _cell(*b)] += 1
    return counts


def edge_rows(k):
    """(rows u32[n, 8], norm u32[n]): the rows at the seams of the rule"""
    n0 = 100 + k - 1                                     # den = 100
    rows = [
        ([40, 0, 30, 2, 10], n0),                        # idxBest = 0
        ([40, T + 1, 30, 2, 10], n0),                    # idxBest past the targets
        ([40, T, 30, 2, 10], n0),                        # the last target
        ([40, 1, 20, 2, 20], n0),                        # a tie: bin 50
        ([40, 1, 40, 0, 0], n0),                         # second = 0: bin 100
        ([40, 1, 30, 2, 10], n0), ([40, 1, 29, 2, 10], n0), ([41, 1, 31, 2, 10], n0),      # 3/4 and one count either side
        ([100, 1, 90, 2, 10], n0), ([99, 1, 89, 2, 10], n0), ([101, 1, 91, 2, 10], n0),    # 9/10 and one count either side
        ([40, 1, 30, 2, 10], k - 1), ([40, 1, 30, 2, 10], 0),                              # norm < k: den <= 0
        ([40, 1, 30, 2, 10], k),                         # den = 1, sum > den: clamped to 100
        ([100, 1, 60, 2, 40], n0),                       # norm - k + 1 == sum: gamma bin 100
        ([99, 1, 60, 2, 39], n0), ([101, 1, 60, 2, 41], n0),
        ([0, 1, 0, 0, 0], n0),                           # best = second = 0 with idxBest != 0
        ([7, 1, 3, 2, 5], n0),                           # a malformed row (best < second): clamped into bin 50
        ([4000000000, 1, 4000000000, 2, 4000000000], 4294967295),                          # u32 extremes: 64-bit products
        ([4294967295, 1, 4294967295, 0, 0], 4294967295),
    ]
    res = np.zeros((len(rows), 8), np.uint32)
    for i, (r, _) in enumerate(rows):
        res[i, :5] = r
    return res, np.array([n for _, n in rows], np.uint32)


def random_rows(rng, n, k):
    res = np.zeros((n, 8), np.uint32)
    best = rng.integers(0, 200, n)
    second = np.minimum(best, rng.integers(0, 200, n) * rng.integers(0, 2, n))
    res[:, 2], res[:, 4] = best, second
    res[:, 0] = best + second + rng.integers(0, 50, n) * rng.integers(0, 2, n)
    res[:, 1] = rng.choice(np.array([0, 1, 2, 7, T, T + 1], np.uint32), n, p=[0.1, 0.3, 0.2, 0.2, 0.15, 0.05])
    res[:, 3] = np.where(second > 0, 3, 0)
    return res, rng.integers(0, 401, n).astype(np.uint32)


@pytest.fixture(scope="module")
def sample(lib):
    """20 000 random rows per k in {20, 27, 31} with the edge rows in front, and their counters by the restatement (computed once)"""
    rng = np.random.default_rng(2024)
    out = {}
    for k in (20, 27, 31):
        e_res, e_norm = edge_rows(k)
        r_res, r_norm = random_rows(rng, 20000, k)
        res, norm = np.concatenate([e_res, r_res]), np.concatenate([e_norm, r_norm])
        out[k] = (res, norm, restate(res, norm, k, T))
    return out


@pytest.mark.parametrize("k", [20, 27, 31])
def test_rule_equals_restatement(lib, sample, k):
    from cuclark_amd import host
    res, norm, want = sample[k]
    got = host.density_host(res, norm, k, T)
    assert got.shape == (WORDS,) and (got == want).all(), np.flatnonzero(got != want)
    assert int(got[0]) == res.shape[0] and int(got[1]) + int(got[2:].sum()) == int(got[0])
    assert int(got[1]) > 0 and int(np.count_nonzero(got[2:])) > 500
    # counts are ADDED; no norm: every assigned read in gamma bin 0
    twice = host.density_host(res, norm, k, T, counts=got.copy())
    assert (twice == 2 * want).all()
    flat = host.density_host(res, None, k, T)
    joint = want[2:].reshape(CONF_BINS, GAMMA_BINS)
    assert (flat[2:].reshape(CONF_BINS, GAMMA_BINS)[:, 0] == joint.sum(axis=1)).all() and int(flat[2:].sum()) == int(joint.sum())


def test_edge_rows_land_where_the_issue_says(lib):
    from cuclark_amd import host
    k = 31
    res, norm = edge_rows(k)
    where = []
    for i in range(res.shape[0]):
        c = host.density_host(res[i:i + 1], norm[i:i + 1], k, T)
        assert int(c[0]) == 1 and int(c.sum()) == 2
        j = int(np.flatnonzero(c[1:])[0]) + 1
        where.append(None if j == 1 else ((j - 2) // GAMMA_BINS + 50, (j - 2) % GAMMA_BINS))
    assert where == [None, None, (75, 40), (50, 40), (100, 40), (75, 40), (74, 40), (75, 41), (90, 100), (89, 99), (90, 100),
                     (75, 0), (75, 0), (75, 100), (60, 100), (60, 99), (59, 100), (100, 0), (50, 7), (50, 93), (100, 100)]


@pytest.mark.parametrize("k", [20, 31])
def test_cumulative_cells_are_the_filters_survivors(lib, sample, k):
    """Bin edges are multiples of 0.01 and the filters are >=: the cells at or above (c, g) hold exactly the reads the abundance
    filter {c, g} keeps."""
    from cuclark_amd import host
    res, norm, _ = sample[k]
    ok = res[:, 2] >= res[:, 4]           # (the malformed edge row, best < second, is clamped into bin 50: no filter keeps it)
    assert int(ok.sum()) == res.shape[0] - 1
    res, norm = res[ok], norm[ok]
    joint = host.density_host(res, norm, k, T)[2:].reshape(CONF_BINS, GAMMA_BINS)
    for c in ("0.5", "0.51", "0.75", "0.9", "1"):
        for g in ("0", "0.03", "0.5", "1"):
            ci, gi = int(Fraction(c) * 100), int(Fraction(g) * 100)
            kept = host.abundance_host(res, norm, k, T, host.abund_filter(c, g))[2:].sum()
            assert int(joint[ci - 50:, gi:].sum()) == int(kept), (c, g)


def _block(head, runs):
    """lines of a marginal block from hand-written runs (first bin, last bin, reads of each bin, cumulative of each bin)"""
    out = [head]
    for lo, hi, reads, cum in runs:
        out += [f"{b // 100}.{b % 100:02d},{reads},{cum}" for b in range(lo, hi + 1)]
    return out


def test_report_text(lib):
    from cuclark_amd import host
    counts = np.zeros(WORDS, np.uint64)
    counts[0], counts[1] = 10, 3
    counts[_cell(50, 0)], counts[_cell(75, 3)], counts[_cell(100, 0)], counts[_cell(100, 100)] = 1, 2, 1, 3
    head = ["Reads,10", "Unassigned,3", "Assigned,7"]
    conf = _block("Confidence,Reads,Cumulative", [(50, 50, 1, 7), (51, 74, 0, 6), (75, 75, 2, 6), (76, 99, 0, 4), (100, 100, 4, 4)])
    gamma = _block("Gamma,Reads,Cumulative", [(0, 0, 2, 7), (1, 2, 0, 5), (3, 3, 2, 5), (4, 99, 0, 3), (100, 100, 3, 3)])
    joint = ["Confidence,Gamma,Reads", "0.50,0.00,1", "0.75,0.03,2", "1.00,0.00,1", "1.00,1.00,3"]
    assert len(conf) == 52 and len(gamma) == 102
    assert host.density_report(counts) == "\n".join(head + conf + gamma + joint) + "\n"
    assert host.density_report(counts, 1) == "\n".join(head + conf) + "\n"
    assert host.density_report(counts, 2) == "\n".join(head + gamma) + "\n"
    with pytest.raises(ValueError):
        host.density_report(counts[:-1])


def _marginals(text):
    """{block head: [(bin text, reads, cumulative)]} of a report"""
    blocks, cur = {}, None
    for line in text.splitlines():
        f = line.split(",")
        if not f[0][0].isdigit():
            cur = blocks.setdefault(line, []) if line.endswith(",Cumulative") else None
        elif cur is not None:
            cur.append((f[0], int(f[1]), int(f[2])))
    return blocks


def test_report_cumulative_columns(lib, sample):
    from cuclark_amd import host
    res, norm, want = sample[27]
    text = host.density_report(want)
    assigned = int(want[2:].sum())
    assert text.startswith(f"Reads,{int(want[0])}\nUnassigned,{int(want[1])}\nAssigned,{assigned}\n")
    b = _marginals(text)
    for head, n, first in (("Confidence,Reads,Cumulative", 51, "0.50"), ("Gamma,Reads,Cumulative", 101, "0.00")):
        rows = b[head]
        assert len(rows) == n and rows[0][0] == first and rows[-1][0] == "1.00"
        cum = [r[2] for r in rows]
        assert cum[0] == assigned and all(x >= y for x, y in zip(cum, cum[1:]))
        assert all(cum[i] - cum[i + 1] == rows[i][1] for i in range(n - 1)) and cum[-1] == rows[-1][1]
    joint = [l for l in text.split("Confidence,Gamma,Reads\n")[1].splitlines()]
    assert len(joint) == int(np.count_nonzero(want[2:])) and joint == sorted(joint)


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def _restate_csv(path):
    """the counters of a result CSV from its own columns: confidence from score1 / score2, gamma from the printed text as a decimal"""
    counts = np.zeros(WORDS, np.uint64)
    for line in open(path).read().splitlines()[1:]:
        f = line.rsplit(",", 7)[1:]
        counts[0] += 1
        if f[2] == "NA":
            counts[1] += 1
            continue
        s1, s2 = int(f[3]), int(f[5])
        c = 100 if s1 + s2 == 0 else max(50, min(100, math.floor(Fraction(100 * s1, s1 + s2))))
        try:
            v = Fraction(f[1])
            g = 0 if f[1].startswith("-") else max(0, min(100, math.floor(100 * v)))
        except ValueError:
            g = 0
        counts[_cell(c, g)] += 1
    return counts


def test_tool_on_golden_csvs(lib, tmp_path):
    from cuclark_amd import host
    fq = os.path.join(gu.GOLDEN, "expected_k31_fq.csv")
    want = _restate_csv(fq)
    assert int(want[0]) == 80 and 0 < int(want[1]) < 80 and int(np.count_nonzero(want[2:])) > 5
    r = _run([EVAL, "-F", fq])
    assert r.returncode == 0 and r.stdout == host.density_report(want), r.stderr
    # plain and --extended CSVs of the same run read alike
    fa, fa_ext = os.path.join(gu.GOLDEN, "expected_k27_fa.csv"), os.path.join(gu.GOLDEN, "expected_k27_fa_ext.csv")
    ra, rb = _run([EVAL, "-F", fa]), _run([EVAL, "-F", fa_ext])
    assert ra.returncode == 0 and rb.returncode == 0 and ra.stdout == rb.stdout == host.density_report(_restate_csv(fa))
    # several files are summed
    both = _run([EVAL, "-F", fq, fa])
    assert both.returncode == 0 and both.stdout == host.density_report(want + _restate_csv(fa))
    # one marginal
    for flag, which in (("--confidence", 1), ("--gamma", 2)):
        r = _run([EVAL, "-F", fq, flag])
        assert r.returncode == 0 and r.stdout == host.density_report(want, which)
    # CLARK's script names
    for sh, which in (("evaluate_density_confidence.sh", 1), ("evaluate_density_gamma.sh", 2)):
        r = _run([os.path.join(gu.ROOT, sh), "-F", fq], cwd=str(tmp_path))
        assert r.returncode == 0 and r.stdout == host.density_report(want, which), r.stderr
        assert _run([os.path.join(gu.ROOT, sh)]).stdout.startswith("Usage:")


def test_tool_gamma_text_forms(lib, tmp_path):
    """the printed forms of "%g": an exponent, a value above 1, -0, -nan and inf, a value on a bin edge"""
    from cuclark_amd import host
    p = os.path.join(str(tmp_path), "r.csv")
    rows = [("5e-05", 0), ("0.0299999", 2), ("0.03", 3), ("1.21053", 100), ("1", 100), ("-0", 0), ("-nan", 0), ("inf", 0), ("0.999999", 99),
            ("1e-02", 1), ("0", 0)]
    with open(p, "w") as f:
        f.write("Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\n")
        for i, (g, _) in enumerate(rows):
            f.write(f"r,{i},with,commas,150,{g},T_a,3,T_b,1,0.75\n")
        f.write("u,150,0,NA,0,NA,0,0\n")
    want = np.zeros(WORDS, np.uint64)
    want[0], want[1] = len(rows) + 1, 1
    for _, g in rows:
        want[_cell(75, g)] += 1
    r = _run([EVAL, "-F", p])
    assert r.returncode == 0 and r.stdout == host.density_report(want), r.stderr


def test_tool_refuses_other_files(tmp_path):
    p = os.path.join(str(tmp_path), "short.csv")
    open(p, "w").write("Object_ID,Length,Gamma\nr0,150,0.5\n")
    r = _run([EVAL, "-F", p])
    assert r.returncode == 1 and "line 2" in r.stderr and r.stdout == ""
    assert _run([EVAL, "-F", os.path.join(str(tmp_path), "missing.csv")]).returncode == 1
    assert _run([EVAL]).returncode == 1
    r = _run([EVAL, "-F", p, "--confidence", "--gamma"])
    assert r.returncode == 1 and "exclude" in r.stderr


def test_cli_density_needs_a_value(lib):
    r = _run([EXE, "-k", "31", "-k", "31", "--density"])
    assert r.returncode == 1 and "density report" in r.stderr
    assert "--density <file>" in _run([EXE, "--help"]).stdout
