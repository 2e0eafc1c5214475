"""Kraken formats on the CPU: mic_kraken_format (the rule: csrc/mic_kraken.h) and exe/estimate_abundance --kraken-report (the formatter:
csrc/kraken_report.hpp) against the Python restatement of tests/kraken_util.py, and the refusals of exe/cuCLARK --kraken-out /
--kraken-report, which need no device.  tools/kraken_host_check.cpp drives the same host code under AddressSanitizer and UBSan as a
stand-alone program.  Expected bytes always come from Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util as gu
import hitmap_util as hu
import kraken_util as kr
from test_abundance import _passes, _rows

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")
K = 31
TNAMES = ["7", "123456789012", "tB", "x3"]            # target names of 1 and 12 characters
T = len(TNAMES)
W = lambda l, n: (l << 16) | n


def _row(total, ib, best, i2=0, second=0):
    return [total, ib, best, i2, second, (1 if best else 0) + (1 if second else 0), 0, 0]


# (name, result row, norm, words): every case of the rule
READS = [
    (b"r", _row(4, 2, 3, 1, 1), K + 99, [W(2, 3), W(0, 96), W(1, 1)]),                  # confidence 0.75, gamma 0.04
    (b"gamma", _row(3, 1, 3), K + 99, [W(1, 3), W(0, 97)]),                              # gamma exactly 0.03
    (b"nohit", _row(0, 0, 0), 150, [W(0, 120)]),                                         # idxBest 0
    (b"above", _row(5, T + 1, 5), 150, [W(T + 1, 5), W(0, 115)]),                        # idxBest above the targets: U, and NA in the map
    (b"n" * 39, _row(9, 3, 9), 100, [W(3, 9)]),
    (b"m" * 40, _row(9, 4, 9), 100, [W(4, 9)]),
    (b"o" * 41, _row(9, 1, 9), 100, [W(1, 9)]),
    (b"empty", _row(0, 0, 0), 12, []),                                                   # shorter than k: U, 0, 0:0
    (b"sepfirst", _row(2, 2, 2), 90, [0, W(2, 2)]),
    (b"seplast", _row(2, 2, 2), 90, [W(2, 2), 0]),
    (b"sepdouble", _row(4, 2, 2, 3, 2), 90, [W(2, 2), 0, 0, W(3, 2)]),                   # a tie: the lower target is best
    (b"zeros", _row(1, 1, 1), 200, [W(0, 65535), W(1, 1), W(0, 7)]),                     # label-0 runs, the longest run
    (b"pair", _row(20, 2, 20), 300 - 1, [W(2, 10), W(0, 110), 0, W(0, 100), W(2, 10)]),  # paired norm: the length minus one
]


def _arrays(reads):
    names = [r[0] for r in reads]
    res = np.array([r[1] for r in reads], np.uint32).reshape(-1, 8)
    norm = np.array([r[2] for r in reads], np.uint32)
    off = np.cumsum([0] + [len(r[3]) for r in reads]).astype(np.uint32)
    words = np.array([w for r in reads for w in r[3]], np.uint32)
    return names, res, norm, off, words


FILTERS = [("0.5", "0"), ("0.75", "0"), ("0.76", "0"), ("0.5", "0.03"), ("0.5", "0.031"), ("0.75", "0.04"), ("1", "1"), ("0", "0")]


@pytest.fixture(scope="module")
def host():
    from cuclark_amd import host
    return host


def test_format_equals_the_restatement(host):
    names, res, norm, off, words = _arrays(READS)
    for c, g in FILTERS:
        got = host.kraken_format(names, res, norm, K, off, words, TNAMES, host.abund_filter(c, g))
        assert got == kr.format_text(names, res, norm, K, kr.filt(c, g), off, words, TNAMES), (c, g)
    line = lambda c, g, i: host.kraken_format(names, res, norm, K, off, words, TNAMES, host.abund_filter(c, g)).split(b"\n")[i]
    # what the restatement says about the cases, so that they are what their comments say
    assert line("0.75", "0", 0) == b"C\tr\t123456789012\t130\t123456789012:3 0:96 7:1"
    assert line("0.76", "0", 0) == b"U\tr\t0\t130\t123456789012:3 0:96 7:1"
    assert line("0.5", "0.03", 1)[:1] == b"C" and line("0.5", "0.031", 1)[:1] == b"U"
    assert line("0.5", "0", 2) == b"U\tnohit\t0\t150\t0:120"
    assert line("0.5", "0", 3) == b"U\tabove\t0\t150\tNA:5 0:115"
    assert line("0.5", "0", 4).split(b"\t")[1] == b"n" * 39 and line("0.5", "0", 5).split(b"\t")[1] == b"m" * 39 == line("0.5", "0", 5).split(b"\t")[1]
    assert line("0.5", "0", 6).split(b"\t")[1] == b"o" * 39
    assert line("0.5", "0", 7) == b"U\tempty\t0\t12\t0:0"
    assert line("0.5", "0", 8).endswith(b"\t|:| 123456789012:2") and line("0.5", "0", 9).endswith(b"\t123456789012:2 |:|")
    assert line("0.5", "0", 10) == b"C\tsepdouble\t123456789012\t90\t123456789012:2 |:| |:| tB:2"
    assert line("0.5", "0", 11).endswith(b"\t0:65535 7:1 0:7")
    assert line("0.5", "0", 12) == b"C\tpair\t123456789012\t299\t123456789012:10 0:110 |:| 0:100 123456789012:10"
    # a name of one byte, no reads, norm absent (no gamma filter: a gamma threshold then drops every read)
    assert host.kraken_format([], np.zeros((0, 8), np.uint32), None, K, [0], [], TNAMES) == b""
    got = host.kraken_format(names, res, None, K, off, words, TNAMES)
    assert got == kr.format_text(names, res, np.zeros(len(names), np.int64), K, kr.DEFAULT, off, words, TNAMES)


def test_format_two_call_sizing_and_null_arguments(host):
    import ctypes as C
    from cuclark_amd import _lib
    L = _lib.load()
    names, res, norm, off, words = _arrays(READS)
    want = kr.format_text(names, res, norm, K, kr.DEFAULT, off, words, TNAMES)
    rn = (C.c_char_p * len(names))(*names)
    tn = (C.c_char_p * T)(*[t.encode() for t in TNAMES])
    f = host.abund_filter()
    args = (rn, len(names), res.ctypes.data, norm.ctypes.data, K, T, C.byref(f), off.ctypes.data, words.ctypes.data, tn)
    assert L.mic_kraken_format(*args, None, 0) == len(want)
    buf = C.create_string_buffer(b"\x5a" * (len(want) + 8))
    assert L.mic_kraken_format(*args, buf, len(want)) == len(want) and buf.raw[:4] == b"\x5a" * 4        # one byte short: left alone
    assert L.mic_kraken_format(*args, buf, len(want) + 1) == len(want) and buf.raw[:len(want) + 1] == want + b"\0"
    bad = list(args)
    for i in (0, 2, 6, 7, 9):                      # names, results, filter, offsets, target names
        a = list(args)
        a[i] = None
        assert L.mic_kraken_format(*a, None, 0) == -1, i
    bad[6] = C.byref(_lib.MicAbundFilter(5, 7, 0, 1))
    assert L.mic_kraken_format(*bad, None, 0) == -1
    desc = np.array(off[::-1], np.uint32)
    assert L.mic_kraken_format(*args[:7], desc.ctypes.data, *args[8:], None, 0) == -1


# ---- exe/estimate_abundance --kraken-report against the restatement -----------------------------------------------------------------
CSVS = ["expected_k27_fa.csv", "expected_k31_fa.csv", "expected_k27_fq.csv", "expected_k31_fq.csv", "expected_k27_pairs.csv", "expected_k31_pairs.csv"]
# three levels: T_alpha and T_delta tie in expected_k31_fq.csv (15 reads each) inside one genus; T_gamma's family is its genus again (an
# inherited rank: the family line is left out); S6 is alone at every level (two inherited ranks: it hangs under the root)
LINEAGE = {"T_alpha": ("G1", "F1", "P1"), "T_delta": ("G1", "F1", "P1"), "T_beta": ("G2", "F1", "P1"), "T_gamma": ("G3", "G3", "P2"),
           "T_epsilon": ("G4", "F4", "P2"), "S6": ("S6", "S6", "S6")}
RANKS = ("genus", "family", "phylum")


def _est(*args):
    assert os.path.exists(EST), "exe/estimate_abundance is not built (build() makes it)"
    return subprocess.run([EST, *args], capture_output=True, text=True, timeout=120)


def _counts(rows, labels, c="0.5", g="0"):
    unassigned = filtered = 0
    per = dict.fromkeys(labels, 0)
    for lab, s1, s2, gt in rows:
        if lab is None:
            unassigned += 1
        elif _passes(s1, s2, gt, c, g):
            per[lab] += 1
        else:
            filtered += 1
    return unassigned, filtered, [per[l] for l in labels]


def _lineage_file(tmp, labels):
    p = os.path.join(tmp, "lineage.tsv")
    open(p, "w").write("#label\t" + "\t".join(RANKS) + "\n" + "".join(l + "\t" + "\t".join(LINEAGE[l]) + "\n" for l in labels))
    return p


def _want(rows, labels, c="0.5", g="0", flat=False, target_rank="species"):
    un, fi, per = _counts(rows, labels, c, g)
    targets = [(l, "UNKNOWN") for l in labels]
    levels = [] if flat else [[(LINEAGE[l][i], "UNKNOWN") for l in labels] for i in range(3)]
    return kr.report(un, fi, per, targets, levels, RANKS, target_rank)


@pytest.mark.parametrize("csv", CSVS)
def test_kraken_report_equals_the_restatement(tmp_path, csv):
    tmp = str(tmp_path)
    labels = list(dict.fromkeys(gu.target_names()))
    assert sorted(labels) == sorted(LINEAGE)
    lin = _lineage_file(tmp, labels)
    path = os.path.join(gu.GOLDEN, csv)
    rows = _rows(path)
    out = os.path.join(tmp, "k.txt")
    for c, g in [("0.5", "0"), ("0.75", "0.03"), ("1", "0.5")]:
        r = _est("-F", path, "-c", c, "-g", g, "--kraken-report", out, "--lineage", lin)
        assert r.returncode == 0, r.stderr
        want = _want(rows, labels, c, g)
        assert open(out).read() == want, (csv, c, g)
        # the flat form: no lineage, no taxonomy - the targets under the root, and that is no error
        r = _est("-F", path, "-c", c, "-g", g, "--kraken-report", out)
        assert r.returncode == 0, r.stderr
        seen = sorted(l for l in labels if _counts(rows, labels, c, g)[2][labels.index(l)])
        assert open(out).read() == _want(rows, seen, c, g, flat=True), (csv, c, g, "flat")
    text = _want(rows, labels)
    lines = text.splitlines()
    assert lines[0].split("\t")[3:] == ["U", "0", "unclassified"] or lines[0].split("\t")[3] == "R"
    assert any(ln.split("\t")[3:] == ["R", "1", "root"] for ln in lines[:2])
    names = [ln.split("\t")[5] for ln in lines]
    assert "    G3" in names and sum(n.strip() == "G3" for n in names) == 1            # the inherited family is left out: the genus under P2
    assert "  S6" in names and sum(n.strip() == "S6" for n in names) == 1              # alone at every level: under the root, once
    assert {ln.split("\t")[3] for ln in lines} >= {"R", "P", "F", "G", "S"}
    if csv == "expected_k31_fq.csv":                                                    # the clade tie: by name
        i = names.index("        T_alpha")
        assert names[i + 1] == "        T_delta" and lines[i].split("\t")[1] == lines[i + 1].split("\t")[1] == "15"
    # --kraken-target-rank: the targets' code
    r = _est("-F", path, "--kraken-report", out, "--lineage", lin, "--kraken-target-rank", "genus")
    assert r.returncode == 0 and open(out).read() == _want(rows, labels, target_rank="genus")
    r = _est("-F", path, "--kraken-report", out, "--lineage", lin, "--kraken-target-rank", "strain")
    assert r.returncode == 0 and open(out).read() == _want(rows, labels, target_rank="strain") and "\t-\t" in open(out).read()


def test_kraken_report_of_no_reads_and_percent_rounding(tmp_path):
    tmp = str(tmp_path)
    p, out = os.path.join(tmp, "r.csv"), os.path.join(tmp, "k.txt")
    open(p, "w").write("Object_ID,Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence\n")
    r = _est("-F", p, "--kraken-report", out)
    assert r.returncode == 0 and open(out).read() == "" == kr.report(0, 0, [], [])      # all = 0: nothing to print
    assert kr.pct(0, 0) == "  0.00" and kr.pct(1, 1) == "100.00" and kr.pct(1, 3) == " 33.33" and kr.pct(2, 3) == " 66.67" and kr.pct(1, 800) == "  0.13"
    # 1 of 800 is 0.125 %: half up; 7 reads of A, 1 of B, 792 without a hit
    open(p, "a").write("".join(f"a{i},100,1,A,9,NA,0,1\n" for i in range(7)) + "b,100,1,B,9,NA,0,1\n" + "".join(f"n{i},100,0,NA,0,NA,0,0\n" for i in range(792)))
    r = _est("-F", p, "--kraken-report", out)
    assert r.returncode == 0
    assert open(out).read() == kr.report(792, 0, [7, 1], [("A", "UNKNOWN"), ("B", "UNKNOWN")])
    assert open(out).read() == " 99.00\t792\t792\tU\t0\tunclassified\n  1.00\t8\t0\tR\t1\troot\n  0.88\t7\t7\tS\t0\t  A\n  0.13\t1\t1\tS\t0\t  B\n"
    # a label the lineage does not have is an error that names it
    lin = os.path.join(tmp, "lin.tsv")
    open(lin, "w").write("A\tg\n")
    r = _est("-F", p, "--kraken-report", out, "--lineage", lin)
    assert r.returncode == 1 and "B" in r.stderr


# ---- the command line's refusals: before any device is touched ---------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_cli_refusals_need_no_device(tmp_path):
    tmp = str(tmp_path)
    t = os.path.join(tmp, "targets.txt")
    open(t, "w").write("x y\n")
    reads = os.path.join(gu.GOLDEN, "reads_k31.fq")
    m1, m2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
    base = [EXE, "-k", "31", "-T", t, "-D", tmp]
    ko = os.path.join(tmp, "k.txt")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, wherever this runs

    def refused(r, word, opt="--kraken-out"):
        assert r.returncode == 1 and opt in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr

    refused(_run(base + ["-O", reads, "--kraken-out", ko, "--hit-maps", os.path.join(tmp, "hm.csv")], env=env), "--hit-maps")
    refused(_run(base + ["-O", reads, "--hit-maps", os.path.join(tmp, "hm.csv"), "--kraken-out", ko], env=env), "--hit-maps")
    refused(_run(base + ["-O", reads, "--kraken-out", ko, "--db-sharded"], env=env), "--db-sharded")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kraken-out", ko, "--parts", "2"], env=env), "--db-sharded")
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    refused(_run(base + ["-O", lo, "-R", lr, "--kraken-out", ko], env=env), "list-of-files")
    refused(_run(base + ["-O", reads, "--kraken-out", reads], env=env), "overwrite the input")
    refused(_run(base + ["-P", m1, m2, "--kraken-out", m2], env=env), "overwrite the input")
    link = os.path.join(tmp, "link.fq")
    os.symlink(reads, link)                                  # another name of the input
    refused(_run(base + ["-O", reads, "--kraken-out", link], env=env), "overwrite the input")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kraken-out", os.path.join(tmp, "o.csv")], env=env), "overwrite the result CSV")
    for opt in ("--abundance", "--kmer-report", "--density", "--rank-report", "--classified-out", "--unclassified-out", "--kraken-report"):
        refused(_run(base + ["-O", reads, opt, ko, "--kraken-out", ko], env=env), "another output")
    other = os.path.join(tmp, "ab.csv")
    open(other, "w").write("")
    os.link(other, os.path.join(tmp, "ab_again.csv"))         # the same inode under another name
    refused(_run(base + ["-O", reads, "--abundance", other, "--kraken-out", os.path.join(tmp, "ab_again.csv")], env=env), "another output")
    refused(_run(base + ["-O", reads, "--kraken-report", reads], env=env), "overwrite the input", "--kraken-report")
    refused(_run(base + ["-O", reads, "--abundance", other, "--kraken-report", os.path.join(tmp, "ab_again.csv")], env=env), "another output", "--kraken-report")
    r = _run(base + ["-O", reads, "--kraken-out"], env=env)
    assert r.returncode == 1 and "Please specify the file of the Kraken output!" in r.stderr
    r = _run(base + ["-O", reads, "--kraken-out", ko, "--extended"], env=env)
    assert r.returncode == 1 and "--extended" in r.stderr
    assert open(reads, "rb").read()[:1] == b"@" and not os.path.exists(ko)
    r = _run([EXE, "--help"])
    assert "--kraken-out <file>" in r.stdout and "--kraken-report <file>" in r.stdout and "--kraken-target-rank" in r.stdout


# ---- the host code under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ------------------------------
def test_host_functions_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "kraken_host_check")
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    # (the sanitizer runtimes are linked statically: the program runs in the environment as it is)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
              "-I", os.path.join(gu.ROOT, "include"), "-I", csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
              os.path.join(gu.ROOT, "tools", "kraken_host_check.cpp"), os.path.join(csrc, "mic_host.cpp"), "-o", exe, "-lpthread"])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(23)

    def random_read():
        per = rng.integers(0, 9, T) * (rng.random(T) < 0.5)
        res = kr.rows_from_counts([per])[0].tolist()
        if rng.random() < 0.1:
            res[1] = T + 3
        words = [0 if rng.random() < 0.2 else W(int(rng.integers(0, T + 2)), int(rng.integers(1, 70000)) & 0xFFFF or 1) for _ in range(int(rng.integers(0, 30)))]
        return (b"q" * int(rng.integers(1, 60)), res, int(rng.integers(0, 400)), words)

    cases = [(K, kr.filt(c, g), READS) for c, g in FILTERS] + [(K, kr.DEFAULT, [])]
    cases += [(int(rng.integers(12, 33)), kr.filt(c, g), [random_read() for _ in range(40)]) for c, g in FILTERS[:4]]
    # the reports: the six golden labels as targets of this program, the hand-written lineage and the flat form
    labels = list(LINEAGE)
    lin = _lineage_file(tmp, labels)
    reports = [("species", lin, [3, 1, 15, 15, 11, 13, 0, 4]), ("genus", lin, [0, 0, 1, 0, 0, 7, 2, 0]), ("species", "", [1, 2, 3, 0, 3, 0, 9, 1]),
               ("species", lin, [0] * 8), ("order", "", [5, 0, 0, 0, 0, 0, 0, 0])]
    blob_in = struct.pack("<I", T) + b"".join(struct.pack("<I", len(n)) + n.encode() for n in TNAMES) + struct.pack("<I", len(cases))
    for k, f, reads in cases:
        blob_in += struct.pack("<I4QI", k, *f, len(reads))
        for name, res, norm, words in reads:
            blob_in += struct.pack("<I", len(name)) + name + np.array(res, np.uint32).tobytes() + struct.pack("<II", norm, len(words)) + np.array(words, np.uint32).tobytes()
    path_in, path_out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    open(path_in, "wb").write(blob_in + struct.pack("<I", 0))
    r = _run([exe, path_in, path_out])
    assert r.returncode == 0 and f"{len(cases)} cases, 0 reports" in r.stdout, r.stdout + r.stderr
    blob, pos = open(path_out, "rb").read(), 0
    for k, f, reads in cases:
        names, res, norm, off, words = _arrays(reads)
        (tb,) = struct.unpack_from("<Q", blob, pos); pos += 8
        assert blob[pos:pos + tb] == kr.format_text(names, res.reshape(-1, 8), norm, k, f, off, words, TNAMES)
        pos += tb
    assert pos == len(blob)
    # the reports need the lineage's six labels as the program's targets: a second run
    blob_in = struct.pack("<I", len(labels)) + b"".join(struct.pack("<I", len(n)) + n.encode() for n in labels) + struct.pack("<II", 0, len(reports))
    for rank, path, counts in reports:
        blob_in += struct.pack("<I", len(rank)) + rank.encode() + struct.pack("<I", len(path)) + path.encode() + np.array(counts, np.uint64).tobytes()
    open(path_in, "wb").write(blob_in)
    r = _run([exe, path_in, path_out])
    assert r.returncode == 0 and f"0 cases, {len(reports)} reports" in r.stdout, r.stdout + r.stderr
    blob, pos = open(path_out, "rb").read(), 0
    for rank, path, counts in reports:
        levels = [[(LINEAGE[l][i], "UNKNOWN") for l in labels] for i in range(3)] if path else []
        (tb,) = struct.unpack_from("<Q", blob, pos); pos += 8
        assert blob[pos:pos + tb].decode() == kr.report(counts[0], counts[1], counts[2:], [(l, "UNKNOWN") for l in labels], levels, RANKS, rank)
        pos += tb
    assert pos == len(blob)
