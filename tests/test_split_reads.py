"""Read splitting on the CPU (csrc/mic_split.h: the rule): mic_split_host and exe/split_reads against a restatement of the rule in
Python - the text cut at its header lines, the integer rule applied to the result rows, the records concatenated - and the refusals
of exe/cuCLARK --classified-out / --unclassified-out, which need no device.  tools/split_host_check.cpp drives mic_split_host on the
same texts under AddressSanitizer and UBSan as a stand-alone program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util as gu

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
SPLIT = os.path.join(gu.ROOT, "exe", "split_reads")
FILTERS = [("0.5", "0"), ("0.75", "0.03"), ("1", "0"), ("0.5", "1")]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def record_starts(text):
    """Byte offsets of the header lines: FASTA lines that begin with '>', FASTQ lines 4r that begin with '@' (a line ends at its
    '\\n'; a '\\r' belongs to the line)."""
    fasta = text[:1] == b">"
    starts, pos, ln = [], 0, 0
    while pos < len(text):
        if (fasta and text[pos:pos + 1] == b">") or (not fasta and ln % 4 == 0 and text[pos:pos + 1] == b"@"):
            starts.append(pos)
        nl = text.find(b"\n", pos)
        pos = len(text) if nl < 0 else nl + 1
        ln += 1
    return starts


def is_classified(row, norm, k, n_targets, filt):
    cn, cd, gn, gd = (int(x) for x in filt)
    s, ib, best, _, second = (int(x) for x in row[:5])
    if ib == 0 or ib > n_targets:
        return False
    den = int(norm) - k + 1
    return best * cd >= cn * (best + second) and (gn == 0 or (den > 0 and s * gd >= gn * den))


def restate(text, rows, norms, k, n_targets, filt):
    """(classified bytes, unclassified bytes, classes) of a text whose records' result rows and Length columns are given"""
    cls = [is_classified(rows[r], norms[r], k, n_targets, filt) for r in range(len(rows))]
    return cut(text, cls) + (cls,)


def filt_tuple(c, g):
    from cuclark_amd import host
    f = host.abund_filter(c, g)
    return (f.conf_num, f.conf_den, f.gamma_num, f.gamma_den)


def gamma_of(text):
    """the printed "%g" Gamma field as an exact decimal; no number ("-nan") is below every positive threshold"""
    from fractions import Fraction
    try:
        return Fraction(text)
    except ValueError:
        return Fraction(-1)


def classes_from_csv(csv_text, c="0.5", g="0"):
    """The class of every row of a plain or --extended result CSV as exe/split_reads and exe/estimate_abundance decide it: the
    1st_assignment is not NA, score1 / (score1 + score2) >= c exactly, the printed gamma >= g as a decimal.  Also the fields."""
    from fractions import Fraction
    rows = [line.rsplit(",", 7) for line in csv_text.splitlines()[1:]]      # id, Length, Gamma, 1st, score1, 2nd, score2, confidence
    cls = [f[3] != "NA" and Fraction(int(f[4]), max(1, int(f[4]) + int(f[6]))) >= Fraction(c) and (Fraction(g) == 0 or gamma_of(f[2]) >= Fraction(g))
           for f in rows]
    return cls, rows


def cut(text, cls):
    """(classified bytes, unclassified bytes) of a text whose records' classes are given"""
    st = record_starts(text) + [len(text)]
    assert st[0] == 0 and len(st) - 1 == len(cls), (len(st) - 1, len(cls))
    out = [b"", b""]
    for r, c in enumerate(cls):
        rec = text[st[r]:st[r + 1]]
        out[0 if c else 1] += rec if rec.endswith(b"\n") else rec + b"\n"
    return out[0], out[1]


# ---- generated texts and crafted rows ------------------------------------------------------------------------------------------
def _texts(rng):
    def seq(n):
        return bytes(rng.choice(list(b"ACGTacgtN"), n).astype(np.uint8))

    def fq(n, eol=b"\n"):
        out = b""
        for i in range(n):
            s = seq(int(rng.integers(1, 200)))
            out += b"@r%d some text" % i + eol + s + eol + b"+r%d" % i + eol + bytes(rng.integers(33, 74, len(s)).astype(np.uint8)) + eol
        return out

    def fa(n, wrap=60):
        out = b""
        for i in range(n):
            s = seq(int(rng.integers(1, 400)))
            out += b">s%d\tdesc\n" % i + b"\n".join(s[j:j + wrap] for j in range(0, len(s), wrap)) + b"\n"
        return out
    return {
        "fastq": fq(61), "fastq_crlf": fq(40, b"\r\n"), "fasta_wrapped": fa(53), "fastq_unterminated": fq(17)[:-1],
        "fasta_unterminated": fa(9)[:-1], "fasta_trailing_blank_lines": fa(21) + b"\n\n\n", "single_fastq": fq(1), "single_fasta": fa(1)[:-1],
    }


def _crafted_rows(rng, n, norms, k, T):
    """rows that sit on and around every threshold of FILTERS, plus no hit, an index past the targets and ties"""
    rows = np.zeros((n, 8), np.uint32)
    for r in range(n):
        den = max(1, int(norms[r]) - k + 1)
        kind = r % 10
        best, second, s, ib = int(rng.integers(1, 300)), int(rng.integers(0, 300)), None, int(rng.integers(1, T + 1))
        if kind == 0:
            ib, best, second = 0, 0, 0                      # no hit
        elif kind == 1:
            ib = T + 1 + int(rng.integers(0, 3))            # an index past the targets
        elif kind == 2:
            second = best                                   # confidence exactly 0.5
        elif kind == 3:
            best, second = 3 * best, best                   # exactly 0.75
        elif kind == 4:
            best, second = 3 * best - 1, best               # just below 0.75
        elif kind == 5:
            second = 0                                      # confidence 1
        elif kind == 6:
            s = den                                         # gamma exactly 1
        elif kind == 7:
            s = max(0, den - 1)                             # just below 1
        elif kind == 8:
            s = (3 * den + 99) // 100                       # the smallest sum with gamma >= 0.03 (exactly 0.03 when 100 | den)
        if s is None:
            s = best + second
        rows[r, :6] = (s, ib, best, int(rng.integers(0, T + 1)), second, 2)
    return rows


def _cases():
    rng = np.random.default_rng(20)
    k, T = 31, 6
    out = []
    for name, text in _texts(rng).items():
        n = len(record_starts(text))
        norms = rng.integers(1, 400, n).astype(np.uint32)
        norms[::3] = 130                                    # 100 | Length - k + 1: gamma exactly 0.03 is reachable
        out.append((name, text, _crafted_rows(rng, n, norms, k, T), norms, k, T))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_split_host_equals_the_restatement(lib, name):
    from cuclark_amd import host
    _, text, rows, norms, k, T = [c for c in CASES if c[0] == name][0]
    ix = host.index_reads(text)
    starts = ix["name_s"] - 1
    assert [int(x) for x in starts] == record_starts(text)          # the library's records are the restatement's
    seen = set()
    for c, g in FILTERS:
        f = host.abund_filter(c, g)
        want_c, want_u, cls = restate(text, rows, norms, k, T, filt_tuple(c, g))
        seen.update(cls)
        n_target_rows = int(host.abundance_host(rows, norms, k, T, f)[2:].sum())
        for which in (1, 2, 3):
            out, (a, b, nc, nu) = host.split_host(text, starts, rows, norms, k, T, f, which)
            assert a + b == len(text) + (0 if text.endswith(b"\n") else 1), (name, c, g)
            assert (a, b) == (len(want_c), len(want_u)) and nc + nu == len(rows)
            assert nc == sum(cls) == n_target_rows, (name, c, g)
            got_c, got_u = out[:a].tobytes(), out[a:a + b].tobytes()
            assert got_c == (want_c if which & 1 else b"\xa5" * a), (name, c, g, which)
            assert got_u == (want_u if which & 2 else b"\xa5" * b), (name, c, g, which)
            assert (out[a + b:] == 0xA5).all()
    if len(rows) > 1:
        assert seen == {True, False}


def test_split_host_refuses_what_is_no_tiling(lib):
    from cuclark_amd import host
    text = b">a\nACGT\n>b\nAC\n"
    rows = np.zeros((2, 8), np.uint32)
    for starts in ([1, 8], [0, 0], [0, 14], [8, 0]):
        with pytest.raises(ValueError):
            host.split_host(text, np.array(starts, np.uint64), rows, None, 31, 6)
    with pytest.raises(ValueError):
        host.split_host(text, np.array([0, 8], np.uint64), rows, None, 31, 6, which=0)
    with pytest.raises(ValueError):       # a gamma threshold needs the lengths
        host.split_host(text, np.array([0, 8], np.uint64), rows, None, 31, 6, host.abund_filter("0.5", "0.1"))


# ---- exe/split_reads on the golden pairs -----------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


# n_below: assigned rows whose printed gamma is below 0.75, counted from the golden CSVs: 46 / 72 rows are below it, 1 / 3 of them are
# NA rows (the fourth NA row of the FASTA file prints "-nan", no number)
@pytest.mark.parametrize("kind,n_unclassified,n_below", [("fq", 1, 45), ("fa", 4, 69)])
def test_split_reads_on_the_golden_files(lib, tmp_path, kind, n_unclassified, n_below):
    tmp = str(tmp_path)
    reads = os.path.join(gu.GOLDEN, f"reads_k31.{kind}")
    csv = os.path.join(gu.GOLDEN, f"expected_k31_{kind}.csv")
    text = open(reads, "rb").read()
    csv_text = open(csv).read()

    def want(c, g):
        cls, _ = classes_from_csv(csv_text, c, g)
        return cut(text, cls) + (cls,)
    from fractions import Fraction
    rows = classes_from_csv(csv_text)[1]
    for extra, c, g in (([], "0.5", "0"), (["-g", "0.75"], "0.5", "0.75")):
        oc, ou = os.path.join(tmp, "c." + kind), os.path.join(tmp, "u." + kind)
        r = _run([SPLIT, "-F", csv, "-O", reads, "--classified-out", oc, "--unclassified-out", ou, *extra])
        assert r.returncode == 0, r.stderr
        want_c, want_u, cls = want(c, g)
        if not extra:
            assert cls.count(False) == n_unclassified
        else:
            assert sum(1 for f in rows if f[3] != "NA" and gamma_of(f[2]) < Fraction("0.75")) == n_below and want_c and want_u
        assert open(oc, "rb").read() == want_c and open(ou, "rb").read() == want_u
        assert f"{cls.count(True)} classified, {cls.count(False)} unclassified" in r.stderr
    # one class alone writes one file
    only = os.path.join(tmp, "only")
    r = _run([SPLIT, "-F", csv, "-O", reads, "--unclassified-out", only])
    assert r.returncode == 0 and open(only, "rb").read() == want("0.5", "0")[1]
    # a CSV whose third row is renamed
    lines = open(csv).read().splitlines(keepends=True)
    lines[3] = "renamed" + lines[3][lines[3].index(","):]
    bad = os.path.join(tmp, "bad.csv")
    open(bad, "w").write("".join(lines))
    r = _run([SPLIT, "-F", bad, "-O", reads, "--classified-out", os.path.join(tmp, "x")])
    assert r.returncode != 0 and "Row 3 " in r.stderr and "renamed" in r.stderr
    # fewer rows than records, and the usage errors
    open(bad, "w").write("".join(lines[:3]))
    r = _run([SPLIT, "-F", bad, "-O", reads, "--classified-out", os.path.join(tmp, "x")])
    assert r.returncode != 0 and "2 rows" in r.stderr
    assert _run([SPLIT, "-F", csv, "-O", reads]).returncode == 1
    assert _run([SPLIT, "-F", csv, "-O", reads, "--classified-out", only, "--unclassified-out", only]).returncode == 1
    assert _run([SPLIT, "-F", csv, "-O", reads, "--classified-out"]).returncode == 1


def test_split_reads_reads_extended_csvs(lib, tmp_path):
    tmp = str(tmp_path)
    reads = os.path.join(gu.GOLDEN, "reads_k31.fa")
    out = {}
    for name in ("expected_k31_fa.csv", "expected_k31_fa_ext.csv"):
        oc, ou = os.path.join(tmp, name + ".c"), os.path.join(tmp, name + ".u")
        r = _run([SPLIT, "-F", os.path.join(gu.GOLDEN, name), "-O", reads, "--classified-out", oc, "--unclassified-out", ou, "-c", "0.75", "-g", "0.03"])
        assert r.returncode == 0, r.stderr
        out[name] = (open(oc, "rb").read(), open(ou, "rb").read())
    assert out["expected_k31_fa.csv"] == out["expected_k31_fa_ext.csv"] and all(out["expected_k31_fa.csv"])


# ---- the command line's refusals: before any device is touched ---------------------------------------------------------------------
def test_cli_refusals_need_no_device(lib, tmp_path):
    tmp = str(tmp_path)
    t = os.path.join(tmp, "targets.txt")
    open(t, "w").write("x y\n")
    reads = os.path.join(gu.GOLDEN, "reads_k31.fq")
    m1, m2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
    base = [EXE, "-k", "31", "-T", t, "-D", tmp]
    c, u = os.path.join(tmp, "c.fq"), os.path.join(tmp, "u.fq")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, wherever this runs
    r = _run(base + ["-P", m1, m2, "-R", os.path.join(tmp, "o"), "--classified-out", c], env=env)
    assert r.returncode == 1 and "paired-end" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    r = _run(base + ["-O", lo, "-R", lr, "--unclassified-out", u], env=env)
    assert r.returncode == 1 and "list-of-files" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = _run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--classified-out", c, "--unclassified-out", c], env=env)
    assert r.returncode == 1 and "same file" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = _run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--unclassified-out", reads], env=env)
    assert r.returncode == 1 and "overwrite the input" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    link = os.path.join(tmp, "link.fq")
    os.symlink(reads, link)                                  # another name of the input
    r = _run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--classified-out", link], env=env)
    assert r.returncode == 1 and "overwrite the input" in r.stderr
    r = _run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--classified-out", os.path.join(tmp, "o.csv")], env=env)
    assert r.returncode == 1 and "overwrite the result CSV" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    for opt in ("--classified-out", "--unclassified-out"):
        r = _run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), opt], env=env)
        assert r.returncode == 1 and "Please specify the file of the" in r.stderr
    assert open(reads, "rb").read()[:1] == b"@" and not os.path.exists(c) and not os.path.exists(u)
    r = _run([EXE, "--help"])
    assert "--classified-out <file>" in r.stdout and "--unclassified-out <file>" in r.stdout


# ---- mic_split_host under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ----------------------------
def test_split_host_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "split_host_check")
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    # (the sanitizer runtimes are linked statically: the program runs in the environment as it is)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
              "-I", os.path.join(gu.ROOT, "include"), "-I", csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
              os.path.join(gu.ROOT, "tools", "split_host_check.cpp"), os.path.join(csrc, "mic_host.cpp"), "-o", exe, "-lpthread"])
    assert r.returncode == 0, r.stderr
    cases = os.path.join(tmp, "cases.bin")
    want = []
    with open(cases, "wb") as f:
        for name, text, rows, norms, k, T in CASES:
            starts = np.array(record_starts(text), np.uint64)
            for c, g in FILTERS:
                ft = filt_tuple(c, g)
                f.write(struct.pack("<QQiI4Q", len(text), len(rows), k, T, *ft))
                f.write(text + starts.tobytes() + np.ascontiguousarray(rows, np.uint32).tobytes() + np.ascontiguousarray(norms, np.uint32).tobytes())
                want.append((name, c, g, len(text)) + restate(text, rows, norms, k, T, ft)[:2])
    out = os.path.join(tmp, "out.bin")
    r = _run([exe, cases, out])
    assert r.returncode == 0, r.stdout + r.stderr
    blob = open(out, "rb").read()
    pos = 0
    for name, c, g, nb, want_c, want_u in want:
        for which in (1, 2, 3):
            a, b, nc, nu = struct.unpack_from("<4Q", blob, pos)
            buf = blob[pos + 32:pos + 32 + nb + 1]
            pos += 32 + nb + 1
            assert (a, b) == (len(want_c), len(want_u)), (name, c, g, which)
            assert buf[:a] == (want_c if which & 1 else b"\xa5" * a) and buf[a:a + b] == (want_u if which & 2 else b"\xa5" * b)
            assert buf[a + b:] == b"\xa5" * (nb + 1 - a - b)
    assert pos == len(blob)
