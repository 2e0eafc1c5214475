"""--mask-low-complexity on the CPU: the host form of the low-complexity mask (mic_text_mask_low_complexity, csrc/mic_lowc.h) against
the rule written out below from its definition, and the command line's handling of the option.

The rule: a RUN is a maximal sequence of ACGTU bytes (either case) of a record's sequence; '\\n' is transparent, every other byte ends
it.  With the run's n nucleotides x[0..n) in the packer's code (A=3 C=2 G=1 T/U=0) and triplets t[j] = 16 x[j] + 4 x[j+1] + x[j+2],
the window of base i is [lo, hi) = [max(0, i-16), min(n, i+16)), l = hi - lo - 2 triplets t[lo .. lo+l) lie in it, c_v of them have
the value v, T = sum_v c_v (c_v - 1) / 2, and base i is masked iff l >= 2 and 10 T > level (l - 1).  A masked base becomes 'N';
nothing else changes.  The rule is applied once, to the original text."""
import os
import subprocess
import time

import numpy as np
import pytest

import golden_util as gu
from test_cli import EXE, _run
from test_ingest import _random_reads

K = 31
_CODE = np.full(256, 4, np.int64)
for _chars, _v in ((b"Aa", 3), (b"Cc", 2), (b"Gg", 1), (b"TtUu", 0)):
    for _c in _chars:
        _CODE[_c] = _v


def window_scores(codes):
    """(T, l) of every base of one run (codes: its 2-bit codes), from the definition: counts per triplet value inside each window."""
    n = codes.size
    i = np.arange(n)
    lo, hi = np.maximum(0, i - 16), np.minimum(n, i + 16)
    l = hi - lo - 2
    if n < 3:
        return np.zeros(n, np.int64), l
    t = 16 * codes[:-2] + 4 * codes[1:-1] + codes[2:]
    upto = np.zeros((64, n - 1), np.int64)               # upto[v, j] = how many of t[0 .. j) have the value v
    upto[t, np.arange(1, n - 1)] = 1
    upto = upto.cumsum(axis=1)
    ll = np.maximum(l, 0)
    c = upto[:, lo + ll] - upto[:, lo]
    return (c * (c - 1) // 2).sum(axis=0), l


def _mask_run(codes, level):
    T, l = window_scores(codes)
    return (l >= 2) & (10 * T > level * (l - 1))


def sequence_ranges(data, lpr=4):
    """[a, b) of every record's sequence: FASTQ ('@' first; lpr lines per record: 4, or 2 for text without '+' and quality lines) its
    second line; FASTA all its sequence lines, the line ends between them included."""
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    starts = np.concatenate(([0], np.cumsum([len(x) + 1 for x in lines]))).tolist()
    if data[:1] == b"@":
        return [(starts[r + 1], starts[r + 1] + len(lines[r + 1])) for r in range(0, len(lines) - 1, lpr)]
    assert data[:1] == b">"
    heads = [j for j, x in enumerate(lines) if x[:1] == b">"] + [len(lines)]
    return [(starts[h + 1], starts[h2 - 1] + len(lines[h2 - 1])) for h, h2 in zip(heads[:-1], heads[1:]) if h2 > h + 1]


def runs_of(seg):
    """(positions, codes, run bounds) of the bytes seg[] of one sequence: positions of its bytes that are no '\\n', their codes, and
    [i, j) into those for every run."""
    keep = np.flatnonzero(seg != 10)
    codes = _CODE[seg[keep]]
    d = np.diff(np.concatenate(([0], (codes < 4).astype(np.int8), [0])))
    return keep, codes, list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def reference_mask_lowc(data, level, lpr=4):
    """The rule, from its definition; does not call the library."""
    arr = np.frombuffer(bytes(data), np.uint8)
    out = arr.copy()
    if level:
        for a, b in sequence_ranges(bytes(data), lpr):
            keep, codes, runs = runs_of(arr[a:b])
            for i, j in runs:
                if j - i >= 4:
                    out[a + keep[i:j][_mask_run(codes[i:j], level)]] = ord("N")
    return out.tobytes()


UNITS = [b"A", b"T", b"C", b"AC", b"GA", b"ACG", b"TTC", b"ACGT", b"AACGT", b"AACGTC"]
PLANT_N = [14, 16, 20, 24, 31, 40, 64, 65]


def plant(rng, data, offsets=()):
    """Four-line FASTQ of _random_reads with low-complexity tracts planted: in every record of at least 50 sequence bytes whose index
    is not 3 mod 4, n bytes (one of PLANT_N, capped at the length) at position p (one of 0, 1, L - n, random, and those of `offsets`
    that fit) are overwritten with a repeated unit (one of UNITS)."""
    crlf = b"\r\n" in data
    lines = data.split(b"\n")
    for i, r in enumerate(range(0, len(lines) - 3, 4)):
        s = bytearray(lines[r + 1])
        L = len(s) - (1 if crlf else 0)
        if L < 50 or i % 4 == 3:
            continue
        n = min(int(rng.choice(PLANT_N)), L)
        ps = [0, 1, L - n, int(rng.integers(0, L - n + 1))] + [p for p in offsets if p + n <= L]
        p = min(ps[int(rng.integers(len(ps)))], L - n)
        u = UNITS[int(rng.integers(len(UNITS)))]
        s[p:p + n] = (u * (n // len(u) + 1))[:n]
        lines[r + 1] = bytes(s)
    return b"\n".join(lines)


def to_fasta(data, widths=(0,)):
    """The sequences of four-line FASTQ text as FASTA, record i wrapped at widths[i % len(widths)] (0: one line)."""
    crlf = b"\r\n" in data
    eol = b"\r\n" if crlf else b"\n"
    lines = data.split(b"\n")
    recs = []
    for i, r in enumerate(range(0, len(lines) - 3, 4)):
        name, s = lines[r][1:].rstrip(b"\r"), lines[r + 1].rstrip(b"\r")
        w = widths[i % len(widths)]
        body = eol.join(s[j:j + w] for j in range(0, len(s), w)) if w and len(s) > w else s
        recs.append(b">" + name + eol + body + eol)
    return b"".join(recs)


def _genomes():
    return [b"".join(l.strip() for l in open(fn, "rb") if not l.startswith(b">")) for fn, _ in gu.target_files_and_labels()]


def _fa(seq):
    return b">r\n" + seq + b"\n"


def _seq(text):
    return text.split(b"\n")[1]


def test_host_form_equals_the_rule(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(41)
    genomes = _genomes()
    levels = [1, 20, 21, 58, 149]
    n_rec = n_changed = 0
    for trial in range(10):
        level = levels[trial % 5]
        fq = plant(rng, _random_reads(rng, genomes, 330, fasta=False, crlf=trial in (3, 4)), offsets=(15, 16, 17, 63, 64, 65))
        data = fq if trial % 2 else to_fasta(fq, widths=(7, 60, 61, 64, 70, 0))     # lower case and U come with _random_reads
        if trial in (1, 2, 6):
            data = data[:-1]                      # no line end after the last record
        n_rec += 330
        want = reference_mask_lowc(data, level)
        assert len(want) == len(data) and (want != data or level == 149), trial
        n_changed += want != data
        assert host.mask_low_complexity(data, level) == want, (trial, level)
        buf = np.frombuffer(data, np.uint8).copy()                                      # in == out
        assert lib.mic_text_mask_low_complexity(buf.ctypes.data, buf.size, level, buf.ctypes.data) == 0
        assert buf.tobytes() == want, trial
        assert host.mask_low_complexity(data, 0) == data
    assert n_rec >= 3000 and n_changed >= 8
    # FASTA of _random_reads itself (its own wrapping, empty sequences, other bytes)
    for trial in range(3):
        data = _random_reads(rng, genomes, 200, fasta=True, crlf=trial == 1)
        assert host.mask_low_complexity(data, 1) == reference_mask_lowc(data, 1) != data


def test_fixed_vectors_and_run_lengths(lib):
    from cuclark_amd import host
    m = lambda s, level=20: _seq(host.mask_low_complexity(_fa(s), level))
    assert m(b"AAAAAA") == b"AAAAAA"              # l = 4, T = 6: 60 > 60 is false
    assert m(b"AAAAAAA") == b"NNNNNNN"            # l = 5, T = 10: 100 > 80
    assert _seq(reference_mask_lowc(_fa(b"AAAAAA"), 20)) == b"AAAAAA" and _seq(reference_mask_lowc(_fa(b"AAAAAAA"), 20)) == b"NNNNNNN"
    # level 149 masks a full window of one letter and nothing less: 10 * 435 > 149 * 29, but 10 * 406 < 149 * 28
    assert m(b"AAAAAAA", 149) == b"AAAAAAA" and m(b"A" * 31, 149) == b"A" * 31 and m(b"A" * 32, 149) == b"A" * 16 + b"N" + b"A" * 15
    assert m(b"uuuuuuu") == b"NNNNNNN" and m(b"AAAaaaa") == b"NNNNNNN" and m(b"TTTUUuu") == b"NNNNNNN"
    # the same as FASTQ, without a final line end, and with CRLF (the '\r' ends the run and is no base)
    assert host.mask_low_complexity(b"@r\nAAAAAAA\n+\nIIIIIII", 20) == b"@r\nNNNNNNN\n+\nIIIIIII"
    assert host.mask_low_complexity(b"@r\r\nAAAAAAA\r\n+\r\nIIIIIII\r\n", 20) == b"@r\r\nNNNNNNN\r\n+\r\nIIIIIII\r\n"
    # wrapped lines join; a '\r' at the line end does not
    assert host.mask_low_complexity(b">r\nAAA\nAAAA\n", 20) == b">r\nNNN\nNNNN\n"
    assert host.mask_low_complexity(b">r\r\nAAA\r\nAAAA\r\n", 20) == b">r\r\nAAA\r\nAAAA\r\n"
    # runs of exactly 2, 3, 4, 31, 32, 33 nucleotides, of one letter and of a dinucleotide, at the levels of the first test
    for n in (2, 3, 4, 31, 32, 33):
        for unit in (b"A", b"AC"):
            for level in (1, 20, 21, 58, 149):
                s = b"GN" + (unit * n)[:n] + b"N" + (unit * n)[:n]
                assert host.mask_low_complexity(_fa(s), level) == reference_mask_lowc(_fa(s), level), (n, unit, level)
    assert m(b"AAA", 1) == b"AAA" and m(b"AAAA", 1) == b"NNNN"                        # l = 1 is never masked; l = 2, T = 1: 10 > 1


def test_tract_positions_and_remainders(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(42)
    g = _genomes()[0]
    for n_run in (33, 64, 100):
        for unit in (b"A", b"AC", b"ACG"):
            for tl in (14, 20, 40):
                for off in (0, 1, 15, 16, 17, n_run - tl):          # the last one ends at n - 1
                    if off < 0 or off + tl > n_run:
                        continue
                    p = int(rng.integers(0, len(g) - n_run))
                    s = bytearray(g[p:p + n_run])
                    s[off:off + tl] = (unit * tl)[:tl]
                    for text in (_fa(bytes(s)), _fa(b"ACGTN" + bytes(s) + b"N" + bytes(s)), _fa(bytes(s[:off]) + b"N" + bytes(s[off:]))):   # a tract next to a real N
                        assert host.mask_low_complexity(text, 20) == reference_mask_lowc(text, 20), (n_run, unit, tl, off)
    # plants that leave unmasked remainders of exactly k-1 and k nucleotides in front of the masked stretch
    found = set()
    for start in (1000, 1500, 2000):
        for front in range(K - 6, K + 12):
            s = g[start:start + front] + b"A" * 30 + g[3000:3060]
            want = _seq(reference_mask_lowc(_fa(s), 20))
            assert _seq(host.mask_low_complexity(_fa(s), 20)) == want
            if b"N" not in s:
                found.add(want.index(b"N"))       # the nucleotides left in front of the masked stretch
    assert {K - 1, K} <= found


def test_the_threshold_is_exact(lib):
    """Windows with 10 T == level (l - 1) are not masked, windows with 10 T == level (l - 1) + 10 are; for level 20 and l = 30 these
    are T = 58 and T = 59.  The input must hold both kinds."""
    from cuclark_amd import host
    rng = np.random.default_rng(43)
    level = 20
    at, above = [], []          # (text, base offset in the sequence)
    for trial in range(4000):
        unit = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 7))).astype(np.uint8))
        s = bytearray((unit * 40)[:40])
        for _ in range(int(rng.integers(0, 9))):
            s[int(rng.integers(40))] = int(rng.choice(list(b"ACGT")))
        s = bytes(s)
        T, l = window_scores(_CODE[np.frombuffer(s, np.uint8)])
        for i in np.flatnonzero((l == 30) & (T == 58))[:1]:
            at.append((s, int(i)))
        for i in np.flatnonzero((l == 30) & (T == 59))[:1]:
            above.append((s, int(i)))
        for i in np.flatnonzero((l >= 2) & (l < 30) & (10 * T == level * (l - 1)))[:1]:
            at.append((s, int(i)))
        for i in np.flatnonzero((l >= 2) & (l < 30) & (10 * T == level * (l - 1) + 10))[:1]:
            above.append((s, int(i)))
        if len(at) >= 20 and len(above) >= 20 and trial > 200:
            break
    assert len(at) >= 20 and len(above) >= 20
    full = lambda lst: [x for x in lst if window_scores(_CODE[np.frombuffer(x[0], np.uint8)])[1][x[1]] == 30]
    assert full(at) and full(above)               # T = 58 and T = 59 at l = 30 among them
    for s, i in at:
        got = _seq(host.mask_low_complexity(_fa(s), level))
        assert got[i] == s[i] and got == _seq(reference_mask_lowc(_fa(s), level)), (s, i)
    for s, i in above:
        got = _seq(host.mask_low_complexity(_fa(s), level))
        assert got[i] == ord("N") and got == _seq(reference_mask_lowc(_fa(s), level)), (s, i)


def test_the_rule_is_not_idempotent_and_is_applied_once(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(44)
    g = _genomes()[1]
    seen = 0
    for trial in range(300):
        p = int(rng.integers(0, len(g) - 200))
        s = bytearray(g[p:p + 90])
        for at in (10, 40):
            u = UNITS[int(rng.integers(len(UNITS)))]
            n = int(rng.choice([12, 14, 16, 20]))
            s[at:at + n] = (u * n)[:n]
        text = _fa(bytes(s))
        once = reference_mask_lowc(text, 20)
        assert host.mask_low_complexity(text, 20) == once
        twice = reference_mask_lowc(once, 20)
        if twice != once:
            seen += 1
            assert host.mask_low_complexity(once, 20) == twice
    assert seen >= 1


def test_rejections(lib):
    from cuclark_amd import host
    for bad in (b"ACGT\n", b"\n>a\nACGT\n", b"+\n", b""):
        with pytest.raises(ValueError):
            host.mask_low_complexity(bad, 20)
    with pytest.raises(ValueError):
        host.mask_low_complexity(b">a\nAAAAAAAA\n", 150)
    out = np.full(32, 7, np.uint8)
    for text, level in ((b"AAAAAAAAAAAA\n", 20), (b">a\nAAAAAAAA\n", 150)):
        src = np.frombuffer(text, np.uint8)
        assert lib.mic_text_mask_low_complexity(src.ctypes.data, src.size, level, out.ctypes.data) != 0 and (out == 7).all()   # nothing written
    assert host.mask_low_complexity(b">a\nAAAAAAAA\n", 149) == b">a\nAAAAAAAA\n"


def test_a_contig_of_megabases_is_linear(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(45)
    n = 2_000_000
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    where = rng.integers(0, n - 100, 400)
    for p in where:
        u = UNITS[int(rng.integers(len(UNITS)))]
        tl = int(rng.choice(PLANT_N))
        s[p:p + tl] = np.frombuffer((u * tl)[:tl], np.uint8)
    s[rng.integers(0, n, 20)] = ord("N")
    body = s.tobytes()
    text = b">contig\n" + b"\n".join(body[j:j + 80] for j in range(0, n, 80)) + b"\n"
    t0 = time.time()
    got = host.mask_low_complexity(text, 20)
    dt = time.time() - t0
    assert dt < 5, dt
    flat = b"".join(got.split(b"\n")[1:])
    assert len(flat) == n and flat != body
    n_masked = 0
    for p in list(where[:60]) + [0, n - 300]:
        a, b = max(0, int(p) - 100), min(n, int(p) + 200)
        a2, b2 = max(0, a - 16), min(n, b + 16)                  # every window of [a, b) lies inside [a2, b2)
        want = _seq(reference_mask_lowc(_fa(body[a2:b2]), 20))[a - a2:a - a2 + (b - a)]
        assert flat[a:b] == want, p
        n_masked += want.count(b"N") - body[a:b].count(b"N")
    assert n_masked >= 100


def test_cli_bad_values_and_help(lib, tmp_path):
    r = _run([EXE, "--help"])
    assert r.returncode == 0 and "--mask-low-complexity <level>" in r.stdout and "[1,149]" in r.stdout
    t = str(tmp_path / "t.txt")
    fq = str(tmp_path / "r.fq")
    open(t, "w").write("")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    base = [EXE, "-T", t, "-D", str(tmp_path), "-O", fq, "-R", str(tmp_path / "out")]
    for v in ("abc", "2.5", "20x", "", "0", "150"):
        r = _run(base + ["--mask-low-complexity", v])
        assert r.returncode == 1 and ("The low-complexity level should be an integer in [1,149]: " + v) in r.stderr, (v, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "out.csv"))
    r = _run(base + ["--mask-low-complexity"])
    assert r.returncode == 1 and "Please specify the low-complexity level!" in r.stderr


def test_bit_plane_count_of_the_device_equals_the_sliding_histogram(tmp_path):
    """mic_lowc_T_planes and the window clipping a lane of lowc_kernel does (tools/lowc_planes_check.cpp restates the lane on the CPU)
    against mic_lowc_run, which the tests above hold to the definition: a later edit of the bit-plane count is caught without a device."""
    exe = str(tmp_path / "planes_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(gu.ROOT, "cuclark_amd", "csrc"),
                        os.path.join(gu.ROOT, "tools", "lowc_planes_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout[-2000:]


def test_the_mock_engine_links_with_the_stubs(lib, tmp_path):
    """tools/sanitize/mock_engine.cpp stands in for the device library under the command line (every slot "classified" into one
    "<name>,<length>" line per record): a plain build of the command line against it links - the new entry point has its stub - and
    the option runs through it and leaves names and lengths alone."""
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in ("classifier.cpp", "classifier_stream.cpp", "classifier_batch.cpp", "cli_main.cpp", "mic_host.cpp")]
    srcs.append(os.path.join(gu.ROOT, "tools", "sanitize", "mock_engine.cpp"))
    exe = str(tmp_path / "cuCLARK_mock")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", f"-I{os.path.join(gu.ROOT, 'include')}", f"-I{csrc}", "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-o", exe, *srcs, "-lz", "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # a database that only has to exist (the mock engine loads nothing)
    db = str(tmp_path / "DB")
    os.makedirs(db)
    genome = str(tmp_path / "g.fa")
    open(genome, "w").write(">g\nACGT\n")
    t = str(tmp_path / "targets.txt")
    open(t, "w").write(f"{genome} T0\n{genome} T1\n")
    stem = os.path.join(db, "db_central_k31_t2_s64_m0.tsk")
    open(stem + ".sz", "wb").write(bytes(64))
    open(stem + ".ky", "wb").write(b"")
    open(stem + ".lb", "wb").write(b"")
    fq = str(tmp_path / "r.fq")
    open(fq, "wb").write(b"@a\n" + b"A" * 60 + b"\n+\n" + b"I" * 60 + b"\n@b\nACGTACGTAGCTAGCTAGGATCGATCGATGCATGCATTAGC\n+\n" + b"I" * 40 + b"\n")
    outs = []
    for extra in ([], ["--mask-low-complexity", "20"]):
        out = str(tmp_path / ("o%d" % len(extra)))
        r = _run([exe, "-k", "31", "--htsize", "64", "-T", t, "-D", db, "-O", fq, "-R", out, "-n", "2"] + extra)
        assert r.returncode == 0, r.stderr
        outs.append(open(out + ".csv", "rb").read())
    assert outs[0] == outs[1] and b"a,60" in outs[0]
