"""K-mer sketches on the CPU (csrc/mic_ksketch.h: the rule): mic_ksketch_add_host, mic_ksketch_estimate and mic_ksketch_format
against a restatement in Python (tests/ksketch_util.py) - hash, register, rank, merge, Ertl's estimator, the report's text - the
estimator's accuracy at four cardinalities, and the refusals of exe/cuCLARK --kmer-report, which need no device.
tools/ksketch_host_check.cpp drives the same host functions under AddressSanitizer and UBSan as a stand-alone program."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util as gu
import ksketch_util as ku

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
T = 7
KS = (20, 27, 31, 32)
# five standard errors of HyperLogLog at M = 16384 registers: 5 x 1.04 / sqrt(M)
BOUND = 5 * 1.04 / math.sqrt(ku.M)
_INV1, _INV2 = pow(0xff51afd7ed558ccd, -1, 1 << 64), pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)


def _unmix(h):
    """the inverse of fmix64 (x ^= x >> 33 is its own inverse; the multipliers are odd)"""
    h ^= h >> 33
    h = h * _INV2 & ku.U64
    h ^= h >> 33
    h = h * _INV1 & ku.U64
    h ^= h >> 33
    return h


def _rand_kmers(rng, n, k):
    if k == 32:
        return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)


def _crafted(rng, k):
    """(k-mers, what they are): all-A, pairs of a k-mer and its reverse complement, palindromes (even k), canonical k-mers whose hash
    has nothing behind the register index (w = 0, rank 51) where k leaves room for them"""
    full = (1 << (2 * k)) - 1
    km, what = [full, 0], ["all-A", "all-T (its reverse complement)"]
    for v in _rand_kmers(rng, 40, k):
        km += [int(v), ku.revcomp(int(v), k)]
        what += ["k-mer", "reverse complement"]
    if k % 2 == 0:
        for v in _rand_kmers(rng, 40, k // 2):
            p = (int(v) << k) | ku.revcomp(int(v), k // 2)
            assert ku.revcomp(p, k) == p
            km.append(p)
            what.append("palindrome")
    n_w0 = 0
    for idx in range(ku.M):
        c = _unmix(idx << ku.Q) ^ ku.SEED
        if c <= full and ku.canonical(c, k) == c:
            assert ku.index_rank(c) == (idx, ku.Q + 1)
            km.append(c)
            what.append("w = 0")
            n_w0 += 1
            if n_w0 == 8:
                break
    return np.array(km, np.uint64), what, n_w0


@pytest.mark.parametrize("k", KS)
def test_host_rule_equals_the_restatement(lib, k):
    from cuclark_amd import host
    rng = np.random.default_rng(1000 + k)
    crafted, what, n_w0 = _crafted(rng, k)
    # the chance of a k-mer with w = 0 in one register is 4^k / 2^64 per register: none at k = 20, a handful at k = 27, thousands above
    assert (n_w0 == 0) if k == 20 else (n_w0 >= 1 if k == 27 else n_w0 == 8), (k, n_w0)
    km = np.concatenate([crafted, _rand_kmers(rng, 6000, k)])
    lb = rng.integers(0, T + 2, km.size).astype(np.uint32)          # 0 and T + 1: no target
    lb[:crafted.size] = 1 + np.arange(crafted.size) // 2 % T        # (a k-mer and its reverse complement share a label)
    regs, hits = host.ksketch_add(km, lb, k, T)
    w_regs, w_hits = ku.sketch(km, lb, k, T)
    assert (hits == w_hits).all() and (regs == w_regs).all()
    assert int(hits.sum()) == int(np.count_nonzero((lb >= 1) & (lb <= T)))
    # the array form of the restatement against its digit-by-digit form
    s_regs, s_hits = ku.sketch_scalar(km[:crafted.size + 300], lb[:crafted.size + 300], k, T)
    a_regs, a_hits = ku.sketch(km[:crafted.size + 300], lb[:crafted.size + 300], k, T)
    assert (s_regs == a_regs).all() and (s_hits == a_hits).all()
    # a k-mer and its reverse complement: one register, one rank; a palindrome is its own canonical form; all-A is all-T
    for i, w in enumerate(what):
        v = int(crafted[i])
        if w == "reverse complement":
            assert ku.index_rank(ku.canonical(v, k)) == ku.index_rank(ku.canonical(int(crafted[i - 1]), k))
            one = host.ksketch_add(crafted[i - 1:i + 1], [1, 1], k, 1)
            assert int(one[1][0]) == 2 and int(np.count_nonzero(one[0])) == 1
        if w == "palindrome":
            assert ku.canonical(v, k) == v
            one = host.ksketch_add([v, v], [1, 1], k, 1)                     # counted once per occurrence
            assert int(one[1][0]) == 2 and int(np.count_nonzero(one[0])) == 1
        if w == "w = 0":
            one = host.ksketch_add([v], [1], k, 1)
            assert int(one[0].max()) == ku.Q + 1 == 51
    assert ku.canonical((1 << (2 * k)) - 1, k) == 0
    # merging: halves added into one sketch, and halves sketched apart and merged by max / sum, are the whole
    h = km.size // 2
    r2, h2 = host.ksketch_add(km[:h], lb[:h], k, T)
    host.ksketch_add(km[h:], lb[h:], k, T, r2, h2)
    assert (r2 == regs).all() and (h2 == hits).all()
    ra, ha = host.ksketch_add(km[h:], lb[h:], k, T)
    rb, hb = host.ksketch_add(km[:h], lb[:h], k, T)
    mr, mh = ku.merge((ra, ha), (rb, hb))
    assert (mr == regs).all() and (mh == hits).all()
    # what is no k-mer value is refused
    if k < 32:
        with pytest.raises(ValueError):
            host.ksketch_add([1 << (2 * k)], [1], k, 1)


def _distinct_kmers(seed, n, k=31):
    rng = np.random.default_rng(seed)
    c = np.unique(ku.canonical_np(_rand_kmers(rng, n + n // 8 + 64, k), k))
    assert c.size >= n
    return rng.permutation(c)[:n]


def test_estimator_equals_the_restatement(lib):
    from cuclark_amd import host
    zero = np.zeros(ku.M, np.uint8)
    assert host.ksketch_estimate(zero) == 0.0 and ku.estimate(zero) == 0.0 and ku.distinct(zero, 0) == 0
    for reg, rank in ((0, 1), (5, 1), (ku.M - 1, 51), (77, 30)):
        one = zero.copy()
        one[reg] = rank
        assert round(host.ksketch_estimate(one)) == 1 == ku.distinct(one, 1), (reg, rank)
    full = np.full(ku.M, 51, np.uint8)
    assert host.ksketch_estimate(full) == math.inf == ku.estimate(full)          # (saturated: no finite estimate)
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 777, 5000, 16384, 41000, 300000):
        regs, _ = host.ksketch_add(_distinct_kmers(100 + n, n), np.ones(n, np.uint32), 31, 1)
        got, want = host.ksketch_estimate(regs[0]), ku.estimate(regs[0])
        assert abs(round(got) - math.floor(want + 0.5)) <= 1, (n, got, want)
        assert abs(got - want) <= 1e-9 * max(1.0, want), (n, got, want)
    for _ in range(4):                    # registers no sketch would hold: every value 0 .. 51 (and one above) somewhere
        regs = rng.integers(0, 53, ku.M).astype(np.uint8)
        assert abs(round(host.ksketch_estimate(regs)) - math.floor(ku.estimate(regs) + 0.5)) <= 1


# seeds fixed here; test_accuracy checks the Python restatement alone first, then the library
@pytest.mark.parametrize("n,seed", [(100, 11), (100, 12), (2000, 21), (2000, 22), (40000, 31), (40000, 32), (160000, 41), (160000, 42)])
def test_accuracy(lib, n, seed):
    """|estimate - n| / n <= 5 x 1.04 / sqrt(16384) = 4.06 %: the small range, around 2.5 M = 40 960 and the raw range"""
    from cuclark_amd import host
    km = _distinct_kmers(seed, n)
    regs_py, hits_py = ku.sketch(km, np.ones(n, np.int64), 31, 1)
    e_py = ku.estimate(regs_py[0])
    print(f"n = {n}, seed {seed}: restatement {e_py:.2f} ({abs(e_py - n) / n:.4%})")
    assert abs(e_py - n) / n <= BOUND
    regs, hits = host.ksketch_add(km, np.ones(n, np.uint32), 31, 1)
    assert (regs == regs_py).all() and int(hits[0]) == n == int(hits_py[0])
    e = host.ksketch_estimate(regs[0])
    print(f"n = {n}, seed {seed}: library {e:.2f} ({abs(e - n) / n:.4%})")
    assert abs(e - n) / n <= BOUND
    # every k-mer a second time, as its reverse complement: more hits, the same registers
    rc = np.array([ku.revcomp(int(v), 31) for v in km[:200]], np.uint64)
    regs2, hits2 = host.ksketch_add(rc, np.ones(rc.size, np.uint32), 31, 1, regs.copy(), hits.copy())
    assert (regs2 == regs).all() and int(hits2[0]) == n + rc.size


def test_report_text(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(9)
    names = ["T_alpha", "T beta", "S6", "empty", "one", "dup", "x,y"]
    regs, hits = np.zeros((T, ku.M), np.uint8), np.zeros(T, np.uint64)
    for t, n in ((0, 30000), (1, 90), (2, 1234)):
        km = _distinct_kmers(200 + t, n)
        reps = rng.integers(1, 50, n)
        host.ksketch_add(np.repeat(km, reps), np.full(int(reps.sum()), t + 1, np.uint32), 31, T, regs, hits)
    host.ksketch_add([12345], [5], 31, T, regs, hits)                                        # one k-mer once: 1, 1, 1.00
    host.ksketch_add(np.full(4000, 999, np.uint64), np.full(4000, 6, np.uint32), 31, T, regs, hits)    # one k-mer 4 000 times: 4000.00
    reads = np.array([400, 4000, 17, 3, 1, 40, 0], np.uint64)
    text = host.ksketch_report(names, reads, regs, hits)
    assert text == ku.report(names, reads, regs, hits)
    lines = text.splitlines()
    assert lines[0] == "Name,Reads,Kmers,DistinctKmers,Duplication" and len(lines) == 1 + 5        # "empty" and "x,y" have no hits: no line
    assert lines[4] == "one,1,1,1,1.00" and lines[5] == "dup,40,4000,1,4000.00"
    for ln, n in zip(lines[1:4], (30000, 90, 1234)):
        d = int(ln.split(",")[3])
        assert abs(d - n) / n <= BOUND
    # Duplication: two decimals, rounded half up, from integers
    assert ku.ratio_text(1, 3) == "0.33" and ku.ratio_text(2, 3) == "0.67" and ku.ratio_text(1, 8) == "0.13" and ku.ratio_text(5, 1) == "5.00"
    assert ku.ratio_text(2 ** 63, 3) == "3074457345618258602.67"
    # a target with hits and registers that estimate below 0.5 still has one distinct k-mer
    z = np.zeros((1, ku.M), np.uint8)
    assert host.ksketch_report(["a"], [2], z, np.array([3], np.uint64)) == "Name,Reads,Kmers,DistinctKmers,Duplication\na,2,3,1,3.00\n"
    assert host.ksketch_report(["a"], [2], z, np.array([0], np.uint64)) == "Name,Reads,Kmers,DistinctKmers,Duplication\n"


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


# ---- the command line's refusals: before any device is touched ---------------------------------------------------------------------
def test_cli_refusals_need_no_device(lib, tmp_path):
    tmp = str(tmp_path)
    t = os.path.join(tmp, "targets.txt")
    open(t, "w").write("x y\n")
    reads = os.path.join(gu.GOLDEN, "reads_k31.fq")
    m1, m2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
    base = [EXE, "-k", "31", "-T", t, "-D", tmp]
    rep = os.path.join(tmp, "kr.csv")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, wherever this runs

    def refused(r, word):
        assert r.returncode == 1 and "--kmer-report" in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr

    refused(_run(base + ["-O", reads, "--kmer-report", rep, "--db-sharded"], env=env), "--db-sharded")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kmer-report", rep, "--parts", "2"], env=env), "--db-sharded")
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    refused(_run(base + ["-O", lo, "-R", lr, "--kmer-report", rep], env=env), "list-of-files")
    refused(_run(base + ["-O", reads, "--kmer-report", reads], env=env), "overwrite the input")
    refused(_run(base + ["-P", m1, m2, "--kmer-report", m2], env=env), "overwrite the input")
    link = os.path.join(tmp, "link.fq")
    os.symlink(reads, link)                                  # another name of the input
    refused(_run(base + ["-O", reads, "--kmer-report", link], env=env), "overwrite the input")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kmer-report", os.path.join(tmp, "o.csv")], env=env), "overwrite the result CSV")
    r = _run(base + ["-O", reads, "--kmer-report"], env=env)
    assert r.returncode == 1 and "Please specify the file of the k-mer report!" in r.stderr
    r = _run(base + ["-O", reads, "--kmer-report", rep, "--extended"], env=env)
    assert r.returncode == 1 and "--extended" in r.stderr
    assert open(reads, "rb").read()[:1] == b"@" and not os.path.exists(rep)
    r = _run([EXE, "--help"])
    assert "--kmer-report <file>" in r.stdout


# ---- the host functions under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ------------------------
def test_host_functions_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "ksketch_host_check")
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    # (the sanitizer runtimes are linked statically: the program runs in the environment as it is)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
              "-I", os.path.join(gu.ROOT, "include"), "-I", csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
              os.path.join(gu.ROOT, "tools", "ksketch_host_check.cpp"), os.path.join(csrc, "mic_host.cpp"), "-o", exe, "-lpthread"])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(3)
    cases, want = os.path.join(tmp, "cases.bin"), []
    with open(cases, "wb") as f:
        for k, n, nt in ((20, 0, 1), (20, 1, 1), (27, 3000, 3), (31, 20000, 2), (32, 5001, 5)):
            km = np.concatenate([_crafted(rng, k)[0], _rand_kmers(rng, n, k)])[:max(n, 0)] if n else np.zeros(0, np.uint64)
            km = np.concatenate([km, km[: n // 3]])                    # repeated k-mers
            lb = rng.integers(0, nt + 2, km.size).astype(np.uint32)
            reads = rng.integers(0, 1 << 40, nt).astype(np.uint64)
            f.write(struct.pack("<QiI", km.size, k, nt) + km.tobytes() + lb.tobytes() + reads.tobytes())
            want.append((k, nt, reads) + ku.sketch(km, lb, k, nt))
    out = os.path.join(tmp, "out.bin")
    r = _run([exe, cases, out])
    assert r.returncode == 0 and f"{len(want)} cases" in r.stdout, r.stdout + r.stderr
    blob, pos = open(out, "rb").read(), 0
    for k, nt, reads, regs, hits in want:
        got_hits = np.frombuffer(blob, np.uint64, nt, pos); pos += nt * 8
        got_regs = np.frombuffer(blob, np.uint8, nt * ku.M, pos).reshape(nt, ku.M); pos += nt * ku.M
        est = np.frombuffer(blob, np.float64, nt, pos); pos += nt * 8
        (ln,) = struct.unpack_from("<Q", blob, pos); pos += 8
        text = blob[pos:pos + ln].decode(); pos += ln
        assert (got_hits == hits).all() and (got_regs == regs).all(), k
        for t in range(nt):
            assert abs(est[t] - ku.estimate(regs[t])) <= 1e-9 * max(1.0, est[t])
        assert text == ku.report([f"target_{t + 1}" for t in range(nt)], reads, regs, hits)
    assert pos == len(blob)
