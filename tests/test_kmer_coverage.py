"""The table census on the CPU (csrc/mic_census.h: the rule): mic_db_census_host against the oracle's database - every k-mer of the
file looked up and counted by the label found - on the golden databases at sampling 1 and 3, on malformed buckets and at the edges;
mic_kcoverage_format against a restatement in Python (tests/kcoverage_util.py); the refusals of exe/cuCLARK --kmer-coverage, which
need no device.  tools/census_host_check.cpp drives the same host functions under AddressSanitizer and UBSan as a stand-alone program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util as gu
import kcoverage_util as kc
import ksketch_util as ku

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
T6 = 6
GOLDEN = ["full_k31_u32", "light_k20_u16", "light_k27_u32", "light_k31_u64", "light_k32_u64", "lightgap4_k27_u32"]
# the k-mers the oracle finds under their own labels (light_k31_u64: whatever it finds - every k-mer of the file at sampling 1)
FOUND = {("full_k31_u32", 1): 21016, ("light_k20_u16", 1): 21401, ("light_k27_u32", 1): 21156, ("light_k32_u64", 1): 20981, ("lightgap4_k27_u32", 1): 208,
         ("full_k31_u32", 3): 7005, ("light_k20_u16", 3): 7133, ("light_k27_u32", 3): 7052, ("light_k32_u64", 3): 6994, ("lightgap4_k27_u32", 3): 69}


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


@pytest.mark.parametrize("sampling", [1, 3])
@pytest.mark.parametrize("name", GOLDEN)
def test_host_census_equals_the_oracle_on_the_golden_databases(lib, name, sampling):
    from cuclark_amd import host
    db = gu.load_golden_db(name)
    sizes = gu.golden_sizes(db)
    counts, stats = host.db_census(sizes, db["ky"], db["lb"], db["k"], T6, sampling)
    want, found, n_elems = kc.oracle_counts(sizes, db["ky"], db["lb"], db["k"], T6, sampling)
    print(name, sampling, counts, stats)
    assert (counts == want).all(), (counts, want)
    assert int(stats[0]) == n_elems == found == int(counts.sum())
    assert [int(v) for v in stats[1:]] == [0] * 7
    if (name, sampling) in FOUND:
        assert found == FOUND[(name, sampling)]
    if sampling == 1:
        assert found == db["ky"].size
    if (name, sampling) == ("light_k27_u32", 3):
        assert [int(v) for v in counts] == [757, 1783, 966, 1730, 939, 877]
    if (name, sampling) == ("full_k31_u32", 1):
        assert [int(v) for v in counts] == [2129, 5344, 2936, 5169, 2878, 2560]


def malformed_db(k=20):
    """the generator of tests/test_gpu_parity.py::test_malformed_buckets_follow_reference_scan: unsorted buckets, duplicate keys"""
    rng = np.random.default_rng(9)
    htsize, T = 251, 9
    sizes = rng.integers(0, 30, htsize).astype(np.uint8)
    n = int(sizes.sum())
    keys = rng.integers(0, 60, n).astype(np.uint32)
    labels = rng.integers(0, T, n).astype(np.uint16)
    return sizes, keys, labels, k, T


@pytest.mark.parametrize("k", [20, 7])
def test_host_census_on_malformed_buckets(lib, k):
    """Expected: the distinct c of the file with canonical(c) == c that the oracle finds, by label.
    At k = 20 every c of this generator is canonical: c <= 59 * 251 + 250 < 4^7 begins with thirteen 'T' (code 0), so its reverse
    complement ends in thirteen 'A' (code 3) and is the larger value - stats[2] is 0 there by arithmetic, whatever the code does.  The
    same arrays read as 7-mers (4^7 = 16384 > 15059) do hold k-mers above their reverse complement: stats[2] > 0 is asserted on them."""
    from cuclark_amd import host
    sizes, keys, labels, k, T = malformed_db(k)
    counts, stats = host.db_census(sizes, keys, labels, k, T)
    want, found, _ = kc.oracle_counts(sizes, keys, labels, k, T)
    print(k, counts, stats)
    assert (counts == want).all(), (counts, want)
    assert int(stats[0]) == found == int(counts.sum()) > 100
    assert (int(stats[2]) > 0) if k == 7 else (int(stats[2]) == 0)
    assert int(stats[1]) == int(stats[3]) == int(stats[4]) == 0
    assert int(stats[0]) + int(stats[2]) < keys.size                 # entries the reference scan cannot reach are not enumerated
    py = kc.census(sizes, keys, labels, k, T)
    assert py[0] == [int(v) for v in counts] and py[1] == [int(v) for v in stats]


def _canonical_key(htsize, bucket, k, start=1):
    """a key whose k-mer key * htsize + bucket is canonical"""
    key = start
    while ku.canonical(key * htsize + bucket, k) != key * htsize + bucket:
        key += 1
    return key


def test_host_census_edges(lib):
    from cuclark_amd import host
    htsize, k, T = 1009, 12, 4                                       # (4^12 / 1009 < 2^16: every key width holds the keys)
    rng = np.random.default_rng(12)
    empty = np.zeros(htsize, np.uint8)
    counts, stats = host.db_census(empty, np.zeros(0, np.uint32), np.zeros(0, np.uint16), k, T)
    assert int(counts.sum()) == 0 and int(stats.sum()) == 0
    for bucket in (0, htsize - 1):
        sizes = empty.copy()
        sizes[bucket] = 1
        key = _canonical_key(htsize, bucket, k)
        for sampling, n in ((1, 1), (2, 0)):                        # the only non-empty bucket has rank 1: not kept at sampling 2
            counts, stats = host.db_census(sizes, np.array([key], np.uint32), np.array([2], np.uint16), k, T, sampling)
            assert [int(v) for v in counts] == [0, 0, n, 0] and [int(v) for v in stats] == [n, 0, 0, 0, 0, 0, 0, 0], (bucket, sampling)
    # a bucket of 255 ascending keys, a neighbour of 1; labels 0 .. 5 of which 4 and 5 are at and above n_targets
    sizes = empty.copy()
    sizes[500], sizes[501] = 255, 1
    keys = np.concatenate([np.sort(rng.choice((1 << 24) // htsize, 255, replace=False)), [_canonical_key(htsize, 501, k)]]).astype(np.uint64)
    labels = (np.arange(256) % 6).astype(np.uint16)
    counts, stats = host.db_census(sizes, keys, labels, k, T)
    canon = np.array([ku.canonical(int(kv) * htsize + b, k) == int(kv) * htsize + b for kv, b in zip(keys, [500] * 255 + [501])])
    assert 50 < int(canon.sum()) < 256
    assert [int(v) for v in counts] == [int(np.count_nonzero(canon & (labels == t))) for t in range(T)]
    assert int(stats[0]) == int(canon.sum()) and int(stats[2]) == 256 - int(canon.sum())
    assert int(stats[4]) == int(np.count_nonzero(canon & (labels >= T))) > 0 and int(counts.sum()) == int(stats[0]) - int(stats[4])
    assert kc.census(sizes, keys, labels, k, T)[0] == [int(v) for v in counts]
    # counts are added to fresh arrays per call; every key width gives the same numbers
    assert int(keys.max()) < 1 << 16
    for dt in (np.uint16, np.uint32):
        c2, s2 = host.db_census(sizes, keys.astype(dt), labels, k, T)
        assert (c2 == counts).all() and (s2 == stats).all()


def _regs_with_distinct(d):
    """registers whose estimate rounds to d: d k-mers sketched, one more or fewer until the estimator says d"""
    rng = np.random.default_rng(77)
    km = np.unique(rng.integers(0, 1 << 62, 4 * d + 64, dtype=np.uint64))
    for n in range(max(d - 8, 1), d + 9):
        regs, _ = ku.sketch(km[:n], np.ones(n, np.int64), 31, 1)
        if ku.distinct(regs[0], n) == d:
            return regs[0]
    raise AssertionError(d)


def test_report_text(lib):
    from cuclark_amd import host
    names = ["T_alpha", "clamped", "third", "two thirds", "empty", "x,y"]
    regs = np.zeros((6, ku.M), np.uint8)
    km = np.unique(np.random.default_rng(78).integers(0, 1 << 62, 3000, dtype=np.uint64))
    regs[0] = ku.sketch(km, np.ones(km.size, np.int64), 31, 1)[0][0]
    d0 = ku.distinct(regs[0], 45000)
    assert abs(d0 - km.size) < 0.05 * km.size
    regs[1], regs[2], regs[3] = _regs_with_distinct(105), _regs_with_distinct(1), _regs_with_distinct(2)
    hits = np.array([45000, 400, 9, 2, 0, 0], np.uint64)
    reads = np.array([500, 4, 1, 1, 0, 7], np.uint64)
    tk = np.array([20000, 100, 3, 3, 55, 0], np.uint64)
    text = host.kcoverage_report(names, reads, regs, hits, tk)
    assert text == kc.report(names, reads, regs, hits, tk)
    lines = text.splitlines()
    assert lines[0] == kc.HEADER and len(lines) == 1 + 4                     # "empty" and "x,y" have no hits: no line
    assert lines[1] == f"T_alpha,500,45000,{d0},{ku.ratio_text(45000, d0)},20000,{kc.ratio6(d0, 20000)}" and lines[1].endswith(",0.15" + lines[1][-4:])
    assert lines[2] == "clamped,4,400,105,3.81,100,1.000000"                 # DistinctKmers 105 of TargetKmers 100: clamped
    assert lines[3] == "third,1,9,1,9.00,3,0.333333" and lines[4] == "two thirds,1,2,2,1.00,3,0.666667"
    # the first five columns and the rows are the k-mer report's
    kr = host.ksketch_report(names, reads, regs, hits).splitlines()
    assert [",".join(ln.split(",")[:5]) for ln in lines] == kr
    assert kc.ratio6(1, 3) == "0.333333" and kc.ratio6(2, 3) == "0.666667" and kc.ratio6(7, 7) == "1.000000" and kc.ratio6(1, 2 ** 40) == "0.000000"
    # hits on a target with no k-mers in the table: no report
    with pytest.raises(ValueError):
        host.kcoverage_report(names, reads, regs, np.array([45000, 400, 9, 2, 0, 1], np.uint64), tk)
    assert host.kcoverage_report(["a"], [0], np.zeros((1, ku.M), np.uint8), [0], [0]) == kc.HEADER + "\n"


# ---- the command line's refusals: before any device is touched ---------------------------------------------------------------------
def test_cli_refusals_need_no_device(lib, tmp_path):
    tmp = str(tmp_path)
    t = os.path.join(tmp, "targets.txt")
    open(t, "w").write("x y\n")
    reads = os.path.join(gu.GOLDEN, "reads_k31.fq")
    m1, m2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
    base = [EXE, "-k", "31", "-T", t, "-D", tmp]
    rep = os.path.join(tmp, "kc.csv")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, wherever this runs

    def refused(r, word):
        assert r.returncode == 1 and "--kmer-coverage" in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr

    refused(_run(base + ["-O", reads, "--kmer-coverage", rep, "--db-sharded"], env=env), "--db-sharded")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kmer-coverage", rep, "--parts", "2"], env=env), "--db-sharded")
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    refused(_run(base + ["-O", lo, "-R", lr, "--kmer-coverage", rep], env=env), "list-of-files")
    refused(_run(base + ["-O", reads, "--kmer-coverage", reads], env=env), "overwrite the input")
    refused(_run(base + ["-P", m1, m2, "--kmer-coverage", m2], env=env), "overwrite the input")
    link = os.path.join(tmp, "link.fq")
    os.symlink(reads, link)                                  # another name of the input
    refused(_run(base + ["-O", reads, "--kmer-coverage", link], env=env), "overwrite the input")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--kmer-coverage", os.path.join(tmp, "o.csv")], env=env), "overwrite the result CSV")
    refused(_run(base + ["-O", reads, "--kmer-report", rep, "--kmer-coverage", rep], env=env), "another output")
    r = _run(base + ["-O", reads, "--kmer-coverage"], env=env)
    assert r.returncode == 1 and "Please specify the file of the k-mer coverage report!" in r.stderr
    r = _run(base + ["-O", reads, "--kmer-coverage", ""], env=env)
    assert r.returncode == 1 and "Please specify the file of the k-mer coverage report!" in r.stderr
    r = _run(base + ["-O", reads, "--kmer-coverage", rep, "--extended"], env=env)
    assert r.returncode == 1 and "--extended" in r.stderr
    assert open(reads, "rb").read()[:1] == b"@" and not os.path.exists(rep)
    r = _run([EXE, "--help"])
    assert "--kmer-coverage <file>" in r.stdout and "sampled" in r.stdout


# ---- the host functions under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ------------------------
def test_host_functions_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "census_host_check")
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    # (the sanitizer runtimes are linked statically: the program runs in the environment as it is)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
              "-I", os.path.join(gu.ROOT, "include"), "-I", csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
              os.path.join(gu.ROOT, "tools", "census_host_check.cpp"), os.path.join(csrc, "mic_host.cpp"), "-o", exe, "-lpthread"])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(4)
    cases, want = os.path.join(tmp, "cases.bin"), []
    with open(cases, "wb") as f:
        # random buckets of 0 .. 255 unsorted keys (the reach rule and the canonical test at work), every key width, and the empty one
        for htsize, k, kb, nt, sampling in ((97, 20, 2, 3, 1), (64, 27, 4, 5, 1), (61, 31, 8, 2, 3), (33, 32, 8, 70, 1), (50, 25, 4, 4, 1)):
            sizes = rng.integers(0, 256, htsize).astype(np.uint8)
            sizes[:2] = (255, 0)
            if htsize == 50:
                sizes[:] = 0
            n = int(sizes.sum(dtype=np.int64))
            top = min((1 << (8 * kb)) - 1, ((1 << (2 * k)) - 1) // htsize)          # c = key * htsize + bucket stays a k-mer value
            keys = rng.integers(0, top, n, dtype=np.uint64, endpoint=True).astype(gu.KEY_DTYPE[kb])
            srt = rng.random(htsize) < 0.5                            # half of the buckets well-formed: ascending keys
            off = 0
            for b in range(htsize):
                sz = int(sizes[b])
                if srt[b]:
                    keys[off:off + sz] = np.sort(keys[off:off + sz])
                off += sz
            labels = rng.integers(0, nt + 2, n).astype(np.uint16)
            f.write(struct.pack("<QQiiII", htsize, n, k, kb, nt, sampling) + sizes.tobytes() + keys.tobytes() + labels.tobytes())
            want.append((nt,) + kc.census(sizes, keys, labels, k, nt, sampling))
    out = os.path.join(tmp, "out.bin")
    r = _run([exe, cases, out])
    assert r.returncode == 0 and f"{len(want)} cases" in r.stdout and r.stderr == "", r.stdout + r.stderr
    blob, pos = open(out, "rb").read(), 0
    for nt, counts, stats in want:
        got_counts = np.frombuffer(blob, np.uint64, nt, pos); pos += nt * 8
        got_stats = np.frombuffer(blob, np.uint64, 8, pos); pos += 64
        (ln,) = struct.unpack_from("<Q", blob, pos); pos += 8
        text = blob[pos:pos + ln].decode(); pos += ln
        assert [int(v) for v in got_counts] == counts and [int(v) for v in got_stats] == stats
        names = [f"target_{t + 1}" for t in range(nt)]
        assert text == kc.report(names, counts, None, counts, counts, distinct_of=[1] * nt)
    assert pos == len(blob)
    assert sum(s[0] for _, _, s in want) > 3000 and sum(s[2] for _, _, s in want) > 1000 and want[-1][2] == [0] * 8
