"""Hit maps on the CPU (csrc/mic_hitmap.h: the rule): mic_hitmap_runs_host and mic_hitmap_format against a restatement in Python
(tests/hitmap_util.py: itertools.groupby over the labels of each part, the words, the text), and the refusals of exe/cuCLARK
--hit-maps, which need no device.  tools/hitmap_host_check.cpp drives the same host functions under AddressSanitizer and UBSan as a
stand-alone program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util as gu
import hitmap_util as hu

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
T = 6
TNAMES = ["A", "target_two", "S6", "x" * 60, "Escherichia_coli_K12", "t6"]        # a name of one byte and one of 60

# label sequences per part (label T + 1 and above: no target), by what they are
LABEL_CASES = {
    "length 1": [[3]],
    "one label throughout": [[2] * 300],
    "alternating labels": [[1, 2] * 70],
    "label 0 only": [[0] * 65],
    "a label above n_targets": [[1, 1, T + 1, T + 1, 1, 9999, 0, T, T]],
    "equal labels on both sides of a cut": [[4] * 40, [4] * 25],
    "zero parts": [],
    "three parts, the middle one of one position": [[0, 0, 5], [5], [5, 0]],
    "a part of 65 535 positions": [[6] * 65535],
    "runs of 1, 9, 10 and 100": [[1] + [2] * 9 + [3] * 10 + [0] * 100],
}


def _runs(host, parts):
    flat = [x for p in parts for x in p]
    return host.hitmap_runs(np.array(flat, np.uint32), np.array([len(p) for p in parts], np.uint32), T)


@pytest.mark.parametrize("what", list(LABEL_CASES))
def test_runs_equal_the_restatement(lib, what):
    from cuclark_amd import host
    parts = LABEL_CASES[what]
    got = _runs(host, parts)
    want = np.array(hu.rle_words(parts, T), np.uint32)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist(), what
    assert sum(int(w) & 0xFFFF for w in got) == sum(len(p) for p in parts)
    if what == "equal labels on both sides of a cut":
        assert got.tolist() == [(4 << 16) | 40, 0, (4 << 16) | 25]                 # a separator, no merge
    if what == "zero parts":
        assert got.size == 0
    if what == "a label above n_targets":
        assert got.tolist() == [(1 << 16) | 2, 2, (1 << 16) | 1, 2, (T << 16) | 2]
    if what == "a part of 65 535 positions":
        assert got.tolist() == [(6 << 16) | 65535]


def test_runs_on_random_labels(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(41)
    for _ in range(60):
        parts = [rng.integers(0, T + 3, int(rng.integers(0, 200))).repeat(int(rng.integers(1, 6))).tolist() for _ in range(int(rng.integers(0, 5)))]
        assert _runs(host, parts).tolist() == hu.rle_words(parts, T)
    with pytest.raises(ValueError):
        host.hitmap_runs(np.zeros(65536, np.uint32), [65536], T)                   # a part the packer never writes


def test_format_equals_the_restatement(lib):
    from cuclark_amd import host
    w = lambda l, n: (l << 16) | n
    reads = [
        (b"r0", []),                                                             # an empty map
        (b"n" * 39, [w(1, 1)]),                                                  # a 39-byte name
        (b"m" * 40, [w(2, 9)]),                                                  # 40 bytes: printed as 39
        (b"long" * 30, [w(3, 10), 0, w(0, 65535)]),
        (b"r4", [w(4, 65535), w(0, 1), w(1, 9), w(5, 10), 0, w(6, 100), 0, w(0, 7)]),
        (b"r5", [0]),                                                            # (never written by the kernels: a lone separator)
    ]
    names = [n for n, _ in reads]
    off = np.cumsum([0] + [len(ws) for _, ws in reads]).astype(np.uint32)
    words = np.array([x for _, ws in reads for x in ws], np.uint32)
    got = host.hitmap_format(names, off, words, TNAMES)
    assert got == hu.format_text(names, off, words, TNAMES)
    lines = got.split(b"\n")
    assert lines[0] == b"r0," and lines[1] == b"n" * 39 + b",A:1" and lines[2] == b"m" * 39 + b",target_two:9"
    assert lines[3] == (b"long" * 30)[:39] + b",S6:10 | 0:65535"
    assert lines[4] == b"r4," + b"x" * 60 + b":65535 0:1 A:9 Escherichia_coli_K12:10 | t6:100 | 0:7" and lines[5] == b"r5,|" and lines[6] == b""
    assert host.hitmap_format([], [0], [], TNAMES) == b""
    with pytest.raises(ValueError):
        host.hitmap_format([b"a"], [2, 1], [1, 2], TNAMES)                         # descending offsets


def test_restatement_cuts_long_runs_like_the_packer(lib):
    """parts_of against host.pack_reads: the part lengths the packer writes for runs around MIC_MAX_PART, with an N between"""
    from cuclark_amd import host
    rng = np.random.default_rng(5)
    k = 31
    for n in (65528, 65529, 70000, 131100):
        seq = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)) + b"N" + b"ACGT" * 20
        text = b">r\n" + seq + b"\n"
        idx = host.index_reads(text)
        rp, cont = host.pack_reads(text, idx["seq_s"], idx["seq_e"], idx["length"], k)
        plens, p = [], int(rp[0])
        while p < int(rp[1]):
            plens.append(int(cont[p]))
            p += 1 + (plens[-1] + 7) // 8
        assert plens == [q.size for q in hu.parts_of(seq, k)], n
        assert sum(x - k + 1 for x in plens) == n - k + 1 + 80 - k + 1


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
    hm = os.path.join(tmp, "hm.csv")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, wherever this runs

    def refused(r, word):
        assert r.returncode == 1 and "--hit-maps" in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr

    refused(_run(base + ["-O", reads, "--hit-maps", hm, "--db-sharded"], env=env), "--db-sharded")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--hit-maps", hm, "--parts", "2"], env=env), "--db-sharded")
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    refused(_run(base + ["-O", lo, "-R", lr, "--hit-maps", hm], env=env), "list-of-files")
    refused(_run(base + ["-O", reads, "--hit-maps", reads], env=env), "overwrite the input")
    refused(_run(base + ["-P", m1, m2, "--hit-maps", m2], env=env), "overwrite the input")
    link = os.path.join(tmp, "link.fq")
    os.symlink(reads, link)                                  # another name of the input
    refused(_run(base + ["-O", reads, "--hit-maps", link], env=env), "overwrite the input")
    refused(_run(base + ["-O", reads, "-R", os.path.join(tmp, "o"), "--hit-maps", os.path.join(tmp, "o.csv")], env=env), "overwrite the result CSV")
    for opt in ("--abundance", "--kmer-report", "--density", "--rank-report", "--classified-out", "--unclassified-out"):
        refused(_run(base + ["-O", reads, opt, hm, "--hit-maps", hm], env=env), "another output")
    other = os.path.join(tmp, "ab.csv")
    open(other, "w").write("")
    os.link(other, os.path.join(tmp, "ab_again.csv"))         # the same inode under another name
    refused(_run(base + ["-O", reads, "--abundance", other, "--hit-maps", os.path.join(tmp, "ab_again.csv")], env=env), "another output")
    r = _run(base + ["-O", reads, "--hit-maps"], env=env)
    assert r.returncode == 1 and "Please specify the file of the hit maps!" in r.stderr
    r = _run(base + ["-O", reads, "--hit-maps", hm, "--extended"], env=env)
    assert r.returncode == 1 and "--extended" in r.stderr
    assert open(reads, "rb").read()[:1] == b"@" and not os.path.exists(hm)
    r = _run([EXE, "--help"])
    assert "--hit-maps <file>" in r.stdout


# ---- the host functions under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ------------------------
def test_host_functions_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "hitmap_host_check")
    csrc = os.path.join(gu.ROOT, "cuclark_amd", "csrc")
    # (the sanitizer runtimes are linked statically: the program runs in the environment as it is)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
              "-I", os.path.join(gu.ROOT, "include"), "-I", csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
              os.path.join(gu.ROOT, "tools", "hitmap_host_check.cpp"), os.path.join(csrc, "mic_host.cpp"), "-o", exe, "-lpthread"])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(17)
    cases = [[(b"r%d" % i, parts) for i, parts in enumerate(LABEL_CASES.values())]]
    cases.append([])                                                              # a batch without reads
    cases.append([(b"q" * int(rng.integers(1, 60)), [rng.integers(0, T + 2, int(rng.integers(0, 90))).tolist() for _ in range(int(rng.integers(0, 4)))])
                  for _ in range(40)])
    blob_in = struct.pack("<I", T) + b"".join(struct.pack("<I", len(n)) + n.encode() for n in TNAMES)
    for reads in cases:
        blob_in += struct.pack("<I", len(reads))
        for name, parts in reads:
            blob_in += struct.pack("<I", len(name)) + name + struct.pack("<I", len(parts)) + np.array([len(p) for p in parts], np.uint32).tobytes()
            blob_in += np.array([x for p in parts for x in p], np.uint32).tobytes()
    path_in, path_out = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    open(path_in, "wb").write(blob_in)
    r = _run([exe, path_in, path_out])
    assert r.returncode == 0 and f"{len(cases)} cases" in r.stdout, r.stdout + r.stderr
    blob, pos = open(path_out, "rb").read(), 0
    for reads in cases:
        per = [hu.rle_words(parts, T) for _, parts in reads]
        off = np.cumsum([0] + [len(w) for w in per]).astype(np.uint32)
        words = np.array([x for w in per for x in w], np.uint32)
        (nw,) = struct.unpack_from("<I", blob, pos); pos += 4
        got_off = np.frombuffer(blob, np.uint32, len(reads) + 1, pos); pos += 4 * (len(reads) + 1)
        got_words = np.frombuffer(blob, np.uint32, nw, pos); pos += 4 * nw
        (tb,) = struct.unpack_from("<Q", blob, pos); pos += 8
        text = blob[pos:pos + tb]; pos += tb
        assert nw == words.size and (got_off == off).all() and (got_words == words).all()
        assert text == hu.format_text([n for n, _ in reads], off, words, TNAMES)
    assert pos == len(blob)
