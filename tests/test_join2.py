"""The joined window of a two-part read on the pipelined road of the per-run query kernel (cuclark_amd/csrc/mic_join2.h), on the
CPU: the host model - the same index arithmetic the kernel is written with - against a brute-force concatenation of the two parts'
nucleotides.  tools/join2_check.cpp is a stand-alone program, built here with AddressSanitizer + UBSan; for k = 31, 27 and 32 it
takes every len1 from k to 128 (so len1 mod 16 = 0 .. 15), second parts from one nucleotide short of k up to one container more
than the read-ahead entry holds, both alignments of the entry, the packer's format and the terminated one, reads with a third part,
and random data behind the read.  Checked: whether the read qualifies (and that the test reads nothing behind the entry), every
nucleotide of every window dword, the bounds of the junction's k-mer positions, and the part-relative position bits of every t-mer
in a k-mer's window as a lane of either front half computes them.  Integer work: every comparison is exact."""
import os
import subprocess

import pytest

import golden_util as gu


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("join2")), "join2_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(gu.ROOT, 'cuclark_amd', 'csrc')}", "-o", exe,
                        os.path.join(gu.ROOT, "tools", "join2_check.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_the_concatenation(check, seed):
    r = subprocess.run([check, str(seed)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    reads, joined = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert reads > 150_000 and joined > 20_000
