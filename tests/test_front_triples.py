"""The three-t-mers-per-lane front half of the per-run query kernel for k = 31, m = 20 (cuclark_amd/csrc/mic_front3.h), on the CPU:
the host model - the same index arithmetic and nine-minimum combination the kernel is written with - against the brute force
min(key[i .. i+23]).  tools/front_triples_check.cpp is a stand-alone program, built here with AddressSanitizer + UBSan; it takes
every chunk size from 1 to 128 k-mers, both tables' keys, random reads and reads of tied t-mers (homopolymers, di- and
trinucleotide repeats, two letters, a repeated t-mer), and what lies past the part filled three ways - with the t-mer of the lowest
order among them - so that the part ends at every offset modulo 3 of a lane's triple; lane 0 reads the wrapped-around dword in front
of the chunk.  Checked: the sampled position of every k-mer, ~0 for the k-mers past the chunk, the number of runs, every record, the
k-mer of the closing record, and that nothing is written behind it.  Integer work: every comparison is exact."""
import os
import subprocess

import pytest

import golden_util as gu


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("front3")), "front_triples_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(gu.ROOT, 'cuclark_amd', 'csrc')}", "-o", exe,
                        os.path.join(gu.ROOT, "tools", "front_triples_check.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_the_brute_force(check, seed):
    r = subprocess.run([check, str(seed)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok: 13824 chunks"), r.stdout[-2000:] + r.stderr[-2000:]
