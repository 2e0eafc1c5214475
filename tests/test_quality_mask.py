"""--min-base-quality on the CPU: the host form of the base-quality mask (mic_fastq_mask_quality, csrc/mic_qmask.h) against the rule
written out below from its definition, and the command line's handling of the two options.

The rule: in a four-line FASTQ record with sequence line S and quality line U (the bytes of the lines without their '\\n'; a '\\r'
belongs to the line), S[i] is masked iff i >= len(U) or U[i] < c0, c0 = offset + Q, bytes compared unsigned.  A masked byte becomes
'N'; nothing else changes."""
import os

import numpy as np
import pytest

import golden_util as gu
from test_cli import EXE, _run
from test_ingest import _random_reads


def reference_mask(data, c0):
    """The rule, from its definition; does not call the library."""
    lines = data.split(b"\n")
    tail = lines.pop() if data.endswith(b"\n") else None     # b"" behind a final newline is no line
    assert len(lines) % 4 == 0 and data[:1] == b"@"
    for r in range(0, len(lines), 4):
        s, u = bytearray(lines[r + 1]), lines[r + 3]
        for i in range(len(s)):
            if i >= len(u) or u[i] < c0:
                s[i] = ord("N")
        lines[r + 1] = bytes(s)
    return b"\n".join(lines) + (b"\n" if tail is not None else b"")


def with_qualities(rng, data, offset, p_low, q, ragged):
    """The records of _random_reads (qualities all 'I') with qualities drawn around the threshold: each base low with probability
    p_low; ragged: some quality lines shorter by 1..5 or longer by 3."""
    crlf = b"\r\n" in data
    lines = data.split(b"\n")
    for r in range(3, len(lines), 4):
        n = len(lines[r]) - (1 if crlf else 0)
        lo = rng.random(n) < p_low
        v = np.where(lo, rng.integers(0, q, n), rng.integers(q, 42, n)) + offset
        u = v.astype(np.uint8).tobytes()
        if ragged and rng.random() < 0.3:
            u = u[:max(0, n - int(rng.integers(1, 6)))] if rng.random() < 0.6 else u + bytes([offset + 40]) * 3
        lines[r] = u + (b"\r" if crlf else b"")
    return b"\n".join(lines)


def _genomes():
    return [b"".join(l.strip() for l in open(fn, "rb") if not l.startswith(b">")) for fn, _ in gu.target_files_and_labels()]


def test_host_form_equals_the_rule(lib):
    from cuclark_amd import host
    rng = np.random.default_rng(20)
    genomes = _genomes()
    n_rec = 0
    for trial in range(8):
        offset = 64 if trial % 2 else 33
        q = [20, 2, 30, 40][trial % 4]
        data = _random_reads(rng, genomes, 450, fasta=False, crlf=trial in (2, 3))
        data = with_qualities(rng, data, offset, [0.025, 0.3][trial % 2], q, ragged=trial >= 4)
        if trial in (1, 2, 6):
            data = data[:-1]                      # no line end after the last record
        n_rec += 450
        want = reference_mask(data, offset + q)
        assert want != data and len(want) == len(data)
        assert host.mask_quality(data, q, offset) == want, trial
        # in == out
        buf = np.frombuffer(data, np.uint8).copy()
        assert lib.mic_fastq_mask_quality(buf.ctypes.data, buf.size, offset + q, buf.ctypes.data) == 0
        assert buf.tobytes() == want, trial
        # threshold bytes at the extremes: 0 is "off", 1 masks only what has no quality byte (or a NUL), 255 masks all but 0xFF
        for c0 in (0, 1, 255):
            assert host.mask_quality(data, 0, threshold_byte=c0) == (data if c0 == 0 else reference_mask(data, c0)), (trial, c0)
    assert n_rec >= 3000
    # bytes 0x00 and 0xFF in a quality line, unsigned compare
    rec = b"@a\nACGTACGT\n+\n\x00\xff\x7f\x80!~\x00\xff\n"
    assert host.mask_quality(rec, 0, threshold_byte=0x80) == b"@a\nNCNTNNNT\n+\n\x00\xff\x7f\x80!~\x00\xff\n" == reference_mask(rec, 0x80)
    assert host.mask_quality(rec, 0, threshold_byte=255) == reference_mask(rec, 255)
    # empty sequence / empty quality line, a record cut off behind its quality line's first bytes
    rec = b"@a\n\n+\n\n@b\nACGT\n+\n\n@c\nACGT\n+\nII"
    assert host.mask_quality(rec, 20) == b"@a\n\n+\n\n@b\nNNNN\n+\n\n@c\nACNN\n+\nII" == reference_mask(rec, 53)


def test_host_form_rejects_what_is_not_four_line_fastq(lib):
    from cuclark_amd import host
    ok = b"@a\nACGT\n+\nIIII\n"
    assert host.mask_quality(ok, 20) == ok
    for bad in (b">a\nACGT\n", b"ACGT\n", ok + b"@b\nACGT\n+\n", ok + b"@b\nACGT\n", ok[:-5], b""):
        with pytest.raises(ValueError):
            host.mask_quality(bad, 20)
    out = np.full(len(ok) + 8, 7, np.uint8)
    src = np.frombuffer(ok + b"@b\nAC\n", np.uint8)
    assert lib.mic_fastq_mask_quality(src.ctypes.data, src.size, 53, out.ctypes.data) != 0 and (out == 7).all()     # nothing written
    assert lib.mic_fastq_mask_quality(src.ctypes.data, len(ok), 256, out.ctypes.data) != 0


def test_cli_bad_values_and_help(lib, tmp_path):
    r = _run([EXE, "--help"])
    assert r.returncode == 0 and "--min-base-quality <Q>" in r.stdout and "--quality-offset 33|64" in r.stdout
    t = str(tmp_path / "t.txt")
    fq = str(tmp_path / "r.fq")
    open(t, "w").write("")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    base = [EXE, "-T", t, "-D", str(tmp_path), "-O", fq, "-R", str(tmp_path / "out")]
    for extra, msg in ((["--min-base-quality", "abc"], "The minimum base quality should be an integer in [1,93]: abc"),
                       (["--min-base-quality", "2.5"], "The minimum base quality should be an integer in [1,93]: 2.5"),
                       (["--min-base-quality", "20x"], "The minimum base quality should be an integer in [1,93]: 20x"),
                       (["--min-base-quality", ""], "The minimum base quality should be an integer in [1,93]: "),
                       (["--min-base-quality", "0"], "The minimum base quality should be an integer in [1,93]: 0"),
                       (["--min-base-quality", "94"], "The minimum base quality should be an integer in [1,93]: 94"),
                       (["--min-base-quality", "-3"], "The minimum base quality should be an integer in [1,93]: -3"),
                       (["--min-base-quality", "20", "--quality-offset", "48"], "The quality offset should be 33 or 64: 48"),
                       (["--min-base-quality", "20", "--quality-offset", "x"], "The quality offset should be 33 or 64: x"),
                       (["--quality-offset", "64"], "--quality-offset goes with --min-base-quality <Q>."),
                       (["--min-base-quality"], "Please specify the minimum base quality!"),
                       (["--min-base-quality", "20", "--quality-offset"], "Please specify the quality offset!")):
        r = _run(base + extra)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "out.csv"))


def test_host_merge_of_paired_files_masks_each_mate(lib, tmp_path):
    """cuCLARK --merge-pairs with a threshold byte (the loaders' parallel merger and the serial reader, no device): the merged text of
    the files equals the merged text of the masked files."""
    rng = np.random.default_rng(9)
    genomes = _genomes()
    recs = [[], []]
    for i in range(500):
        g = genomes[int(rng.integers(len(genomes)))]
        p = int(rng.integers(0, len(g) - 400))
        for m, L in enumerate((int(rng.choice([0, 31, 100, 150])), int(rng.choice([1, 64, 65, 151])))):
            s = g[p + 150 * m:p + 150 * m + L]
            recs[m].append(b"@p%d/%d extra\n" % (i, m + 1) + s + b"\n+\n" + b"I" * L + b"\n")
    mates = [with_qualities(rng, b"".join(r), 33, 0.1, 20, ragged=True) for r in recs]
    mates[1] = mates[1][:-1]                     # the second file ends without a line end
    want = gu.merge_pairs(reference_mask(mates[0], 53), reference_mask(mates[1], 53))
    assert want != gu.merge_pairs(*mates) and want.count(b">") == 500
    f = [str(tmp_path / ("m%d.fq" % m)) for m in (1, 2)]
    for p, d in zip(f, mates):
        open(p, "wb").write(d)
    for mode, extra in (("serial", ["1", "1"]), ("parallel", ["3", "20000"])):
        out = str(tmp_path / (mode + ".fa"))
        r = _run([EXE, "--merge-pairs", f[0], f[1], out, mode, *extra, "53"])
        assert r.returncode == 0, (mode, r.stderr, r.stdout)
        assert open(out, "rb").read() == want, mode
        r = _run([EXE, "--merge-pairs", f[0], f[1], out, mode, *extra])
        assert r.returncode == 0 and open(out, "rb").read() == gu.merge_pairs(*mates), mode
