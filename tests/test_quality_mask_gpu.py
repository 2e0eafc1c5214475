"""--min-base-quality on the device: classifying a FASTQ with the threshold set must equal classifying, without it, the same FASTQ
in which every masked base has been replaced by 'N' - byte for byte, through the packer (pack_kernel<true>), the pair merge kernel
and every route of exe/cuCLARK.  The masked text is made by the rule written out in test_quality_mask.py (reference_mask), never
by the library."""
import gzip
import os

import numpy as np
import pytest

import golden_util as gu
import rollup_util as ru
from test_cli import EXE, _db_dir, _run, _run_many, _targets_file
from test_ingest import _engine, _host_path, _random_reads, _same_packed
from test_quality_mask import _genomes, reference_mask

Q = 20
HI, LO = 40, 5                       # Phred values on either side of the threshold
# The seed of the full_k31_u32 trial (and of the command line's input): with it the unoptioned run of the masked text keeps a first
# assignment for 323 of the 700 records and changes the result row of 348 of them against the unmasked text - counted on the CPU with
# the oracle (gu.oracle_db_from_golden("full_k31_u32")[0].classify_file on both texts) before the test relied on them; the test
# asserts both (>= 50).
SEED_FULL = 31


def _qualities(rng, data, k, mode_of, offset=33, p=1 / 40):
    """The records of _random_reads (qualities all 'I') with a quality mode per record (mode_of(i)):
    0 all high, 1 all low, 2 each base low with probability p, 3 low exactly at {0, 63, 64, 65, 127, 128, L-1} (the packer's 64-byte
    steps), 4 low bases that leave runs of exactly k-1 and exactly k, 5 a low base next to a real N, 6 a quality line shorter by
    1..5 or longer by 3 (over mode 2's qualities)."""
    crlf = b"\r\n" in data
    cut = 1 if crlf else 0
    lines = data.split(b"\n")
    for i, r in enumerate(range(0, len(lines) - 3, 4)):
        s = bytearray(lines[r + 1])
        L = len(s) - cut
        mode = mode_of(i)
        low = np.zeros(L, bool)
        if mode == 1:
            low[:] = True
        elif mode in (2, 6):
            low = rng.random(L) < p
        elif mode == 3:
            for j in (0, 63, 64, 65, 127, 128, L - 1):
                if 0 <= j < L:
                    low[j] = True
        elif mode == 4:
            j, step = k - 1, 0
            while j < L:
                low[j] = True
                j += 1 + (k if step % 2 == 0 else k - 1)
                step += 1
        elif mode == 5 and L >= 3:
            j = int(rng.integers(1, L - 1))
            s[j] = ord("N")
            low[j + (1 if rng.random() < 0.5 else -1)] = True
            lines[r + 1] = bytes(s)
        u = (np.where(low, LO, HI) + offset).astype(np.uint8).tobytes()
        if mode == 6:
            u = u[:max(0, L - int(rng.integers(1, 6)))] if rng.random() < 0.5 else u + bytes([offset + HI]) * 3
        lines[r + 3] = u + (b"\r" if crlf else b"")
    return b"\n".join(lines)


def _rows(csv):
    return csv.split(b"\n")[:-1]


@pytest.mark.gpu
@pytest.mark.parametrize("k,dbname", [(31, "light_k31_u64"), (27, "light_k27_u32"), (20, "light_k20_u16"), (31, "full_k31_u32")])
def test_device_mask_equals_unoptioned_run_of_the_masked_text(k, dbname):
    from cuclark_amd import _lib
    names = gu.target_names()
    genomes = _genomes()
    full = dbname.startswith("full")
    rng = np.random.default_rng(SEED_FULL if full else 200 + k)
    c0 = 33 + Q
    with _engine(k, names, dbname) as e:
        e.ingest_alloc(1, 4 << 20, names, want_results=True)
        for trial in range(1 if full else 4):
            crlf, cut_end = trial == 1, trial == 2
            data = _random_reads(rng, genomes, 700, fasta=False, crlf=crlf)
            data = _qualities(rng, data, k, (lambda i: 2) if full else (lambda i: i % 7))
            if cut_end:
                data = data[:-1]                  # no line end after the last record
            masked = reference_mask(data, c0)
            assert masked != data
            e.ingest_set_min_quality(Q)
            r = e.ingest_classify(0, data)
            assert r["status"] == 0, (trial, r["status"])
            rp_d, ct_d = e.ingest_fetch_packed(0)
            # the qualities are gone from two-line records: refused while a threshold is set
            with pytest.raises(_lib.MicError) as ei:
                e.ingest_classify(0, b"@a\nACGT\n", flags=_lib.MIC_INGEST_FASTQ_2LINE)
            assert ei.value.code == -1 and "FASTQ_2LINE" in str(ei.value)
            e.ingest_set_min_quality(0)
            m = e.ingest_classify(0, masked)
            assert m["status"] == 0
            assert r["csv"] == m["csv"], trial
            assert r["n_reads"] == m["n_reads"] == 700 and (r["results"][:, :7] == m["results"][:, :7]).all(), trial
            csv_h, res_h, rp_h, ct_h = _host_path(e, masked, names, k)
            assert m["csv"] == csv_h
            _same_packed(rp_h, ct_h, rp_d, ct_d)
            # cleared: the unmasked result is back
            u = e.ingest_classify(0, data)
            assert u["status"] == 0 and u["csv"] == _host_path(e, data, names, k)[0]
            assert u["csv"] != m["csv"]
            if full:
                # not vacuous: the masked text still classifies, and masking changed what it classifies as
                assigned = int(np.count_nonzero(m["results"][:, 1]))
                changed = int(np.count_nonzero((m["results"][:, :7] != u["results"][:, :7]).any(axis=1)))
                print(f"full_k31_u32: {assigned} of 700 records keep a first assignment, {changed} rows differ from the unmasked text's")
                assert assigned >= 50 and changed >= 50, (assigned, changed)
        # FASTA has no qualities: the same bytes with a threshold set
        fa = _random_reads(rng, genomes, 300, fasta=True)
        plain = e.ingest_classify(0, fa)
        e.ingest_set_min_quality(Q)
        assert e.ingest_classify(0, fa)["csv"] == plain["csv"] and plain["status"] == 0
        # offset 64
        data64 = _qualities(rng, _random_reads(rng, genomes, 200, fasta=False), k, lambda i: 2, offset=64, p=0.1)
        e.ingest_set_min_quality(Q, offset=64)
        r = e.ingest_classify(0, data64)
        e.ingest_set_min_quality(0)
        assert r["status"] == 0 and r["csv"] == e.ingest_classify(0, reference_mask(data64, 64 + Q))["csv"]
        with pytest.raises(_lib.MicError):
            _lib.check(e.L.mic_ingest_set_min_quality(e.h, 256))
        e.ingest_free()


@pytest.fixture(scope="module")
def cli_rig(tmp_path_factory):
    """The golden full k = 31 database laid out once, and a FASTQ of a few hundred reads with p = 1/40 low qualities: the file, its
    Python-masked twin, both gzipped, the two as mates of a pair, and the same reads with qualities written at offset 64."""
    tmp = str(tmp_path_factory.mktemp("qmask"))
    rig = dict(tmp=tmp, t=_targets_file(tmp), d=_db_dir(tmp, "full_k31_u32", light=False))
    genomes = _genomes()
    rng = np.random.default_rng(SEED_FULL)

    def put(name, data, gz=False):
        p = os.path.join(tmp, name)
        with (gzip.open(p, "wb") if gz else open(p, "wb")) as f:
            f.write(data)
        return p

    raw = _random_reads(rng, genomes, 400, fasta=False)
    x = _qualities(rng, raw, 31, lambda i: 2 if i % 9 else 6)
    x64 = bytes(x)
    lines = x64.split(b"\n")
    for r in range(3, len(lines), 4):
        lines[r] = bytes(c + 31 for c in lines[r])
    x64 = b"\n".join(lines)
    # mates: the same ids in both files
    recs1, recs2 = [], []
    for i in range(300):
        g = genomes[int(rng.integers(len(genomes)))]
        p0 = int(rng.integers(0, len(g) - 400))
        L1, L2 = int(rng.choice([40, 100, 101, 150])), int(rng.choice([31, 100, 129, 150]))
        for recs, s, tag in ((recs1, g[p0:p0 + L1], b"/1"), (recs2, g[p0 + 200:p0 + 200 + L2], b"/2")):
            recs.append(b"@pair%d" % i + tag + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    a = _qualities(rng, b"".join(recs1), 31, lambda i: 2 if i % 7 else 6)
    b = _qualities(rng, b"".join(recs2), 31, lambda i: 2 if i % 5 else 3)
    c0 = 33 + Q
    rig.update(x=put("x.fq", x), xm=put("xm.fq", reference_mask(x, c0)), xg=put("xg.fq.gz", x, True), xmg=put("xmg.fq.gz", reference_mask(x, c0), True),
               x64=put("x64.fq", x64), a=put("a.fq", a), b=put("b.fq", b), am=put("am.fq", reference_mask(a, c0)), bm=put("bm.fq", reference_mask(b, c0)),
               ag=put("ag.fq.gz", a, True), bg=put("bg.fq.gz", b, True), amg=put("amg.fq.gz", reference_mask(a, c0), True),
               bmg=put("bmg.fq.gz", reference_mask(b, c0), True))
    assert reference_mask(x64, 64 + Q).split(b"\n")[1::4] == reference_mask(x, c0).split(b"\n")[1::4]
    rig["lin"] = os.path.join(tmp, "lineage.tsv")
    ru.golden_lineage_file(rig["lin"])
    return rig


@pytest.mark.gpu
def test_every_route_of_the_command_line(cli_rig):
    """For each form: the output with --min-base-quality 20 on the file is byte-equal to the output of the same command without the
    option on the Python-masked file."""
    g = cli_rig
    tmp = g["tmp"]
    base = [EXE, "-k", "31", "-T", g["t"], "-D", g["d"]]
    opt = ["--min-base-quality", str(Q)]
    o = lambda n: os.path.join(tmp, n)
    env0 = dict(os.environ, MIC_CLI_TIMING="1")
    # name: (input with the option, input without, further arguments, environment, files compared)
    forms = {
        "plain_n1": (["-O", g["x"]], ["-O", g["xm"]], ["-n", "1"], {}, "R"),
        "plain_n4": (["-O", g["x"]], ["-O", g["xm"]], ["-n", "4"], {"MIC_INGEST_KB": "64"}, "R"),
        "gz": (["-O", g["xg"]], ["-O", g["xmg"]], [], {}, "R"),
        "gz_stripes": (["-O", g["xg"]], ["-O", g["xmg"]], [], {"MIC_GZ_STRIPES": "2"}, "R"),
        "pairs_plain": (["-P", g["a"], g["b"]], ["-P", g["am"], g["bm"]], ["-n", "2"], {}, "R"),
        "pairs_gz": (["-P", g["ag"], g["bg"]], ["-P", g["amg"], g["bmg"]], [], {}, "R"),
        "extended": (["-O", g["x"]], ["-O", g["xm"]], ["--extended", "-n", "2", "-b", "3"], {}, "R"),
        "abundance": (["-O", g["x"]], ["-O", g["xm"]], [], {}, "A"),
        "rank": (["-O", g["x"]], ["-O", g["xm"]], ["--lineage", g["lin"], "--min-confidence", "0.75"], {}, "K"),
        "sharded": (["-O", g["x"]], ["-O", g["xm"]], ["--db-sharded", "--parts", "2"], {"MIC_SHARD_ENGINES": "2"}, "R"),
        "offset64": (["-O", g["x64"]], ["-O", g["xm"]], [], {}, "R"),
    }

    def job(name, with_opt):
        inp_o, inp_m, extra, env, kind = forms[name]
        tag = o(name + ("_opt" if with_opt else "_ref"))
        out = {"R": ["-R", tag], "A": ["--abundance", tag + ".tsv"], "K": ["--rank-report", tag + ".tsv"]}[kind]
        args = base + (inp_o if with_opt else inp_m) + out + extra
        if with_opt:
            args += opt + (["--quality-offset", "64"] if name == "offset64" else [])
        return lambda: (name, with_opt, tag + (".csv" if kind == "R" else ".tsv"), _run(args, env=dict(env0, **env)))

    jobs = [job(n, w) for n in forms for w in (True, False)]
    # the unmasked file without the option, and a FASTA input with it
    jobs.append(lambda: ("unmasked", False, o("unmasked.csv"), _run(base + ["-O", g["x"], "-R", o("unmasked")], env=env0)))
    jobs.append(lambda: ("fasta", True, o("fasta.csv"), _run(base + ["-O", os.path.join(gu.GOLDEN, "reads_k31.fa"), "-R", o("fasta")] + opt, env=env0)))
    got = {}
    for name, with_opt, path, r in _run_many(jobs):
        assert r.returncode == 0, (name, with_opt, r.stderr)
        got[(name, with_opt)] = (open(path, "rb").read(), r)
    for name in forms:
        assert got[(name, True)][0] == got[(name, False)][0], name
        assert len(got[(name, True)][0]) > 100, name
    # the masking ran where the text is: nothing went through the host path on the streaming routes, and the striped inflate was used
    for name in ("plain_n1", "plain_n4", "gz", "gz_stripes", "pairs_plain", "pairs_gz", "sharded", "abundance", "rank"):
        assert " 0 through the host path" in got[(name, True)][1].stderr, (name, got[(name, True)][1].stderr)
    assert "device inflate in stripes" in got[("gz_stripes", True)][1].stderr
    assert got[("pairs_gz", True)][1].stderr.count("pairs indexed and checked") == 1
    assert got[("plain_n1", True)][0] == got[("plain_n4", True)][0] == got[("gz", True)][0] == got[("sharded", True)][0] == got[("offset64", True)][0]
    # the option changes the result of this file, and leaves FASTA input alone
    assert got[("unmasked", False)][0] != got[("plain_n1", True)][0]
    assert _rows(got[("unmasked", False)][0])[0] == _rows(got[("plain_n1", True)][0])[0]          # (the header line)
    assert got[("fasta", True)][0] == open(os.path.join(gu.GOLDEN, "expected_k31_fa.csv"), "rb").read()


@pytest.mark.gpu
def test_batches_handed_back_are_masked_on_the_host(cli_rig):
    """A batch the device path does not take (here: every batch, MIC_HOST_INGEST=1; and the serial pair reader, MIC_SERIAL_PAIRS=1)
    is masked by the host form of the rule: the same bytes as the device routes give."""
    g = cli_rig
    base = [EXE, "-k", "31", "-T", g["t"], "-D", g["d"]]
    o = lambda n: os.path.join(g["tmp"], n)
    opt = ["--min-base-quality", str(Q)]
    jobs = [lambda: _run(base + ["-O", g["x"], "-R", o("hb_dev")] + opt),
            lambda: _run(base + ["-O", g["x"], "-R", o("hb_host")] + opt, env=dict(os.environ, MIC_HOST_INGEST="1")),
            lambda: _run(base + ["-O", g["xg"], "-R", o("hb_gzhost")] + opt, env=dict(os.environ, MIC_GZ_HOST="1")),
            lambda: _run(base + ["-P", g["a"], g["b"], "-R", o("hb_pdev")] + opt),
            lambda: _run(base + ["-P", g["a"], g["b"], "-R", o("hb_pserial")] + opt, env=dict(os.environ, MIC_SERIAL_PAIRS="1")),
            lambda: _run(base + ["-P", g["am"], g["bm"], "-R", o("hb_pref")])]
    for r in _run_many(jobs):
        assert r.returncode == 0, r.stderr
    rd = lambda n: open(o(n + ".csv"), "rb").read()
    assert rd("hb_dev") == rd("hb_host") == rd("hb_gzhost") and len(rd("hb_dev")) > 100
    assert rd("hb_pdev") == rd("hb_pserial") == rd("hb_pref")
