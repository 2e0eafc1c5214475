"""--mask-low-complexity on the device: classifying a text with the level set must equal classifying, without it, the same text in
which every masked base has been replaced by 'N' - byte for byte, through the mask kernel and the packer (lowc_kernel,
pack_kernel<*, true>) and every route of exe/cuCLARK.  The masked text is made by the rule written out in test_low_complexity.py
(reference_mask_lowc, the definition restated in Python), never by the library."""
import gzip
import os

import numpy as np
import pytest

import golden_util as gu
import rollup_util as ru
from test_cli import EXE, _db_dir, _run, _run_many, _targets_file
from test_ingest import _engine, _host_path, _random_reads, _same_packed
from test_low_complexity import UNITS, _genomes, plant, reference_mask_lowc, to_fasta
from test_quality_mask import reference_mask
from test_quality_mask_gpu import _qualities

LEVEL = 20
Q = 20
# The seed of the full_k31_u32 trial.  Counted on the CPU with the oracle (gu.oracle_db_from_golden("full_k31_u32")[0].classify_file
# on the planted text and on its Python-masked twin) before the test relied on them: the mask changes 277 of the 700 sequences, 337
# records keep a first assignment on the masked text, and 76 result rows differ from the unmasked text's (seeds 31 and 32: 271 / 335 /
# 52 and 266 / 343 / 57).  The test asserts the floors 200 / 50 / 30.
SEED_FULL = 33
STEPS = (0, 1, 63, 64, 65, 127, 128)            # the packer's 64-byte steps


def _fixed_records(rng, genomes):
    """Reads of 31, 64, 65, 129, 600 and 2500 bytes with a tract at each of STEPS and at the end."""
    recs = []
    g = genomes[2]
    for i, L in enumerate((31, 64, 65, 129, 600, 2500) * 3):
        p = int(rng.integers(0, len(g) - L))
        s = bytearray(g[p:p + L])
        u = UNITS[i % len(UNITS)]
        for at in STEPS[i % 3::3] + (L - 20,):
            if 0 <= at and at + 20 <= L:
                s[at:at + 20] = (u * 20)[:20]
        recs.append(b"@fix%d\n" % i + bytes(s) + b"\n+\n" + b"I" * L + b"\n")
    return b"".join(recs)


def _fastq(rng, genomes, n, crlf=False, offsets=STEPS):
    fixed = b"" if crlf else _fixed_records(rng, genomes)
    return plant(rng, _random_reads(rng, genomes, n - fixed.count(b"@fix"), fasta=False, crlf=crlf), offsets=offsets) + fixed


def _merged_pairs(fq):
    """Merged-pair text (">id\\nseq1Nseq2\\n") of consecutive records of four-line FASTQ."""
    lines = fq.split(b"\n")
    seqs = lines[1::4]
    return b"".join(b">p%d\n" % i + seqs[2 * i] + b"N" + seqs[2 * i + 1] + b"\n" for i in range(len(seqs) // 2))


def _two_line(fq):
    lines = fq.split(b"\n")
    return b"".join(h + b"\n" + s + b"\n" for h, s in zip(lines[0::4], lines[1::4]) if h)


def _four_line(two):
    lines = two.split(b"\n")
    return b"".join(h + b"\n" + q + b"\n+\n" + b"I" * len(q) + b"\n" for h, q in zip(lines[0::2], lines[1::2]) if h)


@pytest.mark.gpu
@pytest.mark.parametrize("k,dbname", [(31, "light_k31_u64"), (27, "light_k27_u32"), (20, "light_k20_u16"), (31, "full_k31_u32")])
def test_device_mask_equals_unoptioned_run_of_the_masked_text(k, dbname):
    from cuclark_amd import _lib
    names = gu.target_names()
    genomes = _genomes()
    full = dbname.startswith("full")
    rng = np.random.default_rng(SEED_FULL if full else 300 + k)
    with _engine(k, names, dbname) as e:
        e.ingest_alloc(1, 4 << 20, names, want_results=True)
        # name: (text, paired, flags, lines per FASTQ record)
        if full:
            trials = {"fastq": (plant(rng, _random_reads(rng, genomes, 700, fasta=False)), False, 0, 4)}
        else:
            fq = _fastq(rng, genomes, 700)
            trials = {
                "fastq": (fq, False, 0, 4),
                "crlf": (_fastq(rng, genomes, 700, crlf=True), False, 0, 4),
                "no_final_eol": (_fastq(rng, genomes, 700)[:-1], False, 0, 4),
                "fasta_wrapped": (to_fasta(_fastq(rng, genomes, 700), widths=(7, 60, 61, 64, 70, 0)), False, 0, 4),
                "merged_pairs": (_merged_pairs(_fastq(rng, genomes, 1400)), True, 0, 4),
                "two_line": (_two_line(fq), False, _lib.MIC_INGEST_FASTQ_2LINE, 2),
            }
        for name, (data, paired, flags, lpr) in trials.items():
            masked = reference_mask_lowc(data, LEVEL, lpr)
            n_rec = 700
            seq_changed = sum(a != b for a, b in zip(data.split(b"\n"), masked.split(b"\n")))
            assert masked != data and len(masked) == len(data)
            e.ingest_set_low_complexity(LEVEL)
            r = e.ingest_classify(0, data, paired=paired, flags=flags)
            assert r["status"] == 0, (name, r["status"])
            rp_d, ct_d = e.ingest_fetch_packed(0)
            again = e.ingest_classify(0, data, paired=paired, flags=flags)         # the slot's text was not rewritten: the same bytes
            assert again["status"] == 0 and again["csv"] == r["csv"] and (again["results"] == r["results"]).all(), name
            e.ingest_set_low_complexity(0)
            m = e.ingest_classify(0, masked, paired=paired, flags=flags)
            assert m["status"] == 0
            assert r["csv"] == m["csv"], name
            assert r["n_reads"] == m["n_reads"] == n_rec and (r["results"][:, :7] == m["results"][:, :7]).all(), name
            masked4 = masked if lpr == 4 else _four_line(masked)
            csv_h, res_h, rp_h, ct_h = _host_path(e, masked4, names, k, paired=paired)
            assert m["csv"] == csv_h, name
            _same_packed(rp_h, ct_h, rp_d, ct_d)
            # cleared: the unmasked result is back
            u = e.ingest_classify(0, data, paired=paired, flags=flags)
            assert u["status"] == 0 and u["csv"] != m["csv"], name
            if lpr == 4:
                assert u["csv"] == _host_path(e, data, names, k, paired=paired)[0], name
            if full:
                # not vacuous: the masked text still classifies, and masking changed what it classifies as
                assigned = int(np.count_nonzero(m["results"][:, 1]))
                changed = int(np.count_nonzero((m["results"][:, :7] != u["results"][:, :7]).any(axis=1)))
                print(f"full_k31_u32: the mask changes {seq_changed} sequences, {assigned} of 700 records keep a first assignment, "
                      f"{changed} rows differ from the unmasked text's")
                assert seq_changed >= 200 and assigned >= 50 and changed >= 30, (seq_changed, assigned, changed)
        # both options: this one on the quality-masked text
        c0 = 33 + Q
        data = _qualities(rng, plant(rng, _random_reads(rng, genomes, 700, fasta=False), offsets=STEPS), k, lambda i: 2 if i % 5 else 3)
        both = reference_mask_lowc(reference_mask(data, c0), LEVEL)
        assert both != reference_mask(data, c0) and both != reference_mask_lowc(data, LEVEL)
        e.ingest_set_low_complexity(LEVEL)
        e.ingest_set_min_quality(Q)
        r = e.ingest_classify(0, data)
        rp_d, ct_d = e.ingest_fetch_packed(0)
        e.ingest_set_low_complexity(0)
        e.ingest_set_min_quality(0)
        m = e.ingest_classify(0, both)
        assert r["status"] == 0 and m["status"] == 0 and r["csv"] == m["csv"] and (r["results"][:, :7] == m["results"][:, :7]).all()
        _same_packed(*_host_path(e, both, names, k)[2:], rp_d, ct_d)
        # level 150 is refused through the C ABI, 149 is the last one taken
        with pytest.raises(_lib.MicError):
            _lib.check(e.L.mic_ingest_set_low_complexity(e.h, 150))
        _lib.check(e.L.mic_ingest_set_low_complexity(e.h, 149))
        _lib.check(e.L.mic_ingest_set_low_complexity(e.h, 0))
        e.ingest_free()


@pytest.fixture(scope="module")
def cli_rig(tmp_path_factory):
    """The golden full k = 31 database laid out once, and a FASTQ of about 400 reads with planted tracts (and p = 1/40 low qualities
    for the run with both options): the file, its Python-masked twin, both gzipped, as FASTA, and two such files as mates of a pair."""
    tmp = str(tmp_path_factory.mktemp("lowc"))
    rig = dict(tmp=tmp, t=_targets_file(tmp), d=_db_dir(tmp, "full_k31_u32", light=False))
    genomes = _genomes()
    rng = np.random.default_rng(SEED_FULL)

    def put(name, data, gz=False):
        p = os.path.join(tmp, name)
        with (gzip.open(p, "wb") if gz else open(p, "wb")) as f:
            f.write(data)
        return p

    x = _qualities(rng, plant(rng, _random_reads(rng, genomes, 400, fasta=False), offsets=STEPS), 31, lambda i: 2)
    xm = reference_mask_lowc(x, LEVEL)
    assert xm != x
    fa = to_fasta(x, widths=(0, 60, 70))
    # mates: the same ids in both files
    recs1, recs2 = [], []
    for i in range(300):
        g = genomes[int(rng.integers(len(genomes)))]
        p0 = int(rng.integers(0, len(g) - 400))
        L1, L2 = int(rng.choice([40, 100, 101, 150])), int(rng.choice([31, 100, 129, 150]))
        for recs, s, tag in ((recs1, g[p0:p0 + L1], b"/1"), (recs2, g[p0 + 200:p0 + 200 + L2], b"/2")):
            recs.append(b"@pair%d" % i + tag + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    a, b = plant(rng, b"".join(recs1)), plant(rng, b"".join(recs2))
    am, bm = reference_mask_lowc(a, LEVEL), reference_mask_lowc(b, LEVEL)
    assert am != a and bm != b
    xq = reference_mask_lowc(reference_mask(x, 33 + Q), LEVEL)
    rig.update(x=put("x.fq", x), xm=put("xm.fq", xm), xg=put("xg.fq.gz", x, True), xmg=put("xmg.fq.gz", xm, True),
               fa=put("x.fa", fa), fam=put("xm.fa", reference_mask_lowc(fa, LEVEL)), xq=put("xq.fq", xq),
               a=put("a.fq", a), b=put("b.fq", b), am=put("am.fq", am), bm=put("bm.fq", bm),
               ag=put("ag.fq.gz", a, True), bg=put("bg.fq.gz", b, True), amg=put("amg.fq.gz", am, True), bmg=put("bmg.fq.gz", bm, True))
    rig["lin"] = os.path.join(tmp, "lineage.tsv")
    ru.golden_lineage_file(rig["lin"])
    return rig


@pytest.mark.gpu
def test_every_route_of_the_command_line(cli_rig):
    """For each form: the output with --mask-low-complexity 20 on the file is byte-equal to the output of the same command without
    the option on the Python-masked file."""
    g = cli_rig
    tmp = g["tmp"]
    base = [EXE, "-k", "31", "-T", g["t"], "-D", g["d"]]
    opt = ["--mask-low-complexity", str(LEVEL)]
    o = lambda n: os.path.join(tmp, n)
    env0 = dict(os.environ, MIC_CLI_TIMING="1")
    # name: (input with the option, input without, further arguments, environment, files compared, further options with the option)
    forms = {
        "plain_n1": (["-O", g["x"]], ["-O", g["xm"]], ["-n", "1"], {}, "R", []),
        "plain_n4": (["-O", g["x"]], ["-O", g["xm"]], ["-n", "4"], {"MIC_INGEST_KB": "64"}, "R", []),
        "gz": (["-O", g["xg"]], ["-O", g["xmg"]], [], {}, "R", []),
        "gz_stripes": (["-O", g["xg"]], ["-O", g["xmg"]], [], {"MIC_GZ_STRIPES": "2"}, "R", []),
        "fasta": (["-O", g["fa"]], ["-O", g["fam"]], [], {}, "R", []),
        "pairs_plain": (["-P", g["a"], g["b"]], ["-P", g["am"], g["bm"]], ["-n", "2"], {}, "R", []),
        "pairs_gz": (["-P", g["ag"], g["bg"]], ["-P", g["amg"], g["bmg"]], [], {}, "R", []),
        "extended": (["-O", g["x"]], ["-O", g["xm"]], ["--extended", "-n", "2", "-b", "3"], {}, "R", []),
        "abundance": (["-O", g["x"]], ["-O", g["xm"]], [], {}, "A", []),
        "rank": (["-O", g["x"]], ["-O", g["xm"]], ["--lineage", g["lin"], "--min-confidence", "0.75"], {}, "K", []),
        "density": (["-O", g["x"]], ["-O", g["xm"]], [], {}, "D", []),
        "sharded": (["-O", g["x"]], ["-O", g["xm"]], ["--db-sharded", "--parts", "2"], {"MIC_SHARD_ENGINES": "2"}, "R", []),
        "with_quality": (["-O", g["x"]], ["-O", g["xq"]], [], {}, "R", ["--min-base-quality", str(Q)]),
    }

    def job(name, with_opt):
        inp_o, inp_m, extra, env, kind, more = forms[name]
        tag = o(name + ("_opt" if with_opt else "_ref"))
        out = {"R": ["-R", tag], "A": ["--abundance", tag + ".tsv"], "K": ["--rank-report", tag + ".tsv"], "D": ["--density", tag + ".tsv"]}[kind]
        args = base + (inp_o if with_opt else inp_m) + out + extra + (opt + more if with_opt else [])
        return lambda: (name, with_opt, tag + (".csv" if kind == "R" else ".tsv"), _run(args, env=dict(env0, **env)))

    jobs = [job(n, w) for n in forms for w in (True, False)]
    jobs.append(lambda: ("unmasked", False, o("unmasked.csv"), _run(base + ["-O", g["x"], "-R", o("unmasked")], env=env0)))
    got = {}
    for name, with_opt, path, r in _run_many(jobs):
        assert r.returncode == 0, (name, with_opt, r.stderr)
        got[(name, with_opt)] = (open(path, "rb").read(), r)
    for name in forms:
        assert got[(name, True)][0] == got[(name, False)][0], name
        assert len(got[(name, True)][0]) > 100, name
    # the masking ran where the text is: nothing went through the host path on the streaming routes
    for name in ("plain_n1", "plain_n4", "gz", "gz_stripes", "fasta", "pairs_plain", "pairs_gz", "sharded", "abundance", "rank", "density", "with_quality"):
        assert " 0 through the host path" in got[(name, True)][1].stderr, (name, got[(name, True)][1].stderr)
    assert got[("plain_n1", True)][0] == got[("plain_n4", True)][0] == got[("gz", True)][0] == got[("gz_stripes", True)][0] == got[("sharded", True)][0]
    # the option changes the result of this file
    assert got[("unmasked", False)][0] != got[("plain_n1", True)][0]
    assert got[("unmasked", False)][0].split(b"\n")[0] == got[("plain_n1", True)][0].split(b"\n")[0]          # (the header line)
    assert got[("with_quality", True)][0] != got[("plain_n1", True)][0]


@pytest.mark.gpu
def test_batches_handed_back_are_masked_on_the_host(cli_rig):
    """A batch the device path does not take (here: every batch, MIC_HOST_INGEST=1; the host inflate, MIC_GZ_HOST=1; and the serial pair
    reader, MIC_SERIAL_PAIRS=1) is masked by the host form of the rule: the same bytes as the device routes give."""
    g = cli_rig
    base = [EXE, "-k", "31", "-T", g["t"], "-D", g["d"]]
    o = lambda n: os.path.join(g["tmp"], n)
    opt = ["--mask-low-complexity", str(LEVEL)]
    jobs = [lambda: _run(base + ["-O", g["x"], "-R", o("hb_dev")] + opt),
            lambda: _run(base + ["-O", g["x"], "-R", o("hb_host")] + opt, env=dict(os.environ, MIC_HOST_INGEST="1")),
            lambda: _run(base + ["-O", g["xg"], "-R", o("hb_gzhost")] + opt, env=dict(os.environ, MIC_GZ_HOST="1")),
            lambda: _run(base + ["-O", g["xm"], "-R", o("hb_ref")]),
            lambda: _run(base + ["-P", g["a"], g["b"], "-R", o("hb_pdev")] + opt),
            lambda: _run(base + ["-P", g["a"], g["b"], "-R", o("hb_pserial")] + opt, env=dict(os.environ, MIC_SERIAL_PAIRS="1")),
            lambda: _run(base + ["-P", g["a"], g["b"], "-R", o("hb_phost")] + opt, env=dict(os.environ, MIC_HOST_INGEST="1")),
            lambda: _run(base + ["-P", g["am"], g["bm"], "-R", o("hb_pref")])]
    for r in _run_many(jobs):
        assert r.returncode == 0, r.stderr
    rd = lambda n: open(o(n + ".csv"), "rb").read()
    assert rd("hb_dev") == rd("hb_host") == rd("hb_gzhost") == rd("hb_ref") and len(rd("hb_dev")) > 100
    assert rd("hb_pdev") == rd("hb_pserial") == rd("hb_phost") == rd("hb_pref")
