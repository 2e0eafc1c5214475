"""Kraken formats on the MI355X: kraken_len_kernel / kraken_fmt_kernel behind the engine's hit-map passes (mic_kraken_start) against the
Python restatement of tests/kraken_util.py - result rows from the per-target sums of the restated hit maps through the top-2 rule, the
class by the abundance rule, the line byte for byte - over ingest batches at the format kernel's block edges, on a database whose
lines fit the LDS stage (light_k31_u64) and on one whose lines mostly do not (the gap-sampled lightgap1_k20_u16); exe/cuCLARK
--kraken-out on every input route and --kraken-report against exe/estimate_abundance and Python.  Every comparison is equality."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import hitmap_util as hu
import kraken_util as kr
import ksketch_util as ku
from test_kraken_out import LINEAGE, RANKS, _lineage_file

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")
DBS = {"light_k31_u64": 31, "lightgap1_k20_u16": 20}
STAGE = 24576 - 3                    # bytes of a block's text that still go through the LDS stage (KRAKEN_LDS in csrc/mic_ingest.hip)
STRICT = ("0.9", "0.2")


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=300, env=e, **kw)


def _genomes():
    return [b"".join(ku.sequences(open(fn, "rb").read())) for fn, _ in gu.target_files_and_labels()]


def _fastq(name, seq):
    return b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"


def _pool(k, fastq):
    """513 records (name, sequence): the golden reads (some hold Ns) under fresh names, a hand-made chimera of
    two targets, a read of k - 1 nucleotides, a read with an N in the middle of a target"""
    g = _genomes()
    seqs = ku.sequences(ku.golden_reads(k))
    assert any(b"N" in s for s in seqs)
    recs = [(b"r%d" % i, seqs[i % len(seqs)]) for i in range(513)]
    recs[3] = (b"chimera", g[0][100:220] + g[3][300:420])
    recs[5] = (b"short", g[0][50:50 + k - 1])
    recs[254] = (b"with_N", g[1][400:470] + b"N" + g[1][471:560])
    recs[256] = (b"a_name_of_more_than_forty_bytes_is_cut_to_39", g[6][10:160])
    return recs


def _text(recs, fastq):
    return b"".join(_fastq(n, s) if fastq else b">" + n + b"\n" + s + b"\n" for n, s in recs)


@pytest.fixture(scope="module")
def pools():
    """per database: its dict and arrays, the 513 records, and their expected lines under the default and the strict filter (computed once)"""
    names = gu.target_names()
    out = {}
    for name, k in DBS.items():
        dct, db = ku.golden_dict(name)
        fastq = k == 31
        recs = _pool(k, fastq)
        text = _text(recs, fastq)
        rn, res, norm, off, words = kr.rows_of(dct, text, k, len(names))
        lines = {f: kr.format_text(rn, res, norm, k, kr.filt(*f), off, words, names).splitlines(keepends=True) for f in (("0.5", "0"), STRICT)}
        out[name] = dict(k=k, dct=dct, db=db, fastq=fastq, recs=recs, lines=lines, res=res, norm=norm)
    return out


def _engine(p, slot_bytes=256 << 10):
    from cuclark_amd import MiClarkDB
    e = MiClarkDB(p["k"], len(gu.target_names()))
    e.read_arrays(gu.golden_sizes(p["db"]), p["db"]["ky"], p["db"]["lb"])
    e.ingest_alloc(1, slot_bytes, gu.target_names(), want_results=True)
    return e


# ---- the engine over ingest batches ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DBS))
def test_engine_text_at_the_block_edges(pools, name):
    """1, 255, 256, 257 and 513 reads: the text equals the restatement, with and without MIC_INGEST_NO_CSV, under the default filter and
    under one that flips some reads' class; the result rows the restatement derives are the kernel's"""
    from cuclark_amd import host
    p = pools[name]
    loose, strict = p["lines"][("0.5", "0")], p["lines"][STRICT]
    flipped = [i for i in range(513) if loose[i] != strict[i]]
    assert flipped and all(loose[i][:1] == b"C" and strict[i][:1] == b"U" for i in flipped)
    assert loose[5] == b"U\tshort\t0\t%d\t0:0\n" % (p["k"] - 1)
    assert len({t.split(b":")[0] for t in loose[3].rstrip(b"\n").split(b"\t")[4].split(b" ")} - {b"0", b"|"}) == 2, loose[3]      # the chimera: two targets
    assert b"|:|" in loose[254] and loose[256].split(b"\t")[1] == b"a_name_of_more_than_forty_bytes_is_cut_"
    block_bytes = [sum(map(len, loose[a:a + 256])) for a in (0, 256)]
    if name.startswith("lightgap"):
        assert block_bytes[0] <= STAGE < block_bytes[1]      # many one-k-mer runs: one block goes through the stage, its neighbour stores directly
    else:
        assert max(block_bytes) <= STAGE           # these go through the stage
    with _engine(p) as e:
        for f, lines in ((("0.5", "0"), loose), (STRICT, strict)):
            e.kraken_start(host.abund_filter(*f))
            for n in (1, 255, 256, 257, 513):
                for csv in (True, False) if n in (1, 257) else (True,):
                    out = e.ingest_classify(0, _text(p["recs"][:n], p["fastq"]), csv=csv)
                    assert out["status"] == 0 and out["n_reads"] == n and (out["csv"] != b"") == csv
                    got = e.ingest_kraken_text(0)
                    assert got == b"".join(lines[:n]), (name, f, n, csv)
                    assert (out["results"][:, :5] == p["res"][:n, :5]).all()
        e.kraken_stop()


@pytest.mark.gpu
def test_one_block_overflows_the_stage_between_two_that_fit(pools):
    """768 reads on the gap-sampled database: blocks 0 and 2 are 150-nt reads without hits (short lines: staged), block 1 holds ten reads
    of 5 000 nt cut from the targets among them, whose lines of 3.5 KB each outgrow the stage (direct stores)"""
    p = pools["lightgap1_k20_u16"]
    k, names = p["k"], gu.target_names()
    g = _genomes()
    rng = np.random.default_rng(5)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    recs = [(b"q%d" % i, rnd(150)) for i in range(768)]
    for j, i in enumerate((256, 300, 301, 350, 400, 401, 402, 470, 510, 511)):
        recs[i] = (b"long_%d" % j, (g[j % 8] + g[(j + 1) % 8])[37 * j:37 * j + 5000])
    recs[0] = p["recs"][0]
    recs[767] = p["recs"][3]
    text = _text(recs, False)
    lines = kr.text_of(p["dct"], text, k, names).splitlines(keepends=True)
    blocks = [sum(map(len, lines[a:a + 256])) for a in (0, 256, 512)]
    assert blocks[0] <= STAGE and blocks[2] <= STAGE and blocks[1] > STAGE and len(lines[300]) > 3000, blocks
    with _engine(p, 512 << 10) as e:
        e.kraken_start()
        out = e.ingest_classify(0, text)
        assert out["status"] == 0 and out["n_reads"] == 768
        got = e.ingest_kraken_text(0)
        assert got == b"".join(lines)


@pytest.mark.gpu
def test_paired_text_and_masks(pools):
    """MIC_INGEST_PAIRED: the length is the merged length minus one and the mate joint prints |:|; both masks on: the text is the
    restatement's on the masked text"""
    from cuclark_amd import host
    p = pools["light_k31_u64"]
    k, names = p["k"], gu.target_names()
    f1, f2 = (open(os.path.join(gu.GOLDEN, f"pairs_k31_{i}.fq"), "rb").read() for i in (1, 2))
    merged = gu.merge_pairs(f1, f2)
    want = kr.text_of(p["dct"], merged, k, names, paired=True)
    seqs = ku.sequences(merged)
    assert want.count(b"|:|") >= 30 and want.split(b"\n")[0].split(b"\t")[3] == str(len(seqs[0]) - 1).encode()
    with _engine(p) as e:
        e.kraken_start()
        for csv in (True, False):
            out = e.ingest_classify(0, merged, paired=True, csv=csv)
            assert out["status"] == 0
            assert e.ingest_kraken_text(0) == want
        # both masks: six reads with a homopolymer for the low-complexity mask, quality '#' under the threshold for the quality mask
        text = open(os.path.join(gu.GOLDEN, "reads_k31.fq"), "rb").read()
        for i, s in enumerate(ku.sequences(text)[:6]):
            s = s[:60] + b"A" * 40 + s[60:]
            text += b"@lowc%d\n" % i + s + b"\n+\n" + b"I" * 30 + b"#" * 3 + b"I" * (len(s) - 33) + b"\n"
        e.ingest_set_min_quality(3)
        e.ingest_set_low_complexity(20)
        seen = bytes(host.mask_low_complexity(host.mask_quality(text, 3), 20))
        assert seen.count(b"N") >= text.count(b"N") + 6 * 40 + 6 * 3
        assert e.ingest_classify(0, text)["status"] == 0
        assert e.ingest_kraken_text(0) == kr.text_of(p["dct"], seen, k, names)


@pytest.mark.gpu
def test_a_small_slot_grows_its_buffers(pools):
    """a slot of 64 KiB: its first word buffer holds 1536 words, its first text buffer 20 KiB; the gap-sampled database's batch outgrows
    both, the batches before and after it do not"""
    p = pools["lightgap1_k20_u16"]
    loose = p["lines"][("0.5", "0")]
    n_big = 300
    big, small = _text(p["recs"][:n_big], False), _text(p["recs"][:5], False)
    want_big, want_small = b"".join(loose[:n_big]), b"".join(loose[:5])
    assert len(big) < (64 << 10) - 4096 and len(want_big) > 20 << 10 and want_big.count(b":") > 2 * 1536
    with _engine(p, 64 << 10) as e:
        e.kraken_start()                                 # started behind the allocation: the buffers come with the first batch
        for data, want in ((small, want_small), (big, want_big), (small, want_small), (big, want_big)):
            assert e.ingest_classify(0, data)["status"] == 0
            assert e.ingest_kraken_text(0) == want
        e.ingest_free()
        e.ingest_alloc(1, 64 << 10, gu.target_names())   # started by the allocation: the buffers come with the slots
        assert e.ingest_classify(0, big, csv=False)["status"] == 0
        assert e.ingest_kraken_text(0) == want_big


@pytest.mark.gpu
def test_state_rules(pools):
    """a run has one text or the other: the second start is MIC_E_STATE in either order; each text call is MIC_E_STATE while the other
    format is on; a handed-back batch leaves no text; a group of engines and a bad filter are refused; with hit maps started the
    hit-map text is what it was"""
    from cuclark_amd import MiClarkDB, _lib, host
    from cuclark_amd._lib import MicError
    p = pools["light_k31_u64"]
    k, names = p["k"], gu.target_names()
    batch = _text(p["recs"][:40], True)
    want_k, want_h = b"".join(p["lines"][("0.5", "0")][:40]), hu.text_of(p["dct"], batch, k, names)

    def code(fn, *a):
        with pytest.raises(MicError) as err:
            fn(*a)
        return err.value.code

    with _engine(p) as e, MiClarkDB(k, len(names)) as e2:
        assert e.ingest_classify(0, batch)["status"] == 0
        assert code(e.ingest_kraken_text, 0) == -5 and code(e.ingest_hitmap_text, 0) == -5        # neither started: nothing was made
        e.kraken_start()
        assert code(e.hitmap_start) == -5
        e.hitmap_stop()                                  # (the stop call of the format that is not on does nothing)
        e.kraken_start()                                 # (again: fine)
        assert e.ingest_classify(0, batch)["status"] == 0
        assert code(e.ingest_hitmap_text, 0) == -5
        assert e.ingest_kraken_text(0) == want_k
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + batch
        assert e.ingest_classify(0, bad, csv=False)["status"] & 1
        assert code(e.ingest_kraken_text, 0) == -5       # handed back: no text
        assert code(MiClarkDB.ingest_classify_group, [e, e2], 0, 0, batch) == -7
        assert code(e.kraken_start, _lib.MicAbundFilter(5, 7, 0, 1)) == -1
        e.kraken_stop()
        assert e.ingest_classify(0, batch)["status"] == 0
        assert code(e.ingest_kraken_text, 0) == -5 and code(e.ingest_hitmap_text, 0) == -5
        e.hitmap_start()
        assert code(e.kraken_start) == -5
        e.kraken_stop()
        assert e.ingest_classify(0, batch)["status"] == 0
        assert code(e.ingest_kraken_text, 0) == -5       # the hit-map format is on
        assert e.ingest_hitmap_text(0) == want_h
        e.hitmap_stop()
        e.kraken_start(host.abund_filter(*STRICT))
        assert e.ingest_classify(0, batch)["status"] == 0
        assert e.ingest_kraken_text(0) == b"".join(p["lines"][STRICT][:40])


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_db(tmp_path_factory):
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path_factory.mktemp("kraken_db"))
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


CLI_FILTER = ("0.9", "0.1")


@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["fq", "fa", "pairs"])
def test_cli_kraken_out(tmp_path, cli_db, inp):
    """every route of one input writes the same bytes, equal to the restatement: -n 1, -n 4, --extended (the batch API), the host path,
    the serial pair reader, compressed files, with and without -R; the result CSV does not change with the option"""
    tmp = str(tmp_path)
    t, dbd = cli_db
    o = lambda n: os.path.join(tmp, n)
    env = {"MIC_INGEST_KB": "64"}
    gz = lambda src, dst: gzip.open(dst, "wb").write(open(src, "rb").read())
    if inp == "pairs":
        f1, f2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
        gz(f1, o("p1.fq.gz")); gz(f2, o("p2.fq.gz"))
        plain, packed = ["-P", f1, f2], ["-P", o("p1.fq.gz"), o("p2.fq.gz")]
        text = gu.merge_pairs(open(f1, "rb").read(), open(f2, "rb").read())
    else:
        f = os.path.join(gu.GOLDEN, f"reads_k31.{inp}")
        gz(f, o(f"in.{inp}.gz"))
        plain, packed = ["-O", f], ["-O", o(f"in.{inp}.gz")]
        text = open(f, "rb").read()
    base = [EXE, "-k", "31", "-T", t, "-D", dbd, "--min-confidence", CLI_FILTER[0], "--min-gamma", CLI_FILTER[1]]
    routes = {"n1": (plain + ["-n", "1", "-R", o("r_n1")], env), "n4": (plain + ["-n", "4", "-R", o("r_n4")], env),
              "extended": (plain + ["--extended", "-R", o("r_ext")], env)}
    if inp == "fq":
        routes.update({"gz": (packed + ["-n", "4", "-R", o("r_gz")], env), "host": (plain + ["-R", o("r_host")], {"MIC_HOST_INGEST": "1"}),
                       "summary": (plain + ["-n", "4"], env)})
    if inp == "pairs":
        routes.update({"gz": (packed + ["-n", "4", "-R", o("r_gz")], env), "serial": (plain + ["-R", o("r_serial")], {"MIC_SERIAL_PAIRS": "1"}),
                       "summary": (plain + ["-n", "4"], env)})
    got = {}
    for name, (args, ev) in routes.items():
        r = _run(base + args + ["--kraken-out", o(f"k_{name}.txt")], ev)
        assert r.returncode == 0 and f"Kraken output stored in {o(f'k_{name}.txt')}" in r.stdout, (name, r.stderr)
        got[name] = open(o(f"k_{name}.txt"), "rb").read()
        assert ("Results stored" in r.stdout) == (name != "summary"), name
    dct, _ = ku.golden_dict("full_k31_u32")
    want = kr.text_of(dct, text, 31, gu.target_names(), kr.filt(*CLI_FILTER), paired=inp == "pairs")
    for name, g in got.items():
        assert g == want, name
    classes = [ln[:2] for ln in want.splitlines()]
    assert len(classes) == len(ku.sequences(text)) and classes.count(b"C\t") >= 2 and classes.count(b"U\t") >= 2      # both classes, under this filter
    if inp == "pairs":
        assert want.count(b"|:|") >= 30
    r = _run(base + plain + ["-n", "1", "-R", o("r0")], env)      # the result CSV does not change with the option
    assert r.returncode == 0, r.stderr
    assert open(o("r0.csv"), "rb").read() == open(o("r_n1.csv"), "rb").read()


@pytest.mark.gpu
def test_cli_kraken_agrees_with_the_split_and_the_report(tmp_path, cli_db):
    """one -O run with every output: the C lines' names are the records of --classified-out and the input's records that are not in
    --unclassified-out, in order; --kraken-report equals exe/estimate_abundance --kraken-report on the run's CSV and Python; the taxon
    column of a target's line is the number of its C lines"""
    tmp = str(tmp_path)
    t, dbd = cli_db
    o = lambda n: os.path.join(tmp, n)
    f = os.path.join(gu.GOLDEN, "reads_k31.fq")
    labels = gu.target_names()
    lin = _lineage_file(tmp, labels)
    conf = "0.9"
    r = _run([EXE, "-k", "31", "-T", t, "-D", dbd, "-O", f, "-R", o("r"), "-n", "4", "--min-confidence", conf, "--kraken-out", o("k.txt"),
              "--kraken-report", o("rep.txt"), "--lineage", lin, "--classified-out", o("c.fq"), "--unclassified-out", o("u.fq")], {"MIC_INGEST_KB": "64"})
    assert r.returncode == 0 and "Kraken report stored in" in r.stdout, r.stderr
    text = open(f, "rb").read()
    dct, _ = ku.golden_dict("full_k31_u32")
    rn, res, norm, off, words = kr.rows_of(dct, text, 31, len(labels))
    fl = kr.filt(conf, "0")
    want = kr.format_text(rn, res, norm, 31, fl, off, words, labels)
    lines = open(o("k.txt"), "rb").read()
    assert lines == want
    c_names = [ln.split(b"\t")[1] for ln in lines.splitlines() if ln[:1] == b"C"]
    headers = lambda p: [ln for ln in open(p, "rb").read().split(b"\n")[::4] if ln]
    first = lambda h: hu.names_of(h + b"\nA\n+\nI\n")[0]
    assert c_names == [first(h) for h in headers(o("c.fq"))] and len(c_names) > 10
    unc = set(headers(o("u.fq")))
    assert c_names == [first(h) for h in headers(f) if h not in unc] and 0 < len(unc) < len(headers(f))
    # the report: the device counters, the CSV on the CPU, Python
    cls = [kr.classified(res[i], norm[i], 31, len(labels), fl) for i in range(len(rn))]
    per = [sum(1 for i in range(len(rn)) if cls[i] and int(res[i][1]) == t_ + 1) for t_ in range(len(labels))]
    unassigned = sum(1 for i in range(len(rn)) if int(res[i][1]) == 0)
    want_rep = kr.report(unassigned, len(rn) - unassigned - sum(per), per, [(l, "UNKNOWN") for l in labels],
                         [[(LINEAGE[l][i], "UNKNOWN") for l in labels] for i in range(3)], RANKS)
    rep = open(o("rep.txt")).read()
    assert rep == want_rep
    e = subprocess.run([EST, "-F", o("r.csv"), "-c", conf, "--kraken-report", o("rep_cpu.txt"), "--lineage", lin], capture_output=True, text=True, timeout=120)
    assert e.returncode == 0 and open(o("rep_cpu.txt")).read() == rep, e.stderr
    taxon = {ln.split("\t")[5].strip(): int(ln.split("\t")[2]) for ln in rep.splitlines() if ln.split("\t")[3] == "S"}
    per_c = {}
    for ln in lines.splitlines():
        if ln[:1] == b"C":
            per_c[ln.split(b"\t")[2].decode()] = per_c.get(ln.split(b"\t")[2].decode(), 0) + 1
    assert taxon == per_c and sum(taxon.values()) == len(c_names)
    # the flat form: no lineage, no taxonomy next to the database
    r = _run([EXE, "-k", "31", "-T", t, "-D", dbd, "-O", f, "--min-confidence", conf, "--kraken-report", o("flat.txt")], {"MIC_INGEST_KB": "64"})
    assert r.returncode == 0 and open(o("flat.txt")).read() == kr.report(unassigned, len(rn) - unassigned - sum(per), per, [(l, "UNKNOWN") for l in labels]), r.stderr
