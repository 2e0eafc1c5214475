"""Read splitting on the MI355X (csrc/mic_split.hip; the rule: csrc/mic_split.h): the kernels alone on torch tensors, the ingest path
(mic_split_start + mic_ingest_classify[_group] + mic_ingest_split_text) and exe/cuCLARK --classified-out / --unclassified-out on
every input route, all against the restatement of the rule in tests/test_split_reads.py."""
import gzip
import os
import re

import numpy as np
import pytest

import golden_util as gu
from test_split_reads import FILTERS, SPLIT, classes_from_csv, cut, filt_tuple, is_classified, record_starts, restate, _run

pytestmark = pytest.mark.gpu


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
def _partition(text, starts, cls, which):
    """the nb + 1 bytes of the partition buffer, 0xA5 where nothing is written, and (a, b)"""
    ends = list(starts[1:]) + [len(text)]
    recs = [text[s:e] for s, e in zip(starts, ends)]
    if not text.endswith(b"\n"):
        recs[-1] += b"\n"
    c = b"".join(r for r, y in zip(recs, cls) if y)
    u = b"".join(r for r, y in zip(recs, cls) if not y)
    buf = (c if which & 1 else b"\xa5" * len(c)) + (u if which & 2 else b"\xa5" * len(u))
    return buf + b"\xa5" * (len(text) + 1 - len(buf)), len(c), len(u)


def _kernel_text(rng, unterminated):
    lens = [9 + (i % 72) for i in range(2016)]            # 9 .. 80, 28 times: every residue mod 16 of source and destination start
    lens[700] = 5000
    lens[1300] = 64
    recs = []
    for n in lens:
        body = rng.integers(33, 127, n - 1).astype(np.uint8).tobytes()
        recs.append(body + b"\n")
    text = b"".join(recs)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
    return (text[:-1] if unterminated else text), starts


def _patterns(n):
    return {
        "all": [True] * n, "none": [False] * n, "alternating": [i % 2 == 0 for i in range(n)],
        "runs": [bool(x) for x in np.repeat([(i % 2 == 0) for i in range(n)], [1 + i % 7 for i in range(n)])[:n]],
        "first": [i == 0 for i in range(n)], "last": [i == n - 1 for i in range(n)],
    }


@pytest.mark.parametrize("unterminated", [False, True])
def test_kernels_alone(unterminated):
    import torch
    from cuclark_amd import MiClarkDB, host
    rng = np.random.default_rng(31)
    text, starts = _kernel_text(rng, unterminated)
    n, nb = len(starts), len(text)
    dev = torch.device("cuda:0")
    d_text = torch.zeros((nb + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    d_text[:nb] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    d_starts = torch.from_numpy(starts.view(np.int32)).to(dev)
    with MiClarkDB(31, 6) as e:
        def run(rows, norms, filt, which, n_rec=n, text_b=text, d_t=d_text, d_s=d_starts):
            d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.uint32).view(np.int32)).to(dev)
            d_norm = torch.from_numpy(np.ascontiguousarray(norms, np.uint32).view(np.int32)).to(dev)
            d_out = torch.full((len(text_b) + 1 + 64,), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            tot = e.split_device(d_t.data_ptr(), len(text_b), d_s.data_ptr(), n_rec, d_rows.data_ptr(), d_norm.data_ptr(), d_out.data_ptr(), filt, which)
            out = d_out.cpu().numpy().tobytes()
            assert out[len(text_b) + 1:] == b"\xa5" * 64
            return tot, out[:len(text_b) + 1]
        norms = np.full(n, 150, np.uint32)
        for name, cls in _patterns(n).items():
            rows = np.zeros((n, 8), np.uint32)
            rows[np.array(cls), :5] = (40, 2, 30, 1, 10)
            for which in (1, 2, 3):
                want, a, b = _partition(text, starts, cls, which)
                tot, got = run(rows, norms, host.abund_filter(), which)
                assert tot == (a, b, sum(cls), n - sum(cls)), (name, which)
                assert a + b == nb + (1 if unterminated else 0)
                assert got == want, (name, which)
        # the rule itself on the device: rows on and around the thresholds, every filter of the CPU test
        from test_split_reads import _crafted_rows
        norms = rng.integers(1, 400, n).astype(np.uint32)
        norms[::3] = 130
        rows = _crafted_rows(rng, n, norms, 31, 6)
        for c, g in FILTERS:
            cls = [is_classified(rows[r], norms[r], 31, 6, filt_tuple(c, g)) for r in range(n)]
            assert 50 < sum(cls) < n - 50
            want, a, b = _partition(text, starts, cls, 3)
            tot, got = run(rows, norms, host.abund_filter(c, g), 3)
            assert tot == (a, b, sum(cls), n - sum(cls)) and got == want, (c, g)
            assert sum(cls) == int(host.abundance_host(rows, norms, 31, 6, host.abund_filter(c, g))[2:].sum())
        # n = 1, in either class, with and without the appended line feed
        one = text[:9] if not unterminated else text[:8]
        d_one = torch.zeros(12, dtype=torch.uint8, device=dev)
        d_one[:len(one)] = torch.from_numpy(np.frombuffer(one, np.uint8).copy()).to(dev)
        for c1 in (True, False):
            rows = np.zeros((1, 8), np.uint32)
            if c1:
                rows[0, :5] = (40, 2, 30, 1, 10)
            for which in (1, 2, 3):
                want, a, b = _partition(one, [0], [c1], which)
                tot, got = run(rows, np.array([150], np.uint32), host.abund_filter(), which, 1, one, d_one, d_starts[:1])
                assert tot == (a, b, int(c1), int(not c1)) and got == want and a + b == 9


# ---- 2. the ingest path ----------------------------------------------------------------------------------------------------------
def _randomize_every_third(data, rng):
    """every third record's sequence replaced by uniformly random nucleotides (line structure, '\\r' and lengths kept)"""
    st = record_starts(data) + [len(data)]
    fasta = data[:1] == b">"
    out = []
    for r in range(len(st) - 1):
        rec = data[st[r]:st[r + 1]]
        if r % 3 == 2:
            lines = rec.split(b"\n")
            for i in range(1, len(lines) if fasta else 2):
                body = lines[i].rstrip(b"\r")
                lines[i] = rng.choice(list(b"ACGT"), len(body)).astype(np.uint8).tobytes() + lines[i][len(body):]
            rec = b"\n".join(lines)
        out.append(rec)
    return b"".join(out)


def _low_qualities(data, rng):
    """FASTQ: a stretch of quality '#' (Phred 2) in the middle of every fifth record"""
    st = record_starts(data) + [len(data)]
    out = []
    for r in range(len(st) - 1):
        rec = data[st[r]:st[r + 1]]
        if r % 5 == 0:
            lines = rec.split(b"\n")
            q = bytearray(lines[3])
            n = len(q.rstrip(b"\r"))
            q[n // 3:n // 3 + n // 4] = b"#" * len(q[n // 3:n // 3 + n // 4])
            lines[3] = bytes(q)
            rec = b"\n".join(lines)
        out.append(rec)
    return b"".join(out)


def _oracle_rows(odb, k, data, T):
    from cuclark_amd import host
    idx = host.index_reads(data)
    rp, cont = host.pack_reads(data, idx["seq_s"], idx["seq_e"], idx["length"], k)
    counts, bad = odb.query_batch(k, rp, cont, T)
    assert bad == 0
    return gu.oracle().result_from_counts(counts), idx["length"]


INGEST_FILTERS = [("0.5", "0"), ("0.9", "0.5")]


@pytest.mark.parametrize("k,dbname", [(31, "full_k31_u32"), (27, "light_k27_u32")])
def test_ingest_split_equals_the_restatement(k, dbname):
    from cuclark_amd import MiClarkDB, MicError, _lib, host
    from test_ingest import _engine, _genomes, _random_reads
    names = gu.target_names()
    T = len(names)
    genomes = _genomes()
    rng = np.random.default_rng(700 + k)
    fq = _low_qualities(_randomize_every_third(_random_reads(rng, genomes, 700, fasta=False), rng), rng)
    texts = {
        "fastq": fq,
        "fastq_crlf": _randomize_every_third(_random_reads(rng, genomes, 700, fasta=False, crlf=True), rng),
        "fastq_no_final_lf": fq[:-1],
        "fasta_wrapped": _randomize_every_third(_random_reads(rng, genomes, 700, fasta=True), rng),
    }
    # the input populates both classes under both filters: counted on the CPU, by the oracle
    odb, _ = gu.oracle_db_from_golden(dbname)            # (loaded once: the full table's load is most of this test's time)
    for name, data in texts.items():
        rows, lengths = _oracle_rows(odb, k, data, T)
        assert len(rows) == 700
        for c, g in INGEST_FILTERS:
            n_c = sum(is_classified(rows[r], lengths[r], k, T, filt_tuple(c, g)) for r in range(700))
            assert n_c >= 50 and 700 - n_c >= 50, (name, c, g, n_c)
    del odb
    with _engine(k, names, dbname) as e:
        e.ingest_alloc(1, 4 << 20, names, want_results=True)
        plain = {}
        for name, data in texts.items():
            plain[name] = e.ingest_classify(0, data)
            assert plain[name]["status"] == 0 and plain[name]["n_reads"] == 700
            with pytest.raises(MicError) as ei:               # the split is not started: the batch left none
                e.ingest_split_text(0)
            assert ei.value.code == -5
        for c, g in INGEST_FILTERS:
            for name, data in texts.items():
                lengths = host.index_reads(data)["length"]
                for which in ((3, 1, 2) if name == "fastq" else (3,)):
                    e.split_start(host.abund_filter(c, g), which)
                    r = e.ingest_classify(0, data)
                    assert r["status"] == 0
                    assert r["csv"] == plain[name]["csv"] and (r["results"] == plain[name]["results"]).all()
                    want_c, want_u, cls = restate(data, r["results"], lengths, k, T, filt_tuple(c, g))
                    s = e.ingest_split_text(0)
                    assert (s["n_classified"], s["n_unclassified"]) == (sum(cls), 700 - sum(cls)), (name, c, g, which)
                    assert s["classified"] == (want_c if which & 1 else None), (name, c, g, which)
                    assert s["unclassified"] == (want_u if which & 2 else None), (name, c, g, which)
                    assert sum(cls) == int(host.abundance_host(r["results"], lengths, k, T, host.abund_filter(c, g))[2:].sum())
                    if which == 3:
                        assert len(want_c) + len(want_u) == len(data) + (0 if data.endswith(b"\n") else 1)
                        r2 = e.ingest_classify(0, data, csv=False)          # MIC_INGEST_NO_CSV: the same split
                        assert r2["status"] == 0 and r2["csv"] == b""
                        s2 = e.ingest_split_text(0)
                        assert s2 == s
        # the masks change the classes, never the bytes
        data = texts["fastq"]
        lengths = host.index_reads(data)["length"]
        e.split_stop()
        e.ingest_set_min_quality(20)
        e.ingest_set_low_complexity(20)
        masked = e.ingest_classify(0, data)
        assert masked["status"] == 0 and (masked["results"][:, 0] != plain["fastq"]["results"][:, 0]).any()
        e.split_start(host.abund_filter("0.9", "0.5"))
        r = e.ingest_classify(0, data)
        assert r["status"] == 0 and r["csv"] == masked["csv"] and (r["results"] == masked["results"]).all()
        want_c, want_u, cls = restate(data, masked["results"], lengths, k, T, filt_tuple("0.9", "0.5"))
        s = e.ingest_split_text(0)
        assert s["classified"] == want_c and s["unclassified"] == want_u
        assert cls != restate(data, plain["fastq"]["results"], lengths, k, T, filt_tuple("0.9", "0.5"))[2]
        e.ingest_set_min_quality(0)
        e.ingest_set_low_complexity(0)
        # FASTQ without its quality lines is refused while the split is started; a batch handed back leaves nothing
        two_line = b"@r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n"
        with pytest.raises(MicError) as ei:
            e.ingest_classify(0, two_line, flags=_lib.MIC_INGEST_FASTQ_2LINE)
        assert ei.value.code == -1
        r = e.ingest_classify(0, b">a\nACGT\n>b\n>c\nACGT\n")
        assert r["status"] & _lib.MIC_INGEST_FALLBACK
        with pytest.raises(MicError) as ei:
            e.ingest_split_text(0)
        assert ei.value.code == -5
        r = e.ingest_classify(0, texts["fasta_wrapped"])          # the slot is usable afterwards
        assert r["status"] == 0 and e.ingest_split_text(0)["n_classified"] + e.ingest_split_text(0)["n_unclassified"] == 700
        with pytest.raises(MicError):
            e.split_start(_lib.MicAbundFilter(5, 7, 0, 1))
        with pytest.raises(MicError):
            e.split_start(host.abund_filter(), 0)
        e.split_stop()
        e.ingest_free()


def test_group_of_three_parts_splits_like_one_engine():
    from cuclark_amd import MiClarkDB, host
    from test_ingest import _engine, _genomes, _random_reads
    k, dbname = 31, "full_k31_u32"
    names = gu.target_names()
    T = len(names)
    rng = np.random.default_rng(77)
    data = _randomize_every_third(_random_reads(rng, _genomes(), 700, fasta=False), rng)
    f = host.abund_filter("0.9", "0.5")
    with _engine(k, names, dbname) as e:
        e.ingest_alloc(1, 4 << 20, names, want_results=True)
        e.split_start(f)
        r1 = e.ingest_classify(0, data)
        s1 = e.ingest_split_text(0)
        e.ingest_free()
    assert r1["status"] == 0 and min(s1["n_classified"], s1["n_unclassified"]) >= 50
    db = gu.load_golden_db(dbname)
    group = [MiClarkDB(k, T) for _ in range(3)]
    try:
        for p, g in enumerate(group):
            g.set_part(p, 3)
            g.read_arrays(gu.golden_sizes(db), db["ky"], db["lb"])
        group[1].ingest_alloc(1, 4 << 20, names, want_results=True)
        group[1].split_start(f)
        r3 = MiClarkDB.ingest_classify_group(group, 1, 0, data)
        assert r3["status"] == 0 and r3["csv"] == r1["csv"] and (r3["results"][:, :5] == r1["results"][:, :5]).all()
        assert group[1].ingest_split_text(0) == s1
        want_c, want_u, _ = restate(data, r3["results"], host.index_reads(data)["length"], k, T, filt_tuple("0.9", "0.5"))
        assert (s1["classified"], s1["unclassified"]) == (want_c, want_u)
    finally:
        for g in group:
            g.close()


# ---- 3. the command line: every route of a single input ---------------------------------------------------------------------------------
def test_cli_routes_give_the_same_files(tmp_path):
    from test_cli import _db_dir, _run_many, _targets_file
    tmp = str(tmp_path)
    t, d = _targets_file(tmp), _db_dir(tmp, "light_k27_u32", light=True)       # (the light database: 58 M buckets, loaded in a blink)
    exe_l = os.path.join(gu.ROOT, "exe", "cuCLARK-l")
    rng = np.random.default_rng(3)
    lines = (open(os.path.join(gu.GOLDEN, "reads_k27.fq"), "rb").read() * 4).split(b"\n")
    for i in range(3, len(lines), 4):        # (the golden qualities are uniform in Phred 0 .. 40: Q20 would mask every k-mer away)
        lines[i] = b"I" * len(lines[i])
    fq_text = _low_qualities(b"\n".join(lines), rng)      # Phred 40 but for a stretch of Phred 2 in every fifth record
    fa_text = open(os.path.join(gu.GOLDEN, "reads_k27.fa"), "rb").read() * 3
    # a batch handed back in the middle of the stream: a FASTA record without a sequence line among the reads (MIC_INGEST_ODD_RECORD)
    fa_st = record_starts(fa_text)
    back_text = fa_text + fa_text[:fa_st[len(fa_st) // 2]] + b">lonely header\n" + fa_text[fa_st[len(fa_st) // 2]:] + fa_text
    back = os.path.join(tmp, "back.fa")
    open(back, "wb").write(back_text)
    fq, fa, gz = os.path.join(tmp, "in.fq"), os.path.join(tmp, "in.fa"), os.path.join(tmp, "in.fq.gz")
    open(fq, "wb").write(fq_text)
    open(fa, "wb").write(fa_text)
    with gzip.open(gz, "wb") as f:
        f.write(fq_text)
    filt = ["--min-confidence", "0.6", "--min-gamma", "0.75"]
    small = {"MIC_INGEST_KB": "8", "MIC_INGEST_SLOTS": "3", "MIC_CLI_TIMING": "1"}
    # name: (input, text, extra arguments, extra environment, writes a CSV, the run without the options it is compared to)
    routes = {
        "fq_n1": (fq, fq_text, ["-n", "1"], {}, True),
        "fq_n12": (fq, fq_text, ["-n", "12"], {}, True),
        "fa_n12": (fa, fa_text, ["-n", "12"], {}, True),
        "gz_device": (gz, fq_text, ["-n", "12"], {}, True),
        "gz_host": (gz, fq_text, ["-n", "12"], {"MIC_GZ_HOST": "1"}, True),
        "gz_stripes": (gz, fq_text, ["-n", "12"], {"MIC_GZ_STRIPES": "3"}, True),
        "extended": (fq, fq_text, ["-n", "2", "--extended"], {}, True),
        "host_ingest": (fq, fq_text, ["-n", "2"], {"MIC_HOST_INGEST": "1"}, True),
        "engines3": (fq, fq_text, ["-n", "6", "-b", "6"], {"MIC_SHARD_ENGINES": "3"}, True),
        "sharded2": (fq, fq_text, ["-n", "4", "--db-sharded", "--parts", "2"], {"MIC_SHARD_ENGINES": "2"}, True),
        "split_only": (fq, fq_text, ["-n", "12"], {}, False),
        "reports": (fq, fq_text, ["-n", "12", "--abundance", "AB", "--density", "DN"], {}, True),
        "masks": (fq, fq_text, ["-n", "12", "--min-base-quality", "20", "--mask-low-complexity", "20"], {}, True),
        "unclassified_alone": (fa, fa_text, ["-n", "1"], {}, True),
        "handed_back": (back, back_text, ["-n", "12"], {}, True),
        "handed_back_split_only": (back, back_text, ["-n", "12"], {}, False),
    }

    def job(name, with_split):
        inp, _, extra, env, has_csv = routes[name]
        out = os.path.join(tmp, name + ("_s" if with_split else "_p"))
        args = [exe_l, "-T", t, "-D", d, "-O", inp, *filt]
        args += [a if a not in ("AB", "DN") else out + "." + a for a in extra]
        if has_csv or not with_split:
            args += ["-R", out]
        if with_split:
            if name != "unclassified_alone":
                args += ["--classified-out", out + ".c"]
            args += ["--unclassified-out", out + ".u"]
        return lambda: (name, with_split, out, _run(args, env=dict(os.environ, **small, **env)))
    baselines = ["fq_n1", "fa_n12", "extended", "reports", "masks", "handed_back"]
    done = _run_many([job(n, True) for n in routes] + [job(n, False) for n in baselines], workers=4)
    res = {(n, w): (out, r) for n, w, out, r in done}
    for (n, w), (out, r) in res.items():
        assert r.returncode == 0, (n, w, r.stderr)

    def read(p):
        return open(p, "rb").read()
    plain_csv = {"fq": read(res[("fq_n1", False)][0] + ".csv"), "fa": read(res[("fa_n12", False)][0] + ".csv")}
    base_of = {"extended": "extended", "reports": "reports", "masks": "masks", "fa_n12": "fa_n12", "unclassified_alone": "fa_n12",
               "handed_back": "handed_back", "handed_back_split_only": "handed_back"}
    n_batches = {}
    for name, (inp, text, extra, env, has_csv) in routes.items():
        out, r = res[(name, True)]
        base = res[(base_of.get(name, "fq_n1"), False)][0]
        if has_csv:      # the CSV is the one of the run without the options
            assert read(out + ".csv") == read(base + ".csv"), name
            csv = read(out + ".csv")
        else:
            assert not os.path.exists(out + ".csv") and "Results stored" not in r.stdout
            csv = read(base + ".csv")              # (a run without a CSV: the CSV of the same input's run without the options)
        cls, rows = classes_from_csv(csv.decode(), "0.6", "0.75")
        want_c, want_u = cut(text, cls)
        assert min(sum(cls), len(cls) - sum(cls)) >= 20, name
        assert read(out + ".u") == want_u, name
        assert f" - Unclassified objects stored in {out}.u" in r.stdout
        if name == "unclassified_alone":
            assert not os.path.exists(out + ".c")
        else:
            assert read(out + ".c") == want_c, name
        # ... and exe/split_reads gives the same files from that CSV
        csv_path = out + ".csv" if has_csv else base + ".csv"
        src = inp if not inp.endswith(".gz") else fq
        rs = _run([SPLIT, "-F", csv_path, "-O", src, "--classified-out", out + ".sc", "--unclassified-out", out + ".su", "-c", "0.6", "-g", "0.75"])
        assert rs.returncode == 0, (name, rs.stderr)
        assert read(out + ".sc") == want_c and read(out + ".su") == want_u, name
        m = re.search(r"device ingest: (\d+) batches", r.stderr)
        if m:
            n_batches[name] = int(m.group(1))
    # the handed-back batch went through the host path, among many batches that did not, with and without a CSV
    for name in ("handed_back", "handed_back_split_only"):
        m = re.search(r"device ingest: (\d+) batches .*?, (\d+) through the host path", res[(name, True)][1].stderr)
        assert m and int(m.group(1)) >= 5 and 1 <= int(m.group(2)) < int(m.group(1)), res[(name, True)][1].stderr
        assert b"lonely header\n" in read(res[(name, True)][0] + ".u")
    assert n_batches["fq_n1"] >= 5 and n_batches["fq_n12"] >= 5 and n_batches["gz_device"] >= 5 and "extended" not in n_batches
    # the masks changed classes, not bytes
    assert classes_from_csv(read(res[("masks", True)][0] + ".csv").decode(), "0.6", "0.75")[0] != classes_from_csv(plain_csv["fq"].decode(), "0.6", "0.75")[0]
    # the reports are those of the run without the options, and the abundance table's total is the classified count
    out, _ = res[("reports", True)]
    base = res[("reports", False)][0]
    assert read(out + ".AB") == read(base + ".AB") and read(out + ".DN") == read(base + ".DN")
    table = read(out + ".AB").decode().splitlines()
    cls, _ = classes_from_csv(read(out + ".csv").decode(), "0.6", "0.75")
    assert sum(int(l.split(",")[3]) for l in table[1:-1]) == sum(cls) and int(table[-1].split(",")[3]) == len(cls) - sum(cls)
