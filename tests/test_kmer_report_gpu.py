"""K-mer sketches on the MI355X: ksketch_kernel (mic_ksketch_device on torch tensors) against the Python restatement of
tests/ksketch_util.py - a dict of canonical k-mer -> label from the arrays the table was loaded from, and a walk over the reads' text -
on every table layout, byte for byte; the engine's sketches over ingest batches; the batch API; exe/cuCLARK --kmer-report on every
input route."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import ksketch_util as ku

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
LAYOUTS = {"direct": 1, "minimizer": 2, "super": 3, "super2": 4}       # MIC_LAYOUT_*: table layouts 0, 1, 2 and the two-strand form
GOLDEN_DBS = {20: "light_k20_u16", 27: "light_k27_u32", 31: "light_k31_u64", 32: "light_k32_u64"}
T6 = 6
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=300, env=e, **kw)


def _fasta(seqs):
    return b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs))


def _pack(text, k):
    from cuclark_amd import host
    idx = host.index_reads(text)
    return host.pack_reads(text, idx["seq_s"], idx["seq_e"], idx["length"], k)


class Dev:
    """packed reads on the device, their result rows from query_device + resolve_flagged_device, and sketches to add to"""

    def __init__(self, e, rp, cont, n_targets):
        import torch
        self.e, self.n, self.T = e, rp.size - 1, n_targets
        dev = torch.device("cuda:0")
        self.d_rp = torch.from_numpy(np.ascontiguousarray(rp, np.uint32).view(np.int32)).to(dev)
        self.d_ct = torch.from_numpy(np.concatenate([cont, np.zeros(64, np.uint16)]).view(np.int16)).to(dev)
        self.d_res = torch.zeros((self.n, 8), dtype=torch.int32, device=dev)
        self.d_regs = torch.zeros(n_targets * ku.M, dtype=torch.uint8, device=dev)
        self.d_hits = torch.zeros(n_targets, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        e.query_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), self.n, self.d_res.data_ptr())
        e.resolve_flagged_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), self.d_res.data_ptr())
        e.sync()

    def results(self):
        return self.d_res.cpu().numpy().view(np.uint32)

    def zero_rows(self, rows):
        import torch
        self.d_res[torch.from_numpy(np.asarray(rows, np.int64)).to(self.d_res.device)] = 0
        torch.cuda.synchronize()

    def add(self, n=None):
        import torch
        torch.cuda.synchronize()          # (the tensors are zeroed / copied on torch's stream, the kernel runs on the engine's)
        self.e.ksketch_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), self.n if n is None else n, self.d_res.data_ptr(),
                              self.d_regs.data_ptr(), self.d_hits.data_ptr())
        self.e.sync()
        return self.d_regs.cpu().numpy().reshape(self.T, ku.M), self.d_hits.cpu().numpy().view(np.uint64)


def _same(got, want, what=""):
    assert (got[1] == want[1]).all(), (what, got[1], want[1])
    bad = np.argwhere(got[0] != want[0])
    assert bad.size == 0, (what, bad[:5], got[0][tuple(bad[0])], want[0][tuple(bad[0])])


@pytest.fixture(scope="module")
def golden():
    """per k: the dict of the golden database, its arrays, the golden reads' sequences (one reference for every test below)"""
    out = {}
    for k, name in GOLDEN_DBS.items():
        dct, db = ku.golden_dict(name)
        out[k] = dict(dct=dct, db=db, seqs=ku.sequences(ku.golden_reads(k)))
    return out


# ---- the kernel alone, every layout, the golden databases ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", list(GOLDEN_DBS))
def test_kernel_equals_the_restatement_on_the_golden_databases(golden, k, layout):
    """registers and hits byte-equal to the restatement; sum(hits) = the sum of the query kernels' result rows; 1, 63, 64, 65 and
    257 reads; a second call leaves the registers and doubles the hits; reads whose result row is zeroed add nothing"""
    from cuclark_amd import MiClarkDB
    g = golden[k]
    base = g["seqs"]
    seqs = [base[i % len(base)] for i in range(257)]
    rp, cont = _pack(_fasta(seqs), k)
    assert rp.size - 1 == 257
    with MiClarkDB(k, T6, layout=LAYOUTS[layout]) as e:
        e.read_arrays(gu.golden_sizes(g["db"]), g["db"]["ky"], g["db"]["lb"])
        d = Dev(e, rp, cont, T6)
        res = d.results()
        for n in (1, 63, 64, 65, 257):
            d.d_regs.zero_(); d.d_hits.zero_()
            got = d.add(n)
            want = ku.reads_sketch(g["dct"], seqs[:n], k, T6)
            _same(got, want, (k, layout, n))
            assert int(got[1].sum()) == int(res[:n, 0].astype(np.int64).sum()), (k, layout, n)      # the invariant across kernels
            assert (want[2] == res[:n, 0]).all()
        assert int(want[1].sum()) > 1000 and int(np.count_nonzero(want[1])) >= 3
        again = d.add()                                 # accumulation: max and sum
        assert (again[0] == want[0]).all() and (again[1] == 2 * want[1]).all()
        # early exit: rows zeroed -> those reads add nothing
        off = [r for r in range(257) if r % 3 == 0]
        d.zero_rows(off)
        d.d_regs.zero_(); d.d_hits.zero_()
        _same(d.add(), ku.reads_sketch(g["dct"], [s for r, s in enumerate(seqs) if r % 3], k, T6), (k, layout, "early exit"))
        d.zero_rows(list(range(257)))
        d.d_regs.zero_(); d.d_hits.zero_()
        none = d.add()
        assert int(none[1].sum()) == 0 and int(none[0].max()) == 0


@pytest.mark.gpu
def test_kernel_on_the_full_database_and_under_contention(golden):
    """db_full_k31_u32 (HTSIZE 1 610 612 741, 32-bit keys) with the golden reads; then 70 000 copies of one read, all raising one set of
    registers: the registers of one copy, 70 000 times its hits"""
    from cuclark_amd import MiClarkDB
    k = 31
    dct, db = ku.golden_dict("full_k31_u32")
    seqs = golden[k]["seqs"]
    with MiClarkDB(k, T6) as e:
        e.read_arrays(gu.golden_sizes(db), db["ky"], db["lb"])
        rp, cont = _pack(_fasta(seqs), k)
        d = Dev(e, rp, cont, T6)
        want = ku.reads_sketch(dct, seqs, k, T6)
        _same(d.add(), want, "full")
        assert int(want[1].sum()) == int(d.results()[:, 0].astype(np.int64).sum()) > 1000
        one = next(s for s in seqs if ku.reads_sketch(dct, [s], k, T6)[2][0] > 50)
        w1 = ku.reads_sketch(dct, [one], k, T6)
        rp, cont = _pack(_fasta([one] * 70_000), k)
        d = Dev(e, rp, cont, T6)
        got = d.add()
        assert (got[0] == w1[0]).all() and (got[1] == w1[1] * np.uint64(70_000)).all()


# ---- hand-made reads against an 8-target table ------------------------------------------------------------------------------------
def _hand_db(k, htsize=57777779):
    rng = np.random.default_rng(800 + k)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    genomes = [rnd(600) for _ in range(8)]
    genomes[7] = genomes[7][:300] + b"ACGT" * 15 + b"AT" * 25 + genomes[7][300:540]        # microsatellites: palindromes at even k
    km = [ku.seq_kmers(g, k) for g in genomes]
    canon = ku.canonical_np(np.concatenate(km), k)
    lab = np.concatenate([np.full(v.size, t, np.int64) for t, v in enumerate(km)])
    canon, first = np.unique(canon, return_index=True)
    lab = lab[first]
    order = np.lexsort((canon // np.uint64(htsize), canon % np.uint64(htsize)))
    canon, lab = canon[order], lab[order]
    sizes = np.bincount((canon % np.uint64(htsize)).astype(np.int64), minlength=htsize).astype(np.uint8)
    keys = canon // np.uint64(htsize)
    keys = keys.astype(np.uint32 if int(keys.max()) < (1 << 32) else np.uint64)
    so = np.argsort(canon)
    return genomes, (sizes, keys, lab.astype(np.uint16)), (canon[so], lab[so] + 1), rnd


def _rc(s):
    return s[::-1].translate(_COMP)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", [20, 31])
def test_kernel_on_hand_made_reads(k, layout):
    from cuclark_amd import MiClarkDB
    genomes, (sizes, keys, labels), dct, rnd = _hand_db(k)
    g0, g1 = genomes[0], genomes[1]
    every = bytearray(g1[:150])
    for i in range(k - 1, 150, k):
        every[i] = ord("N")                                    # runs of k - 1 nucleotides: no k-mer
    three = bytearray(g1[200:330])
    three[7:10] = b"NNN"                                       # the end of the first container and the start of the second
    long_read = b"".join(genomes)[:4800] + rnd(200)            # 5 000 nt, all eight targets, 78 rounds of 64 positions
    fwd = genomes[3][50:250]
    micro = b"ACGT" * 30
    reads = {
        "exactly k": g0[100:100 + k], "k - 1": g0[100:100 + k - 1], "an N every k - 1 bases": bytes(every), "N at 7, 8, 9": bytes(three),
        "5 000 nt": long_read, "forward": fwd, "reverse complement": _rc(fwd), "microsatellite": micro, "AT repeat": b"AT" * 40,
        "random": rnd(150),
    }
    assert len(long_read) == 5000
    names, seqs = list(reads), list(reads.values())
    with MiClarkDB(k, 8, layout=LAYOUTS[layout]) as e:
        e.read_arrays(sizes, keys, labels)
        rp, cont = _pack(_fasta(seqs), k)
        d = Dev(e, rp, cont, 8)
        want = ku.reads_sketch(dct, seqs, k, 8)
        _same(d.add(), want, (k, layout))
        res = d.results()
        assert (want[2] == res[:, 0]).all(), (names, want[2], res[:, 0])
        per = dict(zip(names, want[2]))
        assert per["exactly k"] == 1 and per["k - 1"] == 0 and per["an N every k - 1 bases"] == 0 and per["random"] == 0
        assert per["N at 7, 8, 9"] == 130 - 10 - k + 1 and per["5 000 nt"] >= 8 * (600 - k + 1) - 200 and int(np.count_nonzero(want[1])) == 8
        assert per["forward"] == per["reverse complement"] == 200 - k + 1 and per["microsatellite"] == 120 - k + 1
        # each read alone; a read and its reverse complement give the same registers
        alone = {}
        for name in ("exactly k", "forward", "reverse complement", "microsatellite", "5 000 nt"):
            rp1, ct1 = _pack(_fasta([reads[name]]), k)
            alone[name] = Dev(e, rp1, ct1, 8).add()
            _same(alone[name], ku.reads_sketch(dct, [reads[name]], k, 8), (k, layout, name))
        assert (alone["forward"][0] == alone["reverse complement"][0]).all() and (alone["forward"][1] == alone["reverse complement"][1]).all()
        assert int(np.count_nonzero(alone["exactly k"][0])) == 1
        if k == 20:      # (ACGT)n has four 20-mers, two of them palindromes, the other two each other's reverse complement: 3 registers
            assert int(np.count_nonzero(alone["microsatellite"][0])) == 3 and int(alone["microsatellite"][1][7]) == 101


# ---- the engine: ingest batches, the batch API -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("masks", ["plain", "masked"])
def test_engine_sketches_over_ingest_batches(golden, masks):
    """three batches of the golden FASTQ: the fetch equals the stand-alone call on ingest_fetch_packed and the restatement on the text
    (masked bases written as N), with and without MIC_INGEST_NO_CSV; a batch handed back adds nothing; a group of engines is refused"""
    from cuclark_amd import MiClarkDB, host
    from cuclark_amd._lib import MicError
    k = 31
    g = golden[k]
    text = open(os.path.join(gu.GOLDEN, "reads_k31.fq"), "rb").read()
    # (the golden reads are random text: six of them again with a homopolymer in the middle, for the low-complexity mask to find)
    for i, s in enumerate(ku.sequences(text)[:6]):
        s = s[:60] + b"A" * 40 + s[60:]
        text += b"@lowc%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n"
    lines = text.split(b"\n")
    n_rec = len(lines) // 4
    cuts = [0, n_rec // 3, 2 * n_rec // 3, n_rec]
    batches = [b"\n".join(lines[4 * a:4 * b]) + b"\n" for a, b in zip(cuts, cuts[1:])]
    names = gu.target_names()
    with MiClarkDB(k, T6) as e, MiClarkDB(k, T6) as e2:
        e.read_arrays(gu.golden_sizes(g["db"]), g["db"]["ky"], g["db"]["lb"])
        e.ingest_alloc(1, 256 << 10, names, want_results=True)
        with pytest.raises(MicError) as err:            # not started: nothing was allocated, nothing to fetch
            e.ksketch_fetch()
        assert err.value.code == -5
        seen = text
        if masks == "masked":
            e.ingest_set_min_quality(2)
            e.ingest_set_low_complexity(20)
            by_quality = host.mask_quality(text, 2)
            seen = host.mask_low_complexity(by_quality, 20)
            assert seen.count(b"N") >= by_quality.count(b"N") + 6 * 40 and by_quality.count(b"N") > text.count(b"N") + 100
        want = ku.reads_sketch(g["dct"], ku.sequences(bytes(seen)), k, T6)
        assert int(want[1].sum()) > 500
        for csv in (True, False):
            e.ksketch_start()
            alone = None
            for b in batches:
                out = e.ingest_classify(0, b, csv=csv)
                assert out["status"] == 0 and (out["csv"] != b"") == csv
                rp, ct = e.ingest_fetch_packed(0)
                d = Dev(e, rp, ct, T6)
                assert (d.results()[:, :5] == out["results"][:, :5]).all()
                if alone is not None:
                    d.d_regs.copy_(alone.d_regs); d.d_hits.copy_(alone.d_hits)
                d.add()
                alone = d
            got = e.ksketch_fetch()
            _same(got, (alone.d_regs.cpu().numpy().reshape(T6, ku.M), alone.d_hits.cpu().numpy().view(np.uint64)), (masks, csv, "stand-alone"))
            _same(got, want, (masks, csv, "restatement"))
        # a batch that is handed back (an odd record: the empty name) leaves the sketches untouched
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + batches[0]
        out = e.ingest_classify(0, bad, csv=False)
        assert out["status"] & 1
        _same(e.ksketch_fetch(), want, "handed back")
        # the table-sharded mode is refused while started
        with pytest.raises(MicError) as err:
            MiClarkDB.ingest_classify_group([e, e2], 0, 0, batches[0])
        assert err.value.code == -7                     # MIC_E_UNSUPPORTED
        # stopped: the sketches keep their values; started again: zeroed
        e.ksketch_stop()
        assert e.ingest_classify(0, batches[0], csv=False)["status"] == 0
        _same(e.ksketch_fetch(), want, "stopped")
        e.ksketch_start()
        z = e.ksketch_fetch()
        assert int(z[0].max()) == 0 and int(z[1].sum()) == 0
        assert e.L.mic_ksketch_fetch(e.h, z[0].ctypes.data, 8, z[1].ctypes.data, z[1].size) == -1      # MIC_E_INVALID: the sizes are the engine's


@pytest.mark.gpu
def test_batch_api_adds_to_the_engine_sketches(golden):
    from cuclark_amd import MiClarkDB
    from cuclark_amd._lib import MicError
    k = 27
    g = golden[k]
    rp, cont = _pack(_fasta(g["seqs"]), k)
    n = rp.size - 1
    with MiClarkDB(k, T6) as e:
        e.read_arrays(gu.golden_sizes(g["db"]), g["db"]["ky"], g["db"]["lb"])
        bufs = e.malloc(n, n, cont.size, [0, n])
        bufs["reads_pointer"][0][: n + 1] = rp
        bufs["containers"][0][: cont.size] = cont
        e.readyBatch(0, n, cont.size)
        e.queryBatch(0)
        e.waitForBatch(0)
        with pytest.raises(MicError) as err:
            e.batch_ksketch(0)
        assert err.value.code == -5                     # not started
        e.ksketch_start()
        e.batch_ksketch(0)
        want = ku.reads_sketch(g["dct"], g["seqs"], k, T6)
        _same(e.ksketch_fetch(), want, "batch API")
        assert int(want[1].sum()) == int(bufs["results"][:, 0].astype(np.int64).sum()) > 500
        e.freeBatchMemory()


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _parse(report):
    lines = report.splitlines()
    assert lines[0] == "Name,Reads,Kmers,DistinctKmers,Duplication"
    return {f[0]: (int(f[1]), int(f[2]), int(f[3]), f[4]) for f in (ln.split(",") for ln in lines[1:])}


@pytest.fixture(scope="module")
def cli_db(tmp_path_factory):
    """the golden k = 31 database laid out for the command line, once for the three cases"""
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path_factory.mktemp("kmer_report_db"))
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["fq", "fa", "pairs"])
def test_cli_kmer_report(tmp_path, cli_db, inp):
    """every route of one input writes the same bytes: -n 1, -n 4, --extended (the batch API), the host path, a compressed file, with
    and without -R; Kmers and Reads equal the restatement and --abundance, DistinctKmers is within 1 of the Python estimator"""
    tmp = str(tmp_path)
    t, dbd = cli_db
    o = lambda n: os.path.join(tmp, n)
    env = {"MIC_INGEST_KB": "64"}
    gz = lambda src, dst: gzip.open(dst, "wb").write(open(src, "rb").read())
    if inp == "pairs":
        f1, f2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
        gz(f1, o("p1.fq.gz")); gz(f2, o("p2.fq.gz"))
        plain, packed = ["-P", f1, f2], ["-P", o("p1.fq.gz"), o("p2.fq.gz")]
        seqs = ku.sequences(gu.merge_pairs(open(f1, "rb").read(), open(f2, "rb").read()))
    else:
        f = os.path.join(gu.GOLDEN, f"reads_k31.{inp}")
        gz(f, o(f"in.{inp}.gz"))
        plain, packed = ["-O", f], ["-O", o(f"in.{inp}.gz")]
        seqs = ku.sequences(open(f, "rb").read())
    base = [EXE, "-k", "31", "-T", t, "-D", dbd]
    routes = {"n1": (plain + ["-n", "1", "-R", o("r_n1")], env), "n4": (plain + ["-n", "4", "-R", o("r_n4")], env),
              "extended": (plain + ["--extended", "-R", o("r_ext")], env)}
    if inp != "fa":
        routes["gz"] = (packed + ["-n", "4", "-R", o("r_gz")], env)
    if inp == "fq":
        routes.update({"host": (plain + ["-R", o("r_host")], {"MIC_HOST_INGEST": "1"}), "summary": (plain + ["-n", "4"], env), "summary_gz": (packed, env)})
    reports = {}
    for name, (args, ev) in routes.items():
        r = _run(base + args + ["--kmer-report", o(f"k_{name}.csv")], ev)
        assert r.returncode == 0 and "K-mer report stored" in r.stdout, (name, r.stderr)
        reports[name] = open(o(f"k_{name}.csv")).read()
        assert ("Results stored" in r.stdout) == (not name.startswith("summary")), name
    for name, rep in reports.items():
        assert rep == reports["n1"], name
    # the result CSV does not change with the option; --abundance next to it gives the same Reads
    r = _run(base + plain + ["-n", "1", "-R", o("r0"), "--abundance", o("a.csv")], env)
    assert r.returncode == 0, r.stderr
    assert open(o("r0.csv"), "rb").read() == open(o("r_n1.csv"), "rb").read()
    ab = {ln.split(",")[0]: int(ln.split(",")[3]) for ln in open(o("a.csv")).read().splitlines()[1:] if ln.split(",")[0] != "UNKNOWN"}
    dct, _ = ku.golden_dict("full_k31_u32")
    names = gu.target_names()
    regs, hits, _ = ku.reads_sketch(dct, seqs, 31, len(names))
    got = _parse(reports["n1"])
    assert list(got) == [nm for t_, nm in enumerate(names) if int(hits[t_])] and len(got) >= 3
    for t_, nm in enumerate(names):
        if not int(hits[t_]):
            continue
        reads, kmers, distinct, dup = got[nm]
        assert kmers == int(hits[t_]) and reads == ab.get(nm, 0), nm
        assert abs(distinct - ku.distinct(regs[t_], kmers)) <= 1, nm
        assert dup == ku.ratio_text(kmers, distinct)
    if inp != "fq":
        return
    # a stricter filter changes Reads, nothing else
    r = _run(base + plain + ["--kmer-report", o("k_hc.csv"), "--min-confidence", "1"], env)
    assert r.returncode == 0, r.stderr
    hc = _parse(open(o("k_hc.csv")).read())
    assert {n_: v[1:] for n_, v in hc.items()} == {n_: v[1:] for n_, v in got.items()}
    assert sum(v[0] for v in hc.values()) <= sum(v[0] for v in got.values())
