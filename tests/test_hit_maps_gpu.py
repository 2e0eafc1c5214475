"""Hit maps on the MI355X: hitmap_kernel (mic_hitmap_device on torch tensors) against the Python restatement of tests/hitmap_util.py - a
dict of canonical k-mer -> label from the arrays the table was loaded from, a walk over the reads' text, itertools.groupby - on every
table layout, word for word; the engine's maps and text over ingest batches; the batch API; exe/cuCLARK --hit-maps on every input
route.  Every comparison is equality.

Two facts about the golden data, found while writing this file (figures from the restatement):
  * the four golden databases light_k20_u16 / light_k27_u32 / light_k31_u64 / light_k32_u64 hold EVERY k-mer of their targets, so
    their reads' maps are at most 6 words long; the golden database whose maps are many one-k-mer runs is the gap-sampled
    lightgap1_k20_u16 (every other k-mer: a read of 118 words).  The kernel test runs it as a fifth database and asserts the "more
    than 30 words" there.
  * for the same reason the golden k = 27 light database cannot outgrow a 64 KiB slot's first word buffer (172 words in 19 KB of
    FASTQ); the small-slot test runs it AND lightgap1_k20_u16, whose batch needs several times the first allocation of both buffers."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import hitmap_util as hu
import ksketch_util as ku
from test_kmer_report_gpu import GOLDEN_DBS, LAYOUTS, T6, _fasta, _hand_db, _pack, _rc

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
KERNEL_DBS = dict({name: k for k, name in GOLDEN_DBS.items()}, lightgap1_k20_u16=20)
SENTINEL = 0x5A5A5A5A


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=300, env=e, **kw)


class Dev:
    """packed reads on the device, their result rows and sparse rows from query_device + resolve_flagged_device"""

    def __init__(self, e, rp, cont):
        import torch
        self.e, self.n = e, rp.size - 1
        dev = torch.device("cuda:0")
        self.d_rp = torch.from_numpy(np.ascontiguousarray(rp, np.uint32).view(np.int32)).to(dev)
        self.d_ct = torch.from_numpy(np.concatenate([cont, np.zeros(64, np.uint16)]).view(np.int16)).to(dev)
        self.d_res = torch.zeros((self.n, 8), dtype=torch.int32, device=dev)
        self.d_rows = torch.zeros((self.n, e.row_words), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.query_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), self.n, self.d_res.data_ptr(), self.d_rows.data_ptr())
        e.resolve_flagged_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), self.d_res.data_ptr(), self.d_rows.data_ptr())
        e.sync()

    def results(self):
        return self.d_res.cpu().numpy().view(np.uint32)

    def rows(self):
        return self.d_rows.cpu().numpy().view(np.uint32)

    def zero_rows(self, rows):
        import torch
        self.d_res[torch.from_numpy(np.asarray(rows, np.int64)).to(self.d_res.device)] = 0
        torch.cuda.synchronize()

    def size(self, n):
        """first call: d_words null -> (offsets, total)"""
        import torch
        d_off = torch.full((n + 1,), -1, dtype=torch.int32, device=self.d_res.device)
        torch.cuda.synchronize()
        total = self.e.hitmap_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), n, self.d_res.data_ptr(), d_off.data_ptr())
        return d_off.cpu().numpy().view(np.uint32), total

    def fill(self, n, total, cap):
        """second call with cap words: (offsets, the buffer of total + 8 words that was full of SENTINEL, the total it returns)"""
        import torch
        d_off = torch.full((n + 1,), -1, dtype=torch.int32, device=self.d_res.device)
        d_words = torch.full((total + 8,), SENTINEL, dtype=torch.int32, device=self.d_res.device)
        torch.cuda.synchronize()
        got = self.e.hitmap_device(self.d_rp.data_ptr(), self.d_ct.data_ptr(), n, self.d_res.data_ptr(), d_off.data_ptr(), d_words.data_ptr(), cap)
        return d_off.cpu().numpy().view(np.uint32), d_words.cpu().numpy().view(np.uint32), got

    def maps(self, n=None):
        n = self.n if n is None else n
        off, total = self.size(n)
        off2, buf, got = self.fill(n, total, total)
        assert got == total == int(off[-1]) and (off == off2).all()
        assert (buf[total:] == SENTINEL).all(), "words behind the total were written"
        return off, buf[:total]


def _same(got, want, what=""):
    assert got[0].tolist() == want[0].tolist(), (what, "offsets")
    bad = np.flatnonzero(got[1] != want[1])
    assert bad.size == 0, (what, bad[:5], [hex(int(x)) for x in got[1][bad[:5]]], [hex(int(x)) for x in want[1][bad[:5]]])


def _check_invariants(off, words, res, rows, seqs, k, n_targets, what):
    """per read: labelled k-mers = result word 0; per target = the sparse row's count; all k-mers = the parts' positions"""
    hit, per, tot = hu.sums(off, words, n_targets)
    n = off.size - 1
    assert (hit == res[:n, 0]).all(), what
    for r in range(n):
        assert int(tot[r]) == sum(p.size - k + 1 for p in hu.parts_of(seqs[r], k)), (what, r)
        row = rows[r]
        assert int(row[0]) != 0xFFFFFFFF
        sparse = np.zeros(n_targets, np.int64)
        for w in row[1:1 + int(row[0])]:
            sparse[int(w) & 0xFFFF] = int(w) >> 16
        assert (per[r] == sparse).all(), (what, r, per[r], sparse)


@pytest.fixture(scope="module")
def golden():
    """per database: its dict, its arrays, 257 reads (the golden reads repeated), their maps by the restatement - one reference for all layouts"""
    out = {}
    for name, k in KERNEL_DBS.items():
        dct, db = ku.golden_dict(name)
        base = ku.sequences(ku.golden_reads(k))
        seqs = [base[i % len(base)] for i in range(257)]
        out[name] = dict(k=k, dct=dct, db=db, seqs=seqs, want=hu.batch(dct, seqs, k, T6))
    return out


# ---- the kernel alone, every layout, the golden databases ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(KERNEL_DBS))
def test_kernel_equals_the_restatement_on_the_golden_databases(golden, name, layout):
    """offsets and words equal to the restatement for 1, 63, 64, 65 and 257 reads; the three invariants against the query kernels'
    result rows and sparse rows; zeroed result rows give 0:nk maps; the two-call sizing"""
    from cuclark_amd import MiClarkDB
    g = golden[name]
    k, seqs = g["k"], g["seqs"]
    w_off, w_words = g["want"]
    rp, cont = _pack(_fasta(seqs), k)
    assert rp.size - 1 == 257
    with MiClarkDB(k, T6, layout=LAYOUTS[layout]) as e:
        e.read_arrays(gu.golden_sizes(g["db"]), g["db"]["ky"], g["db"]["lb"])
        d = Dev(e, rp, cont)
        res, rows = d.results(), d.rows()
        for n in (1, 63, 64, 65, 257):
            got = d.maps(n)
            _same(got, (w_off[:n + 1], w_words[:int(w_off[n])]), (name, layout, n))
            _check_invariants(got[0], got[1], res, rows, seqs, k, T6, (name, layout, n))
        per_read = np.diff(w_off.astype(np.int64))
        assert int(per_read.max()) <= 6 or name.startswith("lightgap")
        if name.startswith("lightgap"):
            assert int(per_read.max()) > 30                 # many one-k-mer runs: every other k-mer of the targets is in the table
        assert int(np.count_nonzero(w_words >> 16)) >= 100
        # the two-call sizing: d_words null, then the exact capacity, then one word less - which leaves d_words untouched
        off0, total = d.size(257)
        assert total == int(w_off[-1]) and off0.tolist() == w_off.tolist()
        off1, buf, got_total = d.fill(257, total, total - 1)
        assert got_total == total and off1.tolist() == w_off.tolist() and (buf == SENTINEL).all()
        # rows zeroed -> those reads are not probed: 0:nk per part, straight from the part headers
        off_rows = [r for r in range(257) if r % 3 == 0]
        d.zero_rows(off_rows)
        zero = lambda s: hu.rle_words([[0] * (p.size - k + 1) for p in hu.parts_of(s, k)], T6)
        per = [zero(s) if r % 3 == 0 else w_words[int(w_off[r]):int(w_off[r + 1])].tolist() for r, s in enumerate(seqs)]
        want = (np.cumsum([0] + [len(p) for p in per]).astype(np.uint32), np.array([x for p in per for x in p], np.uint32))
        _same(d.maps(), want, (name, layout, "zeroed rows"))


# ---- hand-made reads against an 8-target table ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", [20, 31])
def test_kernel_on_hand_made_reads(k, layout):
    from cuclark_amd import MiClarkDB, host
    genomes, (sizes, keys, labels), dct, rnd = _hand_db(k)
    g0, g1 = genomes[0], genomes[1]
    reads = {}
    # chimeras: the k-mers of g0[a:a+x] are target 1 (positions 0 .. x - k), the k - 1 that span the junction are nothing, from position
    # x on target 2 - label boundaries at x - k + 1 and at x
    def chimera(x):
        """g0[50:50 + x] + 100 nt of g1, joined where neither genome goes on as the other does: no spanning k-mer is in a target"""
        s = next(s for s in range(70, 200) if g1[s] != g0[50 + x] and g1[s - 1] != g0[50 + x - 1])
        return g0[50:50 + x] + g1[s:s + 100]
    reads["chimera 100 + 100"] = chimera(100)
    for b in (63, 64, 65):
        reads[f"chimera, second boundary at {b}"] = chimera(b)
        reads[f"chimera, first boundary at {b}"] = chimera(b + k - 1)
    for nk in (63, 64, 65, 128, 129):
        reads[f"one run of {nk}"] = g0[200:200 + nk + k - 1]
    every = bytearray(g1[:150])
    for i in range(k - 1, 150, k):
        every[i] = ord("N")                                    # runs of k - 1 nucleotides: no k-mer
    three = bytearray(g1[200:330])
    three[7:10] = b"NNN"                                       # the end of the first container and the start of the second
    both = bytearray(genomes[2][100:300])
    both[90] = ord("N")                                        # the same target on both sides of an N: a separator, no merge
    fwd = genomes[3][50:150] + rnd(40) + genomes[4][10:120]
    long_read = b"".join(genomes)[:4800] + rnd(200)            # 5 000 nt, all eight targets, 78 rounds of 64 positions
    reads.update({"exactly k": g0[100:100 + k], "k - 1": g0[100:100 + k - 1], "an N every k - 1 bases": bytes(every), "N at 7, 8, 9": bytes(three),
                  "one target around an N": bytes(both), "forward": fwd, "reverse complement": _rc(fwd), "5 000 nt": long_read, "random": rnd(150)})
    assert len(long_read) == 5000
    names, seqs = list(reads), list(reads.values())
    want = hu.batch(dct, seqs, k, 8)
    words_of = lambda nm: want[1][int(want[0][names.index(nm)]):int(want[0][names.index(nm) + 1])].tolist()
    w = lambda l, n: (l << 16) | n
    # what the restatement says about the reads, so that the cases are what their names say
    for b in (63, 64, 65):
        assert words_of(f"chimera, second boundary at {b}") == [w(1, b - k + 1), w(0, k - 1), w(2, 100 - k + 1)]
        assert words_of(f"chimera, first boundary at {b}") == [w(1, b), w(0, k - 1), w(2, 100 - k + 1)]
    assert words_of("chimera 100 + 100") == [w(1, 101 - k), w(0, k - 1), w(2, 101 - k)]
    for nk in (63, 64, 65, 128, 129):
        assert words_of(f"one run of {nk}") == [w(1, nk)]
    assert words_of("exactly k") == [w(1, 1)] and words_of("k - 1") == [] and words_of("an N every k - 1 bases") == []
    assert words_of("N at 7, 8, 9") == [w(2, 130 - 10 - k + 1)] and words_of("random") == [w(0, 150 - k + 1)]
    assert words_of("one target around an N") == [w(3, 90 - k + 1), 0, w(3, 109 - k + 1)]
    assert words_of("reverse complement") == words_of("forward")[::-1] and len(words_of("forward")) == 3      # each other's mirror
    assert len({x >> 16 for x in words_of("5 000 nt")} - {0}) == 8
    with MiClarkDB(k, 8, layout=LAYOUTS[layout]) as e:
        e.read_arrays(sizes, keys, labels)
        rp, cont = _pack(_fasta(seqs), k)
        d = Dev(e, rp, cont)
        got = d.maps()
        _same(got, want, (k, layout))
        _check_invariants(got[0], got[1], d.results(), d.rows(), seqs, k, 8, (k, layout))
        # each read alone (another wave, another offset)
        for nm in ("chimera, first boundary at 64", "one run of 129", "reverse complement", "5 000 nt", "k - 1"):
            rp1, ct1 = _pack(_fasta([reads[nm]]), k)
            off1, w1 = Dev(e, rp1, ct1).maps()
            assert off1.tolist() == [0, len(words_of(nm))] and w1.tolist() == words_of(nm), nm
        # one read of 70 000 nt through host.pack_reads: the packer cuts it into two overlapping sub-parts
        big = (b"".join(genomes) * 15)[:70000]
        text = b">big\n" + big + b"\n"
        idx = host.index_reads(text)
        rpb, ctb = host.pack_reads(text, idx["seq_s"], idx["seq_e"], idx["length"], k)
        wantb = hu.batch(dct, [big], k, 8)
        assert int(np.count_nonzero(wantb[1] == 0)) == 1 and len(hu.parts_of(big, k)) == 2
        db_ = Dev(e, rpb, ctb)
        gotb = db_.maps()
        _same(gotb, wantb, (k, layout, "70 000 nt"))
        assert sum(int(x) & 0xFFFF for x in gotb[1]) == 70000 - k + 1
        assert int(hu.sums(gotb[0], gotb[1], 8)[0][0]) == int(db_.results()[0, 0])


# ---- the engine: ingest batches, the batch API -----------------------------------------------------------------------------------
def _batches_of(text, n):
    lines = text.split(b"\n")
    n_rec = len(lines) // 4
    cuts = [n_rec * i // n for i in range(n + 1)]
    return [b"\n".join(lines[4 * a:4 * b]) + b"\n" for a, b in zip(cuts, cuts[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("masks", ["plain", "masked"])
def test_engine_maps_over_ingest_batches(masks):
    """three batches of the golden FASTQ: the text equals the restatement on the text (masked bases written as N), with and without
    MIC_INGEST_NO_CSV; a batch handed back leaves none; a group of engines is refused; after stop nothing is produced"""
    from cuclark_amd import MiClarkDB, host
    from cuclark_amd._lib import MicError
    k = 31
    dct, db = ku.golden_dict(GOLDEN_DBS[k])
    text = open(os.path.join(gu.GOLDEN, "reads_k31.fq"), "rb").read()
    # (the golden reads are random text: six of them again with a homopolymer in the middle, for the low-complexity mask to find)
    for i, s in enumerate(ku.sequences(text)[:6]):
        s = s[:60] + b"A" * 40 + s[60:]
        text += b"@lowc%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n"
    names = gu.target_names()
    with MiClarkDB(k, T6) as e, MiClarkDB(k, T6) as e2:
        e.read_arrays(gu.golden_sizes(db), db["ky"], db["lb"])
        e.ingest_alloc(1, 256 << 10, names, want_results=True)
        seen = text
        if masks == "masked":
            e.ingest_set_min_quality(2)
            e.ingest_set_low_complexity(20)
            seen = bytes(host.mask_low_complexity(host.mask_quality(text, 2), 20))
            assert seen.count(b"N") >= text.count(b"N") + 6 * 40 + 100
        batches, seen_batches = _batches_of(text, 3), _batches_of(seen, 3)
        assert e.ingest_classify(0, batches[0], csv=False)["status"] == 0
        with pytest.raises(MicError) as err:            # not started: nothing was made
            e.ingest_hitmap_text(0)
        assert err.value.code == -5
        e.hitmap_start()
        plain_csv = []
        for csv in (True, False):
            for b, sb in zip(batches, seen_batches):
                out = e.ingest_classify(0, b, csv=csv)
                assert out["status"] == 0 and (out["csv"] != b"") == csv
                got = e.ingest_hitmap_text(0)
                want = hu.text_of(dct, sb, k, names)
                assert got == want, (masks, csv)
                assert got.count(b"\n") == out["n_reads"]
                if csv:
                    plain_csv.append(out["csv"])
        assert b" " in want and b":" in want
        # a batch that is handed back (an odd record: the empty name) leaves no text
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + batches[0]
        assert e.ingest_classify(0, bad, csv=False)["status"] & 1
        with pytest.raises(MicError) as err:
            e.ingest_hitmap_text(0)
        assert err.value.code == -5                     # MIC_E_STATE
        # the table-sharded mode is refused while started
        with pytest.raises(MicError) as err:
            MiClarkDB.ingest_classify_group([e, e2], 0, 0, batches[0])
        assert err.value.code == -7                     # MIC_E_UNSUPPORTED
        # stopped: nothing is produced, the CSV is what it was
        e.hitmap_stop()
        out = e.ingest_classify(0, batches[0])
        assert out["status"] == 0 and out["csv"] == plain_csv[0]
        with pytest.raises(MicError) as err:
            e.ingest_hitmap_text(0)
        assert err.value.code == -5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["light_k27_u32", "lightgap1_k20_u16"])
def test_a_small_slot_grows_its_buffers(name):
    """a slot allocated at 64 KiB: its first word buffer holds 64 KiB / 64 = 1024 words (allocated: 1536), its first text buffer 16 KiB (20);
    the gap-sampled database's batch needs several times both, the batches before and after it do not"""
    from cuclark_amd import MiClarkDB
    k = KERNEL_DBS[name]
    dct, db = ku.golden_dict(name)
    recs = ku.golden_reads(k)
    if recs[:1] == b">":       # the k = 20 reads are FASTA
        seqs = ku.sequences(recs)
        rec = lambda i, j: b">r%d_%d\n" % (j, i) + seqs[i] + b"\n"
        n_rec = len(seqs)
    else:
        lines = recs.split(b"\n")
        rec = lambda i, j: b"@r%d_%d\n" % (j, i) + b"\n".join(lines[4 * i + 1:4 * i + 4]) + b"\n"
        n_rec = len(lines) // 4
    big = b"".join(rec(i, j) for j in range(3) for i in range(n_rec))
    small = b"".join(rec(i, 9) for i in range(5))
    assert len(big) < (64 << 10) - 4096
    names = gu.target_names()
    want_big, want_small = hu.text_of(dct, big, k, names), hu.text_of(dct, small, k, names)
    n_words = int(hu.batch(dct, ku.sequences(big), k, T6)[0][-1])
    if name.startswith("lightgap"):
        assert n_words > 2 * 1536 and len(want_big) > 20 << 10
    with MiClarkDB(k, T6) as e:
        e.read_arrays(gu.golden_sizes(db), db["ky"], db["lb"])
        e.ingest_alloc(1, 64 << 10, names)
        e.hitmap_start()                                 # started behind the allocation: the buffers come with the first batch
        for data, want in ((small, want_small), (big, want_big), (small, want_small), (big, want_big)):
            assert e.ingest_classify(0, data)["status"] == 0
            assert e.ingest_hitmap_text(0) == want
        e.ingest_free()
        e.ingest_alloc(1, 64 << 10, names)               # started by the allocation: the buffers come with the slots
        assert e.ingest_classify(0, big, csv=False)["status"] == 0
        assert e.ingest_hitmap_text(0) == want_big


@pytest.mark.gpu
def test_batch_api_equals_the_stand_alone_call():
    from cuclark_amd import MiClarkDB
    k = 27
    dct, db = ku.golden_dict(GOLDEN_DBS[k])
    seqs = ku.sequences(ku.golden_reads(k))
    rp, cont = _pack(_fasta(seqs), k)
    n = rp.size - 1
    with MiClarkDB(k, T6) as e:
        e.read_arrays(gu.golden_sizes(db), db["ky"], db["lb"])
        bufs = e.malloc(n, n, cont.size, [0, n])
        bufs["reads_pointer"][0][: n + 1] = rp
        bufs["containers"][0][: cont.size] = cont
        e.readyBatch(0, n, cont.size)
        e.queryBatch(0)
        e.waitForBatch(0)
        off, words = e.batch_hitmap(0, n)
        alone = Dev(e, rp, cont).maps()
        _same((off, words), alone, "batch API against the stand-alone call")
        _same((off, words), hu.batch(dct, seqs, k, T6), "batch API against the restatement")
        assert (hu.sums(off, words, T6)[0] == bufs["results"][:n, 0]).all() and int(off[-1]) > 100
        e.freeBatchMemory()


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_db(tmp_path_factory):
    """the golden k = 31 database laid out for the command line, once for the three cases"""
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path_factory.mktemp("hit_maps_db"))
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["fq", "fa", "pairs"])
def test_cli_hit_maps(tmp_path, cli_db, inp):
    """every route of one input writes the same bytes, equal to the restatement: -n 1, -n 4, --extended (the batch API), the host
    path, a compressed file, with and without -R; the result CSV does not change with the option"""
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
    if isinstance(text, str):
        text = text.encode()
    base = [EXE, "-k", "31", "-T", t, "-D", dbd]
    routes = {"n1": (plain + ["-n", "1", "-R", o("r_n1")], env), "n4": (plain + ["-n", "4", "-R", o("r_n4")], env),
              "extended": (plain + ["--extended", "-R", o("r_ext")], env)}
    if inp != "fa":
        routes["gz"] = (packed + ["-n", "4", "-R", o("r_gz")], env)
    if inp == "fq":
        routes.update({"host": (plain + ["-R", o("r_host")], {"MIC_HOST_INGEST": "1"}), "summary": (plain + ["-n", "4"], env), "summary_gz": (packed, env)})
    maps = {}
    for name, (args, ev) in routes.items():
        r = _run(base + args + ["--hit-maps", o(f"h_{name}.csv")], ev)
        assert r.returncode == 0 and f"Hit maps stored in {o(f'h_{name}.csv')}" in r.stdout, (name, r.stderr)
        maps[name] = open(o(f"h_{name}.csv"), "rb").read()
        assert ("Results stored" in r.stdout) == (not name.startswith("summary")), name
    dct, _ = ku.golden_dict("full_k31_u32")
    names = gu.target_names()
    want = hu.HEADER + hu.text_of(dct, text, 31, names)
    for name, got in maps.items():
        assert got == want, name
    assert want.count(b"\n") == len(ku.sequences(text)) + 1 and want.count(b":") > 100
    if inp == "pairs":
        assert want.count(b"|") >= 30                   # the mates are parts of the merged read
    # the result CSV does not change with the option
    r = _run(base + plain + ["-n", "1", "-R", o("r0")], env)
    assert r.returncode == 0, r.stderr
    assert open(o("r0.csv"), "rb").read() == open(o("r_n1.csv"), "rb").read()
