"""Abundance profile on the MI355X: the engine's device counters (mic_abundance_*) over ingest batches equal the counting rule
(csrc/mic_abund.h) applied to the result rows, with and without MIC_INGEST_NO_CSV, under every table layout; batches handed back
are counted once, by the host path; exe/cuCLARK --abundance equals exe/estimate_abundance on its own result CSV on every input
path, and a summary-only run (no -R) gives the same profile; mic_abundance_device on torch tensors."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as gu

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")
FILTERS = [("0.5", "0"), ("0.75", "0.03"), ("0.9", "0.5")]


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=600, env=e, **kw)


def _synth(T=4096, genome_nt=16_000_000, htsize=57777779, k=31, mosaic_ppm=0, seed=11):
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    spec = _lib.MicSynthSpec(seed=seed, htsize=htsize, genome_nt=genome_nt, n_targets=T, n_genomes=T, k=k, key_bytes=8,
                             mosaic_ppm=mosaic_ppm)
    cap = genome_nt + 1024
    d_sizes = torch.empty(htsize, dtype=torch.uint8, device=dev)
    d_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    d_labels = torch.empty(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    assert L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None) == 0
    torch.cuda.synchronize()
    return spec, d_sizes, d_keys[: n_el.value], d_labels[: n_el.value]


def _reads_text(spec, n_reads, read_len=150, seed=5, random_frac=0.2):
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    rb = int(L.mic_synth_text_record_bytes(read_len, 0))
    d_text = torch.empty(n_reads * rb + 64, dtype=torch.uint8, device="cuda:0")
    assert L.mic_synth_reads_text_device(C.byref(spec), seed, n_reads, read_len, random_frac, 0.01, 0.002, 0, -1, d_text.data_ptr(),
                                         d_text.numel(), None) == 0
    torch.cuda.synchronize()
    return d_text[: n_reads * rb].cpu().numpy().tobytes(), rb


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["direct", "minimizer", "super", "super2"])
def test_ingest_counters_equal_the_rule(layout):
    """4096 targets, 1 M reads in batches of ~1 MB: the device counters equal the rule on the returned result rows for several
    thresholds, and are identical with MIC_INGEST_NO_CSV (which returns the same rows and no text)."""
    from cuclark_amd import MiClarkDB, host
    ids = {"direct": 1, "minimizer": 2, "super": 3, "super2": 4}
    T, k, n_reads = 4096, 31, 1_000_000
    spec, d_sizes, d_keys, d_labels = _synth(T)
    text, rb = _reads_text(spec, n_reads)
    per = (1 << 20) // rb
    names = [f"L{i}" for i in range(T)]
    with MiClarkDB(k, T, layout=ids[layout]) as e:
        e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, 2 << 20, names, want_results=True)
        rows = None
        for c, g in FILTERS:
            got = {}
            for csv in (True, False):
                e.abundance_start(host.abund_filter(c, g))
                res_all = []
                for r0 in range(0, n_reads, per):
                    r1 = min(n_reads, r0 + per)
                    out = e.ingest_classify(0, text[r0 * rb:r1 * rb], csv=csv)
                    assert out["status"] == 0 and out["n_reads"] == r1 - r0
                    assert (out["csv"] != b"") == csv
                    res_all.append(out["results"])
                got[csv] = e.abundance_fetch()
                res = np.concatenate(res_all)
                if rows is None:
                    rows = res
                assert (res[:, :5] == rows[:, :5]).all()
            e.abundance_stop()
            want = host.abundance_host(rows, np.full(n_reads, 150, np.uint32), k, T, host.abund_filter(c, g))
            assert (got[True] == want).all() and (got[False] == want).all(), (layout, c, g)
            assert int(want.sum()) == n_reads and int((want[2:] > 0).sum()) > T // 2
        # fallback batches add nothing on the device: an odd record (empty name) sends the batch back
        e.abundance_start(host.abund_filter())
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + text[:rb * 100]
        out = e.ingest_classify(0, bad, csv=False)
        assert out["status"] & 1
        assert int(e.abundance_fetch().sum()) == 0


def _synth_db_files(tmp, spec, d_sizes, d_keys, d_labels, T):
    """The synthetic database as the command line's files: targets file (T labels on one dummy genome) and db_central_*.tsk.*"""
    d = os.path.join(tmp, "DB")
    os.makedirs(d, exist_ok=True)
    dummy = os.path.join(tmp, "dummy.fa")
    open(dummy, "w").write(">d\nACGT\n")
    t = os.path.join(tmp, "targets.txt")
    with open(t, "w") as f:
        for i in range(T):
            f.write(f"{dummy} L{i}\n")
    base = os.path.join(d, f"db_central_k{spec.k}_t{T}_s{spec.htsize}_m0.tsk")
    d_sizes.cpu().numpy().tofile(base + ".sz")
    d_keys.cpu().numpy().tofile(base + ".ky")
    d_labels.cpu().numpy().tofile(base + ".lb")
    return t, d


def _host_path_batches(stderr):
    """(batches, batches through the host path) from the MIC_CLI_TIMING line of the streaming path"""
    import re
    m = re.search(r"device ingest: (\d+) batches .*?, (\d+) through the host path", stderr)
    assert m, stderr
    return int(m.group(1)), int(m.group(2))


@pytest.mark.gpu
def test_fallback_batches_counted_once(tmp_path):
    """Reads of mosaic genome stretches hit more than 64 targets (dense path: their batches are handed back) while the other
    batches are counted on the device: the profile equals the -R run's CSV through estimate_abundance, the summary-only run and a
    MIC_HOST_INGEST=1 run, and its total is the number of objects.  An odd record (empty name) sends its batch back as well; the
    host path then reads the rest of that batch the way the reference does, and the profile still equals the CSV's."""
    tmp = str(tmp_path)
    T = 512
    spec, d_sizes, d_keys, d_labels = _synth(T, genome_nt=4_000_000, mosaic_ppm=500, seed=3)
    t, d = _synth_db_files(tmp, spec, d_sizes, d_keys, d_labels, T)
    text, rb = _reads_text(spec, 60000, read_len=300, random_frac=0.05)
    plain, odd = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "odd.fq")
    open(plain, "wb").write(text)
    with open(odd, "wb") as f:
        f.write(text[: rb * 30000])
        f.write(b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
        f.write(text[rb * 30000:])
    env = {"MIC_INGEST_KB": "256", "MIC_CLI_TIMING": "1"}
    for fq, host_too in ((plain, True), (odd, False)):
        base = [EXE, "-k", "31", "-T", t, "-D", d, "-O", fq, "--htsize", str(spec.htsize), "--min-confidence", "0.6"]
        r1 = _run(base + ["-R", os.path.join(tmp, "out"), "--abundance", os.path.join(tmp, "a1.csv")], env)
        assert r1.returncode == 0, r1.stderr
        nb, nh = _host_path_batches(r1.stderr)
        assert 0 < nh < nb, r1.stderr
        r2 = _run(base + ["--abundance", os.path.join(tmp, "a2.csv")], env)
        assert r2.returncode == 0, r2.stderr
        assert _host_path_batches(r2.stderr) == (nb, nh)
        a1, a2 = open(os.path.join(tmp, "a1.csv")).read(), open(os.path.join(tmp, "a2.csv")).read()
        assert a1 == a2
        import re
        n = int(re.search(r"\((\d+) objects\)", r1.stdout).group(1))
        assert n == (60000 if host_too else 60001) and sum(int(l.split(",")[3]) for l in a1.splitlines()[1:]) == n
        if host_too:        # (the odd record's line of the CSV runs on into the next line, as the reference prints it: no CSV to read back)
            assert _run([EST, "-F", os.path.join(tmp, "out.csv"), "-c", "0.6"]).stdout == a1
            r3 = _run(base + ["--abundance", os.path.join(tmp, "a3.csv")], {"MIC_HOST_INGEST": "1"})
            assert r3.returncode == 0, r3.stderr
            assert open(os.path.join(tmp, "a3.csv")).read() == a1


def _golden_db(tmp):
    from test_cli import _db_dir, _targets_file
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


def _repeat(src, dst, times, gz=False):
    data = open(src, "rb").read() * times
    if gz:
        with gzip.open(dst, "wb") as f:
            f.write(data)
    else:
        open(dst, "wb").write(data)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fa", "fq", "pairs", "fq_gz", "fq_gz_host", "sharded2", "sharded3", "throughput"])
def test_cli_abundance_equals_estimate_abundance(tmp_path, case):
    tmp = str(tmp_path)
    t, d = _golden_db(tmp)
    env = {"MIC_INGEST_KB": "64"}
    if case == "pairs":
        m1, m2 = os.path.join(tmp, "m1.fq"), os.path.join(tmp, "m2.fq")
        _repeat(os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), m1, 300)
        _repeat(os.path.join(gu.GOLDEN, "pairs_k31_2.fq"), m2, 300)
        inp = ["-P", m1, m2]
    else:
        src = "reads_k31.fa" if case == "fa" else "reads_k31.fq"
        p = os.path.join(tmp, "in." + ("fa" if case == "fa" else "fq") + (".gz" if "gz" in case else ""))
        _repeat(os.path.join(gu.GOLDEN, src), p, 300, gz="gz" in case)
        inp = ["-O", p]
    extra = []
    if case == "fq_gz_host":
        env["MIC_GZ_HOST"] = "1"
    if case.startswith("sharded"):
        env["MIC_SHARD_ENGINES"] = case[-1]
        extra = ["--db-sharded", "--parts", case[-1]]
    if case == "throughput":
        env["MIC_SHARD_ENGINES"] = "3"
        extra = ["-n", "6", "-b", "6"]
    filt = ["--min-confidence", "0.6", "--min-gamma", "0.25", "--min-abundance", "12.5"]
    base = [EXE, "-k", "31", "-T", t, "-D", d, *inp, *extra]
    out0, out1 = os.path.join(tmp, "o0"), os.path.join(tmp, "o1")
    r0 = _run(base + ["-R", out0], env)
    assert r0.returncode == 0, r0.stderr
    r1 = _run(base + ["-R", out1, "--abundance", os.path.join(tmp, "a1.csv"), *filt], env)
    assert r1.returncode == 0, r1.stderr
    assert open(out0 + ".csv", "rb").read() == open(out1 + ".csv", "rb").read()
    r2 = _run(base + ["--abundance", os.path.join(tmp, "a2.csv"), *filt], env)
    assert r2.returncode == 0, r2.stderr
    assert not os.path.exists(os.path.join(tmp, ".csv")) and "Results stored" not in r2.stdout
    est = _run([EST, "-F", out1 + ".csv", "-c", "0.6", "-g", "0.25", "-a", "12.5"])
    assert est.returncode == 0, est.stderr
    a1, a2 = open(os.path.join(tmp, "a1.csv")).read(), open(os.path.join(tmp, "a2.csv")).read()
    assert a1 == est.stdout and a2 == a1
    n = sum(1 for _ in open(out1 + ".csv")) - 1
    assert sum(int(l.split(",")[3]) for l in a1.splitlines()[1:]) <= n and n > 10000


@pytest.mark.gpu
def test_cli_abundance_argument_errors(tmp_path):
    tmp = str(tmp_path)
    t, d = _golden_db(tmp)
    reads = os.path.join(gu.GOLDEN, "reads_k31.fa")
    r = _run([EXE, "-k", "31", "-T", t, "-D", d, "-O", reads, "--abundance", os.path.join(tmp, "a.csv"), "--extended"])
    assert r.returncode != 0 and "--extended" in r.stderr
    r = _run([EXE, "-k", "31", "-T", t, "-D", d, "-O", reads, "-R", "x", "--min-confidence", "1.5"])
    assert r.returncode == 1 and "--min-confidence" in r.stderr
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    r = _run([EXE, "-k", "31", "-T", t, "-D", d, "-O", lo, "-R", lr, "--abundance", os.path.join(tmp, "a.csv")])
    assert r.returncode != 0 and "list-of-files" in r.stderr
    # --extended with -R: the extended CSV is unchanged and the profile is written
    r = _run([EXE, "-k", "31", "-T", t, "-D", d, "-O", reads, "-R", os.path.join(tmp, "e"), "--extended", "--abundance", os.path.join(tmp, "ae.csv")])
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(tmp, "e.csv"), "rb").read() == open(os.path.join(gu.GOLDEN, "expected_k31_fa_ext.csv"), "rb").read()
    assert open(os.path.join(tmp, "ae.csv")).read() == _run([EST, "-F", os.path.join(gu.GOLDEN, "expected_k31_fa.csv")]).stdout


@pytest.mark.gpu
def test_set_targets_then_classify_with_abundance_names(tmp_path):
    """set_targets.sh -> classify_metagenome.sh --abundance on a taxonomy fixture: scientific names and lineages in the profile."""
    import test_targets_tools as tt
    tmp = str(tmp_path)
    db = os.path.join(tmp, "DBD")
    tax = os.path.join(db, "taxonomy")
    os.makedirs(os.path.join(db, "Custom"))
    golden = gu.target_files_and_labels()
    names_golden = gu.target_names()
    species = {lab: 5000 + i for i, lab in enumerate(names_golden)}
    tt.make_taxonomy(tax)
    with open(os.path.join(tax, "nodes.dmp"), "a") as f:
        for s in species.values():
            f.write(f"{s}\t|\t561\t|\tspecies\t|\tXX\t|\n")
    with open(os.path.join(tax, "nucl_accss"), "a") as f:
        for i, (fn, lab) in enumerate(golden):
            f.write(f"rec{i}a\trec{i}a.1\t{species[lab]}\t{100 + i}\n")
            shutil.copy(fn, os.path.join(db, "Custom", os.path.basename(fn)))
    sci = {2: "Bacteria", 1224: "Proteobacteria", 1236: "Gammaproteobacteria", 91347: "Enterobacterales", 543: "Enterobacteriaceae",
           561: "Escherichia"}
    with open(os.path.join(tax, "names.dmp"), "w") as f:
        for i, n in sci.items():
            f.write(f"{i}\t|\t{n}\t|\t\t|\tscientific name\t|\n")
        for lab, s in species.items():
            f.write(f"{s}\t|\tSpecies {lab}\t|\t\t|\tscientific name\t|\n")
    open(os.path.join(db, ".taxondata"), "w").close()
    r = _run([os.path.join(gu.ROOT, "set_targets.sh"), db, "custom"], cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    reads = os.path.join(gu.GOLDEN, "reads_k27.fa")
    r = _run([os.path.join(gu.ROOT, "classify_metagenome.sh"), "-O", reads, "-R", os.path.join(tmp, "out"), "-k", "27",
              "--htsize", "57777779", "--abundance", os.path.join(tmp, "ab.csv")], cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(os.path.join(tmp, "ab.csv")).read().splitlines()
    assert lines[0] == "Name,TaxID,Lineage,Count,Proportion_All(%),Proportion_Classified(%)"
    lineage = "Bacteria;Proteobacteria;Gammaproteobacteria;Enterobacterales;Enterobacteriaceae;Escherichia"
    body = lines[1:-1]
    assert body and all(l.split(",")[0].startswith("Species ") and l.split(",")[2] == lineage for l in body)
    assert {l.split(",")[1] for l in body} <= {str(s) for s in species.values()}
    est = _run([os.path.join(gu.ROOT, "estimate_abundance.sh"), "-F", os.path.join(tmp, "out.csv")], cwd=tmp)
    assert est.returncode == 0 and est.stdout == "\n".join(lines) + "\n", est.stderr


@pytest.mark.gpu
def test_abundance_device_on_torch_tensors():
    import torch
    from cuclark_amd import MiClarkDB, host
    rng = np.random.default_rng(9)
    T, k, n = 65535, 31, 300_000
    res = np.zeros((n, 8), np.uint32)
    res[:, 2] = rng.integers(1, 300, n)
    res[:, 4] = np.minimum(res[:, 2], rng.integers(0, 300, n))
    res[:, 0] = res[:, 2] + res[:, 4]
    res[:, 1] = rng.choice(np.array([0, 1, 2, 3, 100, 65534, 65535, 65536, 4000000], np.uint32), n)
    norm = rng.integers(1, 500, n).astype(np.uint32)
    dev = torch.device("cuda:0")
    d_res = torch.from_numpy(res.view(np.int32)).to(dev)
    d_norm = torch.from_numpy(norm.view(np.int32)).to(dev)
    with MiClarkDB(k, T) as e:
        for c, g in FILTERS:
            d_counts = torch.zeros(T + 2, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            e.abundance_device(d_res.data_ptr(), d_norm.data_ptr(), n, d_counts.data_ptr(), host.abund_filter(c, g))
            e.sync()
            got = d_counts.cpu().numpy().view(np.uint64)
            assert (got == host.abundance_host(res, norm, k, T, host.abund_filter(c, g))).all(), (c, g)
            assert int(got.sum()) == n and got[0] > 0 and got[T + 1] > 0
        d_counts = torch.zeros(T + 2, dtype=torch.int64, device=dev)
        with pytest.raises(Exception):
            e.abundance_device(d_res.data_ptr(), 0, n, d_counts.data_ptr(), host.abund_filter("0.5", "0.1"))
