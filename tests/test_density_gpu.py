"""Score densities on the MI355X: density_kernel (mic_density_device on torch tensors) against the host rule, which test_density.py
pins to a restatement in exact fractions; the engine's counters over ingest batches equal the rule on the returned result rows, with
and without MIC_INGEST_NO_CSV, next to the abundance counters, and a batch handed back adds nothing; exe/cuCLARK --density equals
exe/evaluate_density on its own result CSV on every input path, and a summary-only run (no -R) writes the same file."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
from test_density import CONF_BINS, GAMMA_BINS, T, WORDS, _cell, edge_rows, random_rows

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
EVAL = os.path.join(gu.ROOT, "exe", "evaluate_density")
EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")
K = 31


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=300, env=e, **kw)


def _device(e, res, norm, d_counts=None):
    """mic_density_device on torch tensors; returns (counters u64[5153], the device tensor they were added to)"""
    import torch
    dev = torch.device("cuda:0")
    d_res = torch.from_numpy(np.ascontiguousarray(res, np.uint32).view(np.int32)).to(dev)
    d_norm = torch.from_numpy(np.ascontiguousarray(norm, np.uint32).view(np.int32)).to(dev) if norm is not None else None
    if d_counts is None:
        d_counts = torch.zeros(WORDS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.density_device(d_res.data_ptr(), d_norm.data_ptr() if d_norm is not None else 0, res.shape[0], d_counts.data_ptr())
    e.sync()
    return d_counts.cpu().numpy().view(np.uint64), d_counts


@pytest.fixture(scope="module")
def rows():
    """the edge rows of test_density.py followed by random ones, 100 003 in all (one reference for every size below)"""
    e_res, e_norm = edge_rows(K)
    r_res, r_norm = random_rows(np.random.default_rng(77), 100_003 - e_res.shape[0], K)
    return np.concatenate([e_res, r_res]), np.concatenate([e_norm, r_norm])


@pytest.mark.gpu
def test_kernel_on_crafted_rows(rows):
    """Sizes around the wave, the block and the grid's stride; maximal contention on one cell; every cell once; a second call adds;
    no lengths: gamma bin 0."""
    from cuclark_amd import MiClarkDB, host
    res, norm = rows
    with MiClarkDB(K, T) as e:
        for n in (1, 63, 64, 65, 255, 256, 257, 100_003):
            got, _ = _device(e, res[:n], norm[:n])
            want = host.density_host(res[:n], norm[:n], K, T)
            assert (got == want).all(), (n, np.flatnonzero(got != want)[:8])
            assert int(got[0]) == n and int(got[1]) + int(got[2:].sum()) == n
        # 70 000 identical rows: every lane of every wave adds to one LDS address
        same = np.tile(np.array([[40, 1, 40, 0, 0, 1, 0, 0]], np.uint32), (70_000, 1))
        got, _ = _device(e, same, np.full(70_000, 150, np.uint32))
        assert int(got[0]) == 70_000 and int(got[_cell(100, 33)]) == 70_000 and int(got.sum()) == 140_000
        # every cell exactly once: den = 100, best = c, second = 100 - c, sum = g
        cg = np.array([(c, g) for c in range(50, 101) for g in range(GAMMA_BINS)], np.uint32)
        every = np.zeros((cg.shape[0], 8), np.uint32)
        every[:, 0], every[:, 1], every[:, 2], every[:, 4] = cg[:, 1], 1 + np.arange(cg.shape[0]) % T, cg[:, 0], 100 - cg[:, 0]
        n1 = np.full(cg.shape[0], 100 + K - 1, np.uint32)
        got, d_counts = _device(e, every, n1)
        assert cg.shape[0] == CONF_BINS * GAMMA_BINS == 5151 and int(got[0]) == 5151 and int(got[1]) == 0 and (got[2:] == 1).all()
        assert (got == host.density_host(every, n1, K, T)).all()
        # counts are ADDED to d_counts
        got2, _ = _device(e, every, n1, d_counts)
        assert int(got2[0]) == 2 * 5151 and (got2[2:] == 2).all()
        # d_norm = NULL
        got, _ = _device(e, res[:1000], None)
        want = host.density_host(res[:1000], None, K, T)
        assert (got == want).all() and int(got[2:].reshape(CONF_BINS, GAMMA_BINS)[:, 1:].sum()) == 0 and int(got[2:].sum()) > 500


def _child_crafted_rows():
    """(runs in a child process: the library reads MIC_DENSITY_AGG once)  crafted rows through the form the variable picks"""
    from cuclark_amd import MiClarkDB, host
    e_res, e_norm = edge_rows(K)
    r_res, r_norm = random_rows(np.random.default_rng(78), 20_000, K)
    res, norm = np.concatenate([e_res, r_res]), np.concatenate([e_norm, r_norm])
    same = np.tile(np.array([[40, 1, 40, 0, 0, 1, 0, 0]], np.uint32), (5_000, 1))
    with MiClarkDB(K, T) as e:
        for n in (1, 65, 257, res.shape[0]):
            got, _ = _device(e, res[:n], norm[:n])
            assert (got == host.density_host(res[:n], norm[:n], K, T)).all(), n
        got, _ = _device(e, same, np.full(5_000, 150, np.uint32))
        assert int(got[_cell(100, 33)]) == 5_000 and int(got.sum()) == 10_000
    print("CHILD OK")


@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["0", "2"])
def test_kernel_alternative_aggregations(agg):
    """The two forms kept for the measurement of DESIGN.md 4.7 (MIC_DENSITY_AGG: one add per lane, the full ballot loop) count what
    the default form counts."""
    import sys
    code = f"import sys; sys.path[:0] = [{gu.ROOT!r}, {os.path.join(gu.ROOT, 'tests')!r}]; import test_density_gpu as t; t._child_crafted_rows()"
    r = _run([sys.executable, "-c", code], {"MIC_DENSITY_AGG": agg})
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _synth(n_targets=256, genome_nt=2_000_000, htsize=57777779, k=K, seed=11):
    """a synthetic database in device memory (as test_abundance_gpu.py builds its own)"""
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    spec = _lib.MicSynthSpec(seed=seed, htsize=htsize, genome_nt=genome_nt, n_targets=n_targets, n_genomes=n_targets, k=k, key_bytes=8)
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
@pytest.mark.parametrize("layout", ["direct", "super"])
def test_ingest_counters_equal_the_rule(layout):
    """256 targets, 50 000 reads in batches of ~256 KB: the engine's counters equal the rule on the returned result rows, are the same
    with MIC_INGEST_NO_CSV, and abundance and density started together each give what they give alone."""
    from cuclark_amd import MiClarkDB, host
    from cuclark_amd._lib import MicError
    n_targets, n_reads = 256, 50_000
    spec, d_sizes, d_keys, d_labels = _synth(n_targets)
    text, rb = _reads_text(spec, n_reads)
    per = (256 << 10) // rb
    names = [f"L{i}" for i in range(n_targets)]
    norm = np.full(n_reads, 150, np.uint32)

    def run(e, csv):
        out_rows = []
        for r0 in range(0, n_reads, per):
            r1 = min(n_reads, r0 + per)
            out = e.ingest_classify(0, text[r0 * rb:r1 * rb], csv=csv)
            assert out["status"] == 0 and out["n_reads"] == r1 - r0 and (out["csv"] != b"") == csv
            out_rows.append(out["results"])
        return np.concatenate(out_rows)

    with MiClarkDB(K, n_targets, layout={"direct": 1, "super": 3}[layout]) as e:
        e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, 512 << 10, names, want_results=True)
        with pytest.raises(MicError) as err:            # not started: nothing was allocated, nothing to fetch
            e.density_fetch()
        assert err.value.code == -5                     # MIC_E_STATE
        res0 = run(e, True)                             # (counting off)
        got = {}
        for csv in (True, False):
            e.density_start()
            res = run(e, csv)
            got[csv] = e.density_fetch()
            assert (res[:, :5] == res0[:, :5]).all()
        e.density_stop()
        want = host.density_host(res0, norm, K, n_targets)
        assert (got[True] == want).all() and (got[False] == want).all(), layout
        assert int(want[0]) == n_reads and int(want[1]) > 0 and int(np.count_nonzero(want[2:])) > 20
        # stopped: the counters keep their values
        run(e, False)
        assert (e.density_fetch() == want).all()
        # abundance alone, then both together
        f = host.abund_filter("0.75", "0.03")
        e.abundance_start(f)
        run(e, False)
        ab_alone = e.abundance_fetch()
        e.abundance_start(f)
        e.density_start()
        run(e, False)
        assert (e.abundance_fetch() == ab_alone).all() and (e.density_fetch() == want).all()
        assert (ab_alone == host.abundance_host(res0, norm, K, n_targets, f)).all()
        e.abundance_stop()
        # a batch that is handed back (an odd record: the empty name) adds nothing on the device
        e.density_start()
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + text[:rb * 100]
        out = e.ingest_classify(0, bad, csv=False)
        assert out["status"] & 1
        assert int(e.density_fetch().sum()) == 0
        assert e.L.mic_density_fetch(e.h, np.zeros(8, np.uint64).ctypes.data, 8) == -1      # MIC_E_INVALID: n must be MIC_DENSITY_WORDS


def _golden_db(tmp):
    from test_cli import _db_dir, _targets_file
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fq", "fq_gz", "pairs", "extended"])
def test_cli_density_equals_evaluate_density(tmp_path, case):
    """--density d.csv -R out equals evaluate_density -F out.csv byte for byte; the summary-only run writes the same file and no CSV;
    the result CSV does not change with the option."""
    tmp = str(tmp_path)
    t, d = _golden_db(tmp)
    o = lambda n: os.path.join(tmp, n)
    env = {"MIC_INGEST_KB": "64"}
    extra = []
    if case == "pairs":
        inp = ["-P", os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")]
    elif case == "fq_gz":
        with gzip.open(o("in.fq.gz"), "wb") as f:
            f.write(open(os.path.join(gu.GOLDEN, "reads_k31.fq"), "rb").read())
        inp = ["-O", o("in.fq.gz")]
    else:
        inp = ["-O", os.path.join(gu.GOLDEN, "reads_k31.fq")]
    if case == "extended":
        extra = ["--extended"]
    base = [EXE, "-k", "31", "-T", t, "-D", d, *inp]
    r0 = _run(base + ["-R", o("o0"), *extra], env)
    r1 = _run(base + ["-R", o("o1"), *extra, "--density", o("d1.csv")], env)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert open(o("o0.csv"), "rb").read() == open(o("o1.csv"), "rb").read()
    assert "Density report stored" in r1.stdout
    ev = _run([EVAL, "-F", o("o1.csv")])
    assert ev.returncode == 0, ev.stderr
    d1 = open(o("d1.csv")).read()
    assert d1 == ev.stdout
    n = sum(1 for _ in open(o("o1.csv"))) - 1
    assert d1.startswith(f"Reads,{n}\n") and n >= 10
    if case == "fq":
        assert open(o("o1.csv"), "rb").read() == open(os.path.join(gu.GOLDEN, "expected_k31_fq.csv"), "rb").read()
    if case != "extended":          # (--extended writes the result CSV: it needs -R)
        r2 = _run(base + ["--density", o("d2.csv")], env)
        assert r2.returncode == 0, r2.stderr
        assert open(o("d2.csv")).read() == d1
        assert "Results stored" not in r2.stdout and not os.path.exists(os.path.join(tmp, ".csv"))
    else:
        r2 = _run(base + ["--density", o("d2.csv"), "--extended"], env)
        assert r2.returncode != 0 and "--extended" in r2.stderr


@pytest.mark.gpu
def test_cli_density_with_abundance_and_rank_report(tmp_path):
    """one run with all three summaries writes three files, each equal to the file of its solo run; host-path runs count the same"""
    import rollup_util as ru
    tmp = str(tmp_path)
    t, d = _golden_db(tmp)
    o = lambda n: os.path.join(tmp, n)
    lin = o("lineage.tsv")
    ru.golden_lineage_file(lin)
    env = {"MIC_INGEST_KB": "64"}
    base = [EXE, "-k", "31", "-T", t, "-D", d, "-O", os.path.join(gu.GOLDEN, "reads_k31.fq"), "--min-confidence", "0.75"]
    all3 = _run(base + ["--density", o("d.csv"), "--abundance", o("a.csv"), "--rank-report", o("r.csv"), "--lineage", lin], env)
    assert all3.returncode == 0, all3.stderr
    solo = [_run(base + ["--density", o("d1.csv")], env), _run(base + ["--abundance", o("a1.csv")], env),
            _run(base + ["--rank-report", o("r1.csv"), "--lineage", lin], env)]
    assert all(r.returncode == 0 for r in solo), [r.stderr for r in solo]
    for a, b in (("d.csv", "d1.csv"), ("a.csv", "a1.csv"), ("r.csv", "r1.csv")):
        assert open(o(a)).read() == open(o(b)).read(), a
    assert open(o("d.csv")).read() == _run([EVAL, "-F", os.path.join(gu.GOLDEN, "expected_k31_fq.csv")]).stdout
    # the host path (MIC_HOST_INGEST) counts every batch with the host rule
    rh = _run(base + ["--density", o("dh.csv")], {"MIC_HOST_INGEST": "1"})
    assert rh.returncode == 0 and open(o("dh.csv")).read() == open(o("d.csv")).read(), rh.stderr


@pytest.mark.gpu
def test_cli_density_refuses_list_of_files(tmp_path):
    """(the check sits behind the database load, so it needs the device: tests/test_density.py has the argument check without one)"""
    tmp = str(tmp_path)
    t, d = _golden_db(tmp)
    reads = os.path.join(gu.GOLDEN, "reads_k31.fa")
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    r = _run([EXE, "-k", "31", "-T", t, "-D", d, "-O", lo, "-R", lr, "--density", os.path.join(tmp, "d.csv")])
    assert r.returncode != 0 and "--density" in r.stderr and "list-of-files" in r.stderr and "evaluate_density" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "d.csv"))
