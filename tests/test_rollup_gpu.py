"""Rank roll-up on the MI355X: mic_rollup_device / mic_rollup_dense_device on torch tensors against the host rule (which
test_rollup.py pins to the plain-Python restatement), and the engine's roll-up counters and rows over ingest batches under every
table layout against the host rule on the rows mic_query_device writes for the same packed reads."""
import numpy as np
import pytest

import rollup_util as ru
from test_abundance_gpu import _reads_text, _synth


def _random_rows(rng, n, T, rw, n_invalid):
    """u32[n, rw]: ascending distinct targets below T, many rows of 0 / 1 entries, ties, counts of 65535, n_invalid invalid rows."""
    cap = rw - 1
    u = rng.random(n)
    ne = np.where(u < 0.15, 0, np.where(u < 0.6, 1, np.where(u < 0.65, cap, rng.integers(2, cap + 1, n)))).astype(np.int64)
    # a row's targets lie in a window of its own width, so that close relatives (one group a few levels up) and strangers both occur
    width = rng.choice(np.array([1, 16, 256, 4096, T - cap]), n)
    base = (rng.random(n) * (T - cap - width + 1)).astype(np.int64)
    tg = np.sort((rng.random((n, cap)) * width[:, None]).astype(np.int64), axis=1) + np.arange(cap) + base[:, None]
    cn = rng.integers(1, 4, (n, cap))
    big = rng.random((n, cap)) < 0.02
    cn[big] = rng.choice(np.array([65535, 300, 1000]), int(big.sum()))
    rows = np.zeros((n, rw), np.uint32)
    rows[:, 1:] = ((cn.astype(np.uint32) << 16) | tg.astype(np.uint32)) * (np.arange(cap)[None, :] < ne[:, None])
    rows[:, 0] = ne
    bad = rng.choice(n, n_invalid, replace=False)
    rows[bad, 0] = ru.ROW_INVALID
    return rows, np.sort(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("rw", [16, 65])
def test_rollup_device_on_torch_tensors(rw):
    import torch
    from cuclark_amd import MiClarkDB, host
    rng = np.random.default_rng(40 + rw)
    T, L, k, n, n_bad = 65535, 7, 31, 1_000_000, 600
    gof = np.stack([np.arange(T) // 4 ** l for l in range(1, L + 1)]).astype(np.uint16)
    rows, bad = _random_rows(rng, n, T, rw, n_bad)
    norm = rng.integers(20, 400, n).astype(np.uint32)
    dense = np.zeros((n_bad, T), np.uint32)
    for i in range(n_bad):
        m = int(rng.integers(1, 200))
        dense[i, rng.choice(T, m, replace=False)] = rng.integers(1, 4, m)
    dense[::7, 5] = 70000
    dev = torch.device("cuda:0")
    d_rows = torch.from_numpy(rows.view(np.int32)).to(dev)
    d_norm = torch.from_numpy(norm.view(np.int32)).to(dev)
    d_dense = torch.from_numpy(dense.view(np.int32)).to(dev)
    d_ids = torch.from_numpy(bad.astype(np.int32)).to(dev)
    with MiClarkDB(k, T, row_words=rw) as e:
        with pytest.raises(Exception):
            e.rollup_layout()                    # no lineage yet
        e.rollup_set(gof)
        n_groups, n_counters = e.rollup_layout()
        assert n_groups.tolist() == [T] + [int(gof[l].max()) + 1 for l in range(L)] and n_counters == 2 + int(n_groups.sum())
        for c, g in ru.FILTERS:
            f = host.abund_filter(c, g)
            d_roll = torch.full((n, 8), -1, dtype=torch.int32, device=dev)
            d_lev = torch.full((n, L + 1, 4), -1, dtype=torch.int32, device=dev)
            d_cnt = torch.zeros(n_counters, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            e.rollup_device(d_rows.data_ptr(), d_norm.data_ptr(), n, d_roll.data_ptr(), d_lev.data_ptr(), d_cnt.data_ptr(), f)
            e.sync()
            want = host.rollup_host(rows, norm, k, T, gof, f, want_levels=True)
            got = (d_roll.cpu().numpy().view(np.uint32), d_lev.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint64))
            for a, b, what in zip(got, want, ("rollup", "levels", "counters")):
                assert (a == b).all(), (what, rw, c, g, np.argwhere(a != b)[:5])
            assert (got[0][bad, 5] == ru.PENDING).all() and (got[0][bad, 6] == 1).all()
            assert int(got[2].sum()) == n - n_bad
            if c != "0.5":                       # (confidence is never below 0.5: the default filter stops at level 0)
                assert set(got[0][:, 5].tolist()) >= {0, 1, 2, 3, 4, 5, 6, 7, ru.UNRESOLVED, ru.PENDING}
            # the dense form completes the pending reads to the host result
            e.rollup_dense_device(d_dense.data_ptr(), d_ids.data_ptr(), n_bad, d_norm.data_ptr(), d_roll.data_ptr(), d_lev.data_ptr(),
                                  d_cnt.data_ptr(), f)
            e.sync()
            w2 = host.rollup_host(None, norm[bad], k, T, gof, f, dense=dense, want_levels=True)
            got = (d_roll.cpu().numpy().view(np.uint32), d_lev.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint64))
            assert (got[0][bad] == w2[0]).all() and (got[1][bad] == w2[1]).all()
            assert (got[2] == want[2] + w2[2]).all() and int(got[2].sum()) == n
            keep = np.ones(n, bool)
            keep[bad] = False
            assert (got[0][keep] == want[0][keep]).all()
        # counters are optional, and a gamma threshold needs the lengths
        e.rollup_device(d_rows.data_ptr(), 0, 1000, d_roll.data_ptr(), 0, 0, host.abund_filter("0.75", "0"))
        e.sync()
        assert (d_roll[:1000].cpu().numpy().view(np.uint32) == host.rollup_host(rows[:1000], None, k, T, gof, host.abund_filter("0.75", "0"))[0]).all()
        with pytest.raises(Exception):
            e.rollup_device(d_rows.data_ptr(), 0, n, d_roll.data_ptr(), 0, 0, host.abund_filter("0.5", "0.1"))
        with pytest.raises(Exception):
            e.rollup_set(gof[::-1])              # not a coarsening
        e.rollup_set(None)
        with pytest.raises(Exception):
            e.rollup_device(d_rows.data_ptr(), d_norm.data_ptr(), n, d_roll.data_ptr(), 0, 0, host.abund_filter())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["direct", "minimizer", "super", "super2"])
def test_ingest_rollup_counters_equal_the_host_rule(layout):
    """4096 targets with mosaic stretches (reads that hit several close relatives), lineage t // 4, t // 32, t // 512, 1 M reads in
    batches of ~1 MB: the fetched counters and the returned roll-up rows equal the host rule on the rows mic_query_device writes for
    the packed reads of the same batch; identical with MIC_INGEST_NO_CSV; a batch that is handed back adds nothing."""
    import torch
    from cuclark_amd import MiClarkDB, host
    ids = {"direct": 1, "minimizer": 2, "super": 3, "super2": 4}
    T, k, n_reads = 4096, 31, 1_000_000
    spec, d_sizes, d_keys, d_labels = _synth(T, mosaic_ppm=2000)
    text, rb = _reads_text(spec, n_reads)
    per = (1 << 20) // rb
    names = [f"L{i}" for i in range(T)]
    t = np.arange(T)
    gof = np.stack([t // 4, t // 32, t // 512]).astype(np.uint16)
    dev = torch.device("cuda:0")
    RW = 65
    with MiClarkDB(k, T, layout=ids[layout], row_words=RW) as e:
        e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        e.ingest_alloc(1, 2 << 20, names, want_results=True)
        e.rollup_set(gof)
        _, n_counters = e.rollup_layout()
        plain = e.ingest_classify(0, text[:per * rb])                     # before roll-up is started: the default path
        with pytest.raises(Exception):
            e.ingest_rollup_rows(0)
        for c, g in [("0.75", "0"), ("0.9", "0.03")]:
            f = host.abund_filter(c, g)
            got, rolls, want = {}, {}, np.zeros(n_counters, np.uint64)
            levels_seen = set()
            for csv in (True, False):
                e.rollup_start(f)
                rolls[csv] = []
                handed_back = 0
                for r0 in range(0, n_reads, per):
                    r1 = min(n_reads, r0 + per)
                    out = e.ingest_classify(0, text[r0 * rb:r1 * rb], csv=csv)
                    if out["status"] != 0:
                        assert out["status"] & 32                          # a read of more than 64 targets: the host path's batch
                        handed_back += 1
                        rolls[csv].append(None)
                        continue
                    if r0 == 0:
                        assert (out["results"] == plain["results"]).all() and (not csv or out["csv"] == plain["csv"])
                    roll = e.ingest_rollup_rows(0)
                    assert roll.shape == (r1 - r0, 8)
                    rolls[csv].append(roll)
                    if csv:                                                # the expectation, once per filter
                        rp, ct = e.ingest_fetch_packed(0)
                        d_rp = torch.from_numpy(rp.view(np.int32)).to(dev)
                        d_ct = torch.zeros(ct.size + 64, dtype=torch.int16, device=dev)
                        d_ct[:ct.size] = torch.from_numpy(ct.view(np.int16)).to(dev)
                        d_res = torch.zeros((r1 - r0, 8), dtype=torch.int32, device=dev)
                        d_rows = torch.zeros((r1 - r0, RW), dtype=torch.int32, device=dev)
                        torch.cuda.synchronize()
                        e.query_device(d_rp.data_ptr(), d_ct.data_ptr(), r1 - r0, d_res.data_ptr(), d_rows.data_ptr())
                        e.sync()
                        rows = d_rows.cpu().numpy().view(np.uint32)
                        assert (rows[:, 0] != ru.ROW_INVALID).all()
                        w = host.rollup_host(rows, np.full(r1 - r0, 150, np.uint32), k, T, gof, f)
                        assert (roll == w[0]).all(), (layout, c, g, r0)
                        want += w[2]
                        levels_seen |= set(w[0][:, 5].tolist())
                got[csv] = e.rollup_fetch()
                e.rollup_stop()
                assert handed_back < n_reads // per // 2
            assert (got[True] == want).all() and (got[False] == want).all(), (layout, c, g)
            assert all((a is None and b is None) or (a == b).all() for a, b in zip(rolls[True], rolls[False]))
            assert int(want.sum()) == sum(len(r) for r in rolls[True] if r is not None)
            assert {0, ru.UNRESOLVED} <= levels_seen, levels_seen                    # (mosaic labels are spread over all groups: few reads stop in between)
        # a batch that is handed back adds nothing on the device: an odd record (empty name)
        e.rollup_start(host.abund_filter())
        bad = b"@\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" + text[:rb * 100]
        out = e.ingest_classify(0, bad, csv=False)
        assert out["status"] & 1
        assert int(e.rollup_fetch().sum()) == 0
        with pytest.raises(Exception):
            e.rollup_set(None)                   # not while counting is started
        e.rollup_stop()


# ---- the command line ----------------------------------------------------------------------------------------------------------
import gzip
import os
import re
import subprocess

import golden_util as gu

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
EST = os.path.join(gu.ROOT, "exe", "estimate_abundance")


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=600, env=e, **kw)


def _expected_report(dbname, data, paired, c="0.75", g="0"):
    names = gu.target_names()
    counts, norm, k, _ = ru.oracle_counts(dbname, data, paired)
    _, _, counters = ru.restate(ru.pairs_of_dense(counts), norm, k, len(names), ru.GOLDEN_LINEAGE, c, g)
    return ru.report(counters, len(names), ru.GOLDEN_LINEAGE, ru.GOLDEN_RANKS, [names] + ru.GOLDEN_GROUPS[1:]), int(counters.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fa", "fq", "pairs", "fq_gz", "sharded2", "throughput", "fa_light"])
def test_cli_rank_report_three_ways(tmp_path, case):
    """The chimeric reads of test_rollup.py through exe/cuCLARK: the report of the device ingest path (no -R), of the host path
    (-R --extended) and of estimate_abundance on the extended CSV are equal and equal the restatement on the oracle's counts."""
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path)
    light = case == "fa_light"
    dbname = "light_k27_u32" if light else "full_k31_u32"
    exe = EXE + ("-l" if light else "")
    t, d = _targets_file(tmp), _db_dir(tmp, dbname, light=light)
    seqs = ru.chimeric_reads()
    env = {"MIC_INGEST_KB": "64"}
    paired = case == "pairs"
    if paired:
        m1, m2 = os.path.join(tmp, "m1.fq"), os.path.join(tmp, "m2.fq")
        f1, f2 = ru.fastq([s[:75] for s in seqs], "/1"), ru.fastq([s[75:] for s in seqs], "/2")
        open(m1, "wb").write(f1)
        open(m2, "wb").write(f2)
        inp, data = ["-P", m1, m2], gu.merge_pairs(f1, f2)
    else:
        fa = case in ("fa", "fa_light")
        data = ru.fasta(seqs) if fa else ru.fastq(seqs)
        p = os.path.join(tmp, "in." + ("fa" if fa else "fq") + (".gz" if "gz" in case else ""))
        if "gz" in case:
            with gzip.open(p, "wb") as f:
                f.write(data)
        else:
            open(p, "wb").write(data)
        inp = ["-O", p]
    extra = []
    if case == "sharded2":
        env["MIC_SHARD_ENGINES"] = "2"
        extra = ["--db-sharded", "--parts", "2"]
    if case == "throughput":
        env["MIC_SHARD_ENGINES"] = "3"
        extra = ["-n", "6", "-b", "6"]
    want, total = _expected_report(dbname, data, paired)
    assert total == len(seqs)
    lin = os.path.join(tmp, "lineage.tsv")
    ru.golden_lineage_file(lin)
    base = [exe, "-k", "27" if light else "31", "-T", t, "-D", d, *inp, *extra]
    filt = ["--min-confidence", "0.75"]
    o = lambda n: os.path.join(tmp, n)
    # (a) -R --extended, then estimate_abundance on its CSV
    ra = _run(base + ["-R", o("a"), "--extended"], env)
    assert ra.returncode == 0, ra.stderr
    est = _run([EST, "-F", o("a.csv"), "--rank-report", o("ra.csv"), "--lineage", lin, "-c", "0.75"])
    assert est.returncode == 0, est.stderr
    assert open(o("ra.csv")).read() == want, case
    # (b) the device ingest path, summary only: no CSV is written
    rb = _run(base + ["--rank-report", o("rb.csv"), "--lineage", lin, *filt], env)
    assert rb.returncode == 0, rb.stderr
    assert open(o("rb.csv")).read() == want, case
    assert "Results stored" not in rb.stdout and "Rank report stored" in rb.stdout and not os.path.exists(os.path.join(tmp, ".csv"))
    # (c) the host path
    rc = _run(base + ["-R", o("c"), "--extended", "--rank-report", o("rc.csv"), "--lineage", lin, *filt], env)
    assert rc.returncode == 0, rc.stderr
    assert open(o("rc.csv")).read() == want, case
    assert open(o("c.csv"), "rb").read() == open(o("a.csv"), "rb").read()
    # the -R CSV is byte-identical with and without the flag; together with --abundance both files equal their stand-alone runs
    r0 = _run(base + ["-R", o("p0")], env)
    r1 = _run(base + ["-R", o("p1"), "--rank-report", o("r1.csv"), "--lineage", lin, "--abundance", o("ab1.csv"), *filt], env)
    r2 = _run(base + ["--abundance", o("ab2.csv"), *filt], env)
    assert r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r0.stderr + r1.stderr + r2.stderr
    assert open(o("p0.csv"), "rb").read() == open(o("p1.csv"), "rb").read()
    assert open(o("r1.csv")).read() == want and open(o("ab1.csv")).read() == open(o("ab2.csv")).read()


@pytest.mark.gpu
def test_cli_rank_report_argument_errors(tmp_path):
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path)
    t, d = _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)
    reads = os.path.join(gu.GOLDEN, "reads_k31.fa")
    base = [EXE, "-k", "31", "-T", t, "-D", d, "-O", reads]
    r = _run(base + ["--rank-report", os.path.join(tmp, "r.csv")])             # no --lineage, no taxonomy next to the database
    assert r.returncode != 0 and "taxonomy" in r.stderr and "Loading database" not in r.stderr
    lin = os.path.join(tmp, "lineage.tsv")
    ru.golden_lineage_file(lin)
    r = _run(base + ["--lineage", lin, "-R", os.path.join(tmp, "x")])
    assert r.returncode != 0 and "--rank-report" in r.stderr
    r = _run(base + ["--rank-report", os.path.join(tmp, "r.csv"), "--lineage", lin, "--extended"])
    assert r.returncode != 0 and "--extended" in r.stderr
    open(lin, "w").write("\n".join(f"{n}\t{'X' if n in ('T_alpha', 'T_beta') else 'Y'}\t{'P' if n != 'T_beta' else 'Q'}" for n in gu.target_names()) + "\n")
    r = _run(base + ["--rank-report", os.path.join(tmp, "r.csv"), "--lineage", lin])
    assert r.returncode != 0 and "T_beta" in r.stderr and "Loading database" not in r.stderr
    lo, lr = os.path.join(tmp, "objs.txt"), os.path.join(tmp, "ress.txt")
    open(lo, "w").write(reads + "\n")
    open(lr, "w").write(os.path.join(tmp, "l1") + "\n")
    ru.golden_lineage_file(lin)
    r = _run(base[:-1] + [lo, "-R", lr, "--rank-report", os.path.join(tmp, "r.csv"), "--lineage", lin])
    assert r.returncode != 0 and "list-of-files" in r.stderr
    # the lineage from <DB>/../taxonomy: custom labels stay alone at every level, the report still adds up
    import test_targets_tools as tt
    tt.make_taxonomy(os.path.join(tmp, "taxonomy"))
    r = _run(base + ["--rank-report", os.path.join(tmp, "rt.csv")])
    assert r.returncode == 0, r.stderr
    body = [l.split(",") for l in open(os.path.join(tmp, "rt.csv")).read().splitlines()[1:]]
    assert sum(int(l[4]) for l in body) == 131 and {l[0] for l in body} == {"0", "1", "2", "3", "4", "5", "6", "-"}


@pytest.mark.gpu
def test_cli_rank_report_fallback_batches_counted_once(tmp_path):
    """Reads of mosaic stretches hit more than 64 targets: their batches take the host path, the others are counted on the device;
    the report's total is the number of objects and the report equals the MIC_HOST_INGEST=1 run's."""
    from test_abundance_gpu import _host_path_batches, _synth_db_files
    tmp = str(tmp_path)
    T = 512
    spec, d_sizes, d_keys, d_labels = _synth(T, genome_nt=4_000_000, mosaic_ppm=500, seed=3)
    t, d = _synth_db_files(tmp, spec, d_sizes, d_keys, d_labels, T)
    text, rb = _reads_text(spec, 60000, read_len=300, random_frac=0.05)
    fq = os.path.join(tmp, "reads.fq")
    open(fq, "wb").write(text)
    lin = os.path.join(tmp, "lineage.tsv")
    with open(lin, "w") as f:
        f.write("#label\tgenus\tfamily\n" + "".join(f"L{i}\tg{i // 8}\tf{i // 64}\n" for i in range(T)))
    env = {"MIC_INGEST_KB": "256", "MIC_CLI_TIMING": "1"}
    base = [EXE, "-k", "31", "-T", t, "-D", d, "-O", fq, "--htsize", str(spec.htsize), "--min-confidence", "0.75", "--lineage", lin]
    r1 = _run(base + ["--rank-report", os.path.join(tmp, "r1.csv")], env)
    assert r1.returncode == 0, r1.stderr
    nb, nh = _host_path_batches(r1.stderr)
    assert 0 < nh < nb, r1.stderr
    rep = open(os.path.join(tmp, "r1.csv")).read()
    n = int(re.search(r"\((\d+) objects\)", r1.stdout).group(1))
    assert n == 60000 and sum(int(l.split(",")[4]) for l in rep.splitlines()[1:]) == n
    r2 = _run(base + ["--rank-report", os.path.join(tmp, "r2.csv")], {"MIC_HOST_INGEST": "1"})
    assert r2.returncode == 0, r2.stderr
    assert open(os.path.join(tmp, "r2.csv")).read() == rep
    r3 = _run(base + ["-R", os.path.join(tmp, "o3"), "--rank-report", os.path.join(tmp, "r3.csv")], env)
    assert r3.returncode == 0 and open(os.path.join(tmp, "r3.csv")).read() == rep
    # and estimate_abundance on the extended CSV of the same reads
    r4 = _run(base[:-4] + ["-R", os.path.join(tmp, "o4"), "--extended"], env)
    assert r4.returncode == 0, r4.stderr
    est = _run([EST, "-F", os.path.join(tmp, "o4.csv"), "--rank-report", os.path.join(tmp, "r4.csv"), "--lineage", lin, "-c", "0.75"])
    assert est.returncode == 0 and open(os.path.join(tmp, "r4.csv")).read() == rep
