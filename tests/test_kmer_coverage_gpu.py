"""The table census on the MI355X (csrc/mic_census.h: the rule): census_kernel - every k-mer of the database probed through the
resident table - against mic_db_census_host and against the oracle's count (every k-mer of the file looked up in the oracle's
database, counted by the label found), on every table layout, on crowded minimizers, on parts and shards of a table, on both counting
roads; mic_db_census_device on torch tensors; exe/cuCLARK --kmer-coverage on every input route."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import kcoverage_util as kc
import ksketch_util as ku
from test_kmer_coverage import malformed_db

EXE = os.path.join(gu.ROOT, "exe", "cuCLARK")
LAYOUTS = {"direct": 1, "minimizer": 2, "super": 3, "super2": 4}       # MIC_LAYOUT_*
GOLDEN_DBS = {20: "light_k20_u16", 27: "light_k27_u32", 31: "light_k31_u64", 32: "light_k32_u64"}      # tests/test_kmer_report_gpu.py's
T6 = 6
TILE = 256
FULL_K31 = [2129, 5344, 2936, 5169, 2878, 2560]            # k-mers per label of full_k31_u32
LIGHT_K27_S3 = [757, 1783, 966, 1730, 939, 877]            # of light_k27_u32 at sampling 3


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, capture_output=True, text=True, timeout=300, env=e, **kw)


def _load(k, T, layout, arrays, sampling=1, part=None, shard=(0, 0), census=True):
    """(counts, stats, info, build report) of a table loaded with the census on"""
    from cuclark_amd import MiClarkDB
    with MiClarkDB(k, T, layout=LAYOUTS[layout]) as e:
        if part:
            e.set_part(*part)
        if census:
            e.census_enable()
        e.read_arrays(*arrays, sampling, shard)
        counts, stats = e.census_fetch()
        return counts, stats, e.info(), e.L.mic_db_last_build_report().decode()


def _healthy(counts, stats, info, want, what):
    assert (counts == want[0]).all(), (what, counts, want[0])
    assert [int(v) for v in stats] == [int(v) for v in want[1]], (what, stats, want[1])
    assert int(stats[3]) == 0 and int(stats[1]) == 0 and int(stats[0]) == info["n_elems"], (what, stats, info["n_elems"])
    assert int(counts.sum()) == int(stats[0]) - int(stats[4]), what


@pytest.fixture(scope="module")
def golden():
    """per (k, sampling): the arrays of the golden database, the host census and the oracle's count (one reference for the tests below)"""
    from cuclark_amd import host
    out = {}
    for k, name in GOLDEN_DBS.items():
        db = gu.load_golden_db(name)
        arrays = (gu.golden_sizes(db), db["ky"], db["lb"])
        for sampling in (1, 3):
            out[k, sampling] = dict(arrays=arrays, host=host.db_census(*arrays, k, T6, sampling), oracle=kc.oracle_counts(*arrays, k, T6, sampling))
    return out


# ---- every layout, every golden k ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sampling", [1, 3])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", list(GOLDEN_DBS))
def test_census_on_the_golden_databases(golden, k, layout, sampling):
    g = golden[k, sampling]
    counts, stats, info, report = _load(k, T6, layout, g["arrays"], sampling)
    _healthy(counts, stats, info, g["host"], (k, layout, sampling))
    want, found, n_elems = g["oracle"]
    assert (counts == want).all() and int(stats[0]) == found == n_elems > (5000 if sampling == 3 else 20000)
    if (k, sampling) == (27, 3):
        assert [int(v) for v in counts] == LIGHT_K27_S3
    assert info["layout"] == LAYOUTS[layout] and "\ncensus: " in report


# ---- crowded minimizers: the side table, palindromic repeats ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowded():
    from cuclark_amd import host
    from test_crowded import _microsatellite_db
    out = {}
    for k in (31, 32):
        T = 12
        _, sizes, keys, labels = _microsatellite_db(np.random.default_rng(41 + k), k, 1 << 18, T)
        out[k] = dict(T=T, arrays=(sizes, keys, labels), host=host.db_census(sizes, keys, labels, k, T))
    # the palindromic units of test_crowded.test_palindromic_repeats_at_even_k: a k-mer the one-strand table would store twice
    T = 9
    _, sizes, keys, labels = _microsatellite_db(np.random.default_rng(7308 + 32 + 400), 32, 1 << 14, T, n_sites=400, units=("GC", "AT", "ACGT", "AGCT", "AC"))
    out["palindromic"] = dict(T=T, arrays=(sizes, keys, labels), host=host.db_census(sizes, keys, labels, 32, T))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["super", "super2"])
@pytest.mark.parametrize("case", [31, 32, "palindromic"])
def test_census_on_crowded_minimizers(crowded, case, layout):
    c = crowded[case]
    k = 32 if case == "palindromic" else case
    counts, stats, info, _ = _load(k, c["T"], layout, c["arrays"])
    assert info["side_kmers"] > (0 if case == "palindromic" else 500), info["side_kmers"]          # the precondition: the side table is in use
    _healthy(counts, stats, info, c["host"], (case, layout))
    assert int(stats[0]) == c["arrays"][1].size > 10000                      # every k-mer of the file, each counted once


# ---- parts and shards -------------------------------------------------------------------------------------------------------------
def _device_census(e, arrays, T, sampling=1, shard=(0, 0), calls=1):
    """mic_db_census_device on torch tensors of the whole images"""
    import torch
    dev = torch.device("cuda:0")
    sizes, keys, labels = (np.ascontiguousarray(a) for a in arrays)
    signed = {2: np.int16, 4: np.int32, 8: np.int64}[keys.dtype.itemsize]
    d_sz = torch.from_numpy(sizes).to(dev)
    d_ky = torch.from_numpy(np.concatenate([keys, np.zeros(8, keys.dtype)]).view(signed)).to(dev)
    d_lb = torch.from_numpy(np.concatenate([labels, np.zeros(8, np.uint16)]).view(np.int16)).to(dev)
    d_counts = torch.zeros(max(T, 1), dtype=torch.int64, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for _ in range(calls):
        e.census_device(d_sz.data_ptr(), sizes.size, d_ky.data_ptr(), keys.dtype.itemsize, d_lb.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(),
                        sampling, shard)
    e.sync()
    return d_counts.cpu().numpy().view(np.uint64)[:T], d_stats.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["2 parts", "3 parts", "2 shards"])
@pytest.mark.parametrize("layout", ["super", "direct"])
def test_census_of_parts_and_shards(layout, cut):
    """super: mic_db_set_part cuts the resident table by slot range and every part sees the whole images - the k-mers of the other
    parts are stats[1]; direct: the cut is a bucket range and a part's load sees its own buckets only, so stats[1] shows when the
    WHOLE images are counted against the part's table (mic_db_census_device).  Either way every k-mer is `mine` on exactly one part."""
    from cuclark_amd import MiClarkDB, host
    k, htsize = 25, 10007
    arrays = gu.random_db(np.random.default_rng(5), htsize, 20000, k, 8, T6)[:3]
    whole = _load(k, T6, layout, arrays)
    _healthy(*whole[:3], host.db_census(*arrays, k, T6), layout)
    assert int(whole[1][0]) == 20000
    cuts = {"2 parts": [dict(part=(p, 2)) for p in range(2)], "3 parts": [dict(part=(p, 3)) for p in range(3)],
            "2 shards": [dict(shard=(0, htsize // 2)), dict(shard=(htsize // 2, htsize))]}
    for cut in [cuts[cut]]:
        total, found = np.zeros(T6, np.uint64), 0
        for kw in cut:
            with MiClarkDB(k, T6, layout=LAYOUTS[layout]) as e:
                if "part" in kw:
                    e.set_part(*kw["part"])
                e.census_enable()
                e.read_arrays(*arrays, 1, kw.get("shard", (0, 0)))
                counts, stats = e.census_fetch()
                assert int(counts.sum()) == int(stats[0]) - int(stats[4]) and int(stats[3]) == 0 and 0 < int(stats[0]) < int(whole[1][0]), (kw, stats)
                by_slots = layout == "super" and "part" in kw
                assert (int(stats[1]) > 0) == by_slots, (kw, stats)
                assert int(stats[0]) + int(stats[1]) == (int(whole[1][0]) if by_slots else e.info()["n_elems"])
                # the whole images against this part's table: the same counts, the others' k-mers in stats[1]
                d_counts, d_stats = _device_census(e, arrays, T6)
                assert (d_counts == counts).all() and int(d_stats[0]) == int(stats[0]) and int(d_stats[3]) == 0, (kw, d_stats)
                assert int(d_stats[1]) == int(whole[1][0]) - int(stats[0]) > 0, (kw, d_stats)
            total += counts
            found += int(stats[0])
        assert (total == whole[0]).all() and found == int(whole[1][0]), (layout, cut)


# ---- many targets: the two counting roads, a bucket of 255, a table that is no multiple of the tile ---------------------------------
def _bucket_db(rng, htsize, k, T, big):
    """a well-formed database with 0 .. 8 canonical k-mers per bucket and 255 in bucket `big`"""
    sizes, keys = np.zeros(htsize, np.uint8), []
    top = (1 << (2 * k)) // htsize - 1
    for b in range(htsize):
        n = 255 if b == big else int(rng.integers(0, 9))
        kv = np.unique(rng.integers(0, top, 4 * n + 16, dtype=np.uint64))
        c = kv * np.uint64(htsize) + np.uint64(b)
        kv = kv[ku.canonical_np(c, k) == c][:n]
        assert kv.size == n
        sizes[b] = n
        keys.append(kv)
    keys = np.concatenate(keys)
    return sizes, keys, rng.integers(0, T, keys.size).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [8192, 8193, 40000])
def test_census_with_many_targets(T):
    """8192 targets: the last table size counted in the LDS histogram; 8193: the first on the wave-aggregated road"""
    from cuclark_amd import host
    rng = np.random.default_rng(21 + T)
    k = 25
    sizes, keys, labels, canon = gu.random_db(rng, 10007, 20000, k, 8, T)
    want = host.db_census(sizes, keys, labels, k, T)
    assert int(want[1][0]) == canon.size and int(want[0].max()) >= 4 and int(np.count_nonzero(want[0])) > (5000 if T < 40000 else 15000)
    for layout in ("direct", "super"):
        counts, stats, info, _ = _load(k, T, layout, (sizes, keys, labels))
        _healthy(counts, stats, info, want, (T, layout))
    if T == 40000:
        return
    for htsize in (TILE - 1, TILE + 1):
        arrays = _bucket_db(rng, htsize, k, T, big=htsize - 2)
        arrays[2][: 40] = T - 1                                              # the last target's counter
        want = host.db_census(*arrays, k, T)
        assert int(want[1][0]) == arrays[1].size > 255 + 500 and int(want[0][T - 1]) >= 40 and int(arrays[0].max()) == 255
        for layout in ("direct", "minimizer", "super", "super2"):
            counts, stats, info, _ = _load(k, T, layout, arrays)
            _healthy(counts, stats, info, want, (T, htsize, layout))
    # labels at and above the engine's targets: found, in stats[4], in no counts entry
    few = T // 2
    want = host.db_census(*arrays, k, few)
    counts, stats, info, _ = _load(k, few, "super", arrays)
    _healthy(counts, stats, info, want, (T, "half the targets"))
    assert int(stats[4]) > 100 and int(stats[0]) == arrays[1].size


# ---- caller-owned images; the option off -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["direct", "super2"])
def test_census_device_and_option_off(golden, layout):
    from cuclark_amd import MiClarkDB
    from cuclark_amd._lib import MicError
    k = 27
    for sampling in (1, 3):
        g = golden[k, sampling]
        with MiClarkDB(k, T6, layout=LAYOUTS[layout]) as e:
            e.read_arrays(*g["arrays"], sampling)
            with pytest.raises(MicError) as err:            # not enabled at load: nothing was counted, nothing to fetch
                e.census_fetch()
            assert err.value.code == -5                     # MIC_E_STATE
            off_report = e.L.mic_db_last_build_report().decode()
            assert "census" not in off_report and "table build, total: " in off_report
            with pytest.raises(MicError) as err:            # a table is loaded: too late to enable
                e.census_enable()
            assert err.value.code == -5
            once = _device_census(e, g["arrays"], T6, sampling)
            assert (once[0] == g["host"][0]).all() and (once[1] == g["host"][1]).all()
            twice = _device_census(e, g["arrays"], T6, sampling, calls=2)
            assert (twice[0] == 2 * g["host"][0]).all() and (twice[1] == 2 * g["host"][1]).all()
            # halves of the buckets add up to the whole
            h = g["arrays"][0].size // 2
            a, b = _device_census(e, g["arrays"], T6, sampling, (0, h)), _device_census(e, g["arrays"], T6, sampling, (h, 0))
            assert (a[0] + b[0] == g["host"][0]).all() and int(a[1][0]) > 0 and int(b[1][0]) > 0
        on_report = _load(k, T6, layout, g["arrays"], sampling)[3]
        # with the option on: the parent's lines and one more
        strip = lambda rep: [ln.split(":")[0] for ln in rep.splitlines()]
        assert strip(on_report) == strip(off_report) + ["census"], (on_report, off_report)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, 7])
def test_census_on_malformed_buckets(k):
    """the direct layout answers like the reference's scan (tests/test_gpu_parity.py): the census gives the oracle's counts; at k = 7
    the same arrays hold k-mers above their reverse complement (tests/test_kmer_coverage.py: why k = 20 has none)"""
    from cuclark_amd import host
    sizes, keys, labels, k, T = malformed_db(k)
    want, found, _ = kc.oracle_counts(sizes, keys, labels, k, T)
    counts, stats, info, _ = _load(k, T, "direct", (sizes, keys, labels))
    hc, hs = host.db_census(sizes, keys, labels, k, T)
    assert (counts == want).all() and (counts == hc).all() and (stats == hs).all()
    assert int(stats[0]) == found > 100 and int(stats[3]) == 0 and ((int(stats[2]) > 0) if k == 7 else (int(stats[2]) == 0))


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _parse(report):
    lines = report.splitlines()
    assert lines[0] == kc.HEADER
    return {f[0]: f[1:] for f in (ln.split(",") for ln in lines[1:])}


@pytest.fixture(scope="module")
def cli_db(tmp_path_factory):
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path_factory.mktemp("kmer_coverage_db"))
    return _targets_file(tmp), _db_dir(tmp, "full_k31_u32", light=False)


@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["fq", "pairs"])
def test_cli_kmer_coverage(tmp_path, cli_db, inp):
    """every route of one input writes the same bytes: -n 1, -n 4, --extended (the batch API), a compressed file, without -R; the
    first five columns are --kmer-report's of the same run, TargetKmers the golden counts, Coverage the restatement; the result CSV
    does not change with the option"""
    tmp = str(tmp_path)
    t, dbd = cli_db
    o = lambda n: os.path.join(tmp, n)
    env = {"MIC_INGEST_KB": "64"}
    gz = lambda src, dst: gzip.open(dst, "wb").write(open(src, "rb").read())
    if inp == "pairs":
        f1, f2 = os.path.join(gu.GOLDEN, "pairs_k31_1.fq"), os.path.join(gu.GOLDEN, "pairs_k31_2.fq")
        gz(f1, o("p1.fq.gz")); gz(f2, o("p2.fq.gz"))
        plain, packed = ["-P", f1, f2], ["-P", o("p1.fq.gz"), o("p2.fq.gz")]
    else:
        f = os.path.join(gu.GOLDEN, "reads_k31.fq")
        gz(f, o("in.fq.gz"))
        plain, packed = ["-O", f], ["-O", o("in.fq.gz")]
    base = [EXE, "-k", "31", "-T", t, "-D", dbd]
    routes = {"n1": plain + ["-n", "1", "-R", o("r_n1")], "gz": packed + ["-n", "4", "-R", o("r_gz")]}
    if inp == "fq":
        routes.update({"n4": plain + ["-n", "4", "-R", o("r_n4")], "extended": plain + ["--extended", "-R", o("r_ext")], "alone": plain + ["-n", "4"]})
    reports = {}
    for name, args in routes.items():
        both = name != "alone"                                  # (alone: no -R and no --kmer-report next to it)
        r = _run(base + args + ["--kmer-coverage", o(f"c_{name}.csv")] + (["--kmer-report", o(f"k_{name}.csv")] if both else []), env)
        assert r.returncode == 0 and " - K-mer coverage report stored in " + o(f"c_{name}.csv") in r.stdout, (name, r.stderr)
        reports[name] = open(o(f"c_{name}.csv")).read()
        assert ("Results stored" in r.stdout) == both, name
        if both:
            kr = open(o(f"k_{name}.csv")).read().splitlines()
            assert [",".join(ln.split(",")[:5]) for ln in reports[name].splitlines()] == kr, name
    for name, rep in reports.items():
        assert rep == reports["n1"], name
    # the result CSV does not change with the option
    r = _run(base + plain + ["-n", "1", "-R", o("r0")], env)
    assert r.returncode == 0, r.stderr
    assert open(o("r0.csv"), "rb").read() == open(o("r_n1.csv"), "rb").read()
    names = gu.target_names()
    got = _parse(reports["n1"])
    assert len(got) >= 3 and set(got) <= set(names)
    for nm, (reads, kmers, distinct, dup, tk, cov) in got.items():
        assert int(tk) == FULL_K31[names.index(nm)], nm
        assert cov == kc.ratio6(min(int(distinct), int(tk)), int(tk)) and 0.0 < float(cov) <= 1.0, nm


@pytest.mark.gpu
def test_cli_kmer_coverage_with_sampling(tmp_path):
    """-s 3: the coverage is relative to the sampled (resident) k-mers"""
    from test_cli import _db_dir, _targets_file
    tmp = str(tmp_path)
    t, dbd = _targets_file(tmp), _db_dir(tmp, "light_k27_u32", light=False)
    base = [EXE, "-k", "27", "--htsize", "57777779", "-T", t, "-D", dbd, "-O", os.path.join(gu.GOLDEN, "reads_k27.fq")]
    names = gu.target_names()
    tks = {}
    for s in ("1", "3"):
        out = os.path.join(tmp, f"c{s}.csv")
        r = _run(base + (["-s", s] if s != "1" else []) + ["--kmer-coverage", out])
        assert r.returncode == 0, r.stderr
        tks[s] = {nm: int(f[4]) for nm, f in _parse(open(out).read()).items()}
    assert len(tks["3"]) >= 3
    for nm, tk in tks["3"].items():
        assert tk == LIGHT_K27_S3[names.index(nm)] and tk < tks["1"][nm], nm
