"""The changes of road of the per-run query kernel (cuclark_amd/csrc/mic_kernels.hip: query_kernel_r - the steady-state loop of the
pipelined road, its entry, the way out of it and back) through the C ABI.  Which road a read takes, and whether a read is pending
while it is taken up, are positions in the kernel's code: what can go wrong is the change between them.  So the read sets are
SEQUENCES OF KINDS of read - no k-mers, length 0, one part, two parts joined, three parts, two chunks, more runs than a round stages,
a crowded run - in which every ordered pair of kinds is adjacent in one wavefront's sequence of reads (on one block, MIC_QUERY_BLOCKS=1,
read r belongs to wavefront r mod 4: every element stands four times), every kind is a wavefront's first and its last read (the
drain), and launches of 1, 3, 4 and 5 reads leave wavefronts with one read, or none.  Tables of the `tiny` workload for k = 31 on the
one-strand and the two-strand super-k-mer layout, whole and as two slot-range parts each, for k = 27 and k = 32 (the other
instantiations with constant k and m) and for k = 28 (k and m from the table: no pipelined road), and `tiny_repeats` for k = 31
(crowded runs; with MIC_CROWD_CAP=0 their reads are flagged and recounted).  Against the direct layout, which knows neither windows
nor runs nor roads: all 8 result words and the sparse rows equal on every read, in the packer's format and in the terminated one, on
one block and on the full grid.  Integer work: every comparison is exact."""
import contextlib
import os

import numpy as np
import pytest

from test_strand_bits_gpu import DIRECT, SUPER, SUPER2, MANY_RUNS, _pack, _synth_db, _synth_spec
from test_two_part_reads_gpu import _genome_reads, _pack_terminated, _with_n
from test_entry_walk_gpu import _kernel_name, _rows_equal

pytestmark = pytest.mark.gpu

T = 50
KINDS = ("no k-mers", "length 0", "one part", "two parts", "three parts", "two chunks", "many runs", "crowded")
SMALL = (1, 3, 4, 5)
# name -> k, generator settings, slot-range parts too
TABLES = {"k31 tiny": (31, dict(), True), "k31 tiny_repeats": (31, dict(genome_nt=3_000_000, repeat_ppm=50_000), True),
          "k27 tiny": (27, dict(), False), "k32 tiny": (32, dict(), False), "k28 tiny": (28, dict(), False)}


def _circuit(n):
    """a closed walk over n kinds that takes every ordered pair (a, b), a == b too, exactly once: n * n + 1 elements, the first again
    at the end (Hierholzer on the complete directed graph with loops)"""
    nxt = [list(range(n)) for _ in range(n)]
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == n * n + 1 and len({(a, b) for a, b in zip(out, out[1:])}) == n * n
    return out


def _read_of(kind, s, k, i, rng, crowded):
    """one read of the kind, made from the generator's read s (190 nucleotides, no N); crowded: reads known to meet a crowded minimizer"""
    if kind == "no k-mers":                     # parts, none of them as long as k
        return (s[:k - 1 - i % 7], _with_n(s[:2 * k - 2], k - 1), b"N" * 40)[i % 3]
    if kind == "length 0":
        return b""
    if kind == "one part":
        return s[:100 + (i * 7) % 51]
    if kind == "two parts":                     # both parts hold k-mers
        return _with_n(s[:150], k + (i * 11) % (150 - 2 * k))
    if kind == "three parts":
        return _with_n(s[:150], k + 2 + i % 9, 150 - k - 3 - i % 7)
    if kind == "two chunks":
        return s[:k + 130]
    if kind == "many runs":                     # (searched for k = 31: more than 32 runs; at another k it is a read like any other)
        return (MANY_RUNS, MANY_RUNS[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")), s[:32] + MANY_RUNS[32:])[i % 3]
    assert kind == "crowded"
    if crowded:
        return crowded[i % len(crowded)]
    # a table without crowded minimizers: a tandem repeat inside a genome read (test_two_part_reads_gpu: "repeats"), tied t-mers everywhere
    unit = bytes(rng.choice(list(b"ACGT"), 1 + i % 3).astype(np.uint8))
    n = 40 + (i * 7) % 40
    p = 35 + (i * 13) % (150 - n - 70)
    return (s[:p] + (unit * n)[:n] + s[p + n:])[:150]


def _launches(g, k, crowded):
    """the launches of a set as lists of reads: per kind the closed walk over the kinds turned so that it starts and ends with that kind,
    every element four times; and the first 1, 3, 4 and 5 reads of a walk that starts with one-part reads"""
    rng = np.random.default_rng(12)
    walk = _circuit(len(KINDS))
    out, i = [], 0
    for first in range(len(KINDS)):
        at = walk.index(first)
        turned = walk[at:-1] + walk[:at] + [first]
        assert turned[0] == turned[-1] == first and len({(a, b) for a, b in zip(turned, turned[1:])}) == len(KINDS) ** 2
        reads = []
        for kind in turned:
            for _ in range(4):
                reads.append(_read_of(KINDS[kind], g[i % len(g)], k, i, rng, crowded))
                i += 1
        out.append(reads)
    for n in SMALL:
        out.append([_read_of(("one part", "two parts", "one part", "crowded", "one part")[j], g[(i + j) % len(g)], k, i + j, rng, crowded) for j in range(n)])
    return out


def _pack_both(reads, k):
    """packer's format and terminated format.  A read of length 0 has no line of its own in FASTA text: the packer is given an N in its
    place - no part either - and the packed form is checked to be the empty range of a read without parts."""
    rp, cont = _pack([s if s else b"N" for s in reads], k)
    for r, s in enumerate(reads):
        if not s:
            assert rp[r + 1] == rp[r]
    return (rp, cont), _pack_terminated(reads, k)


def _merge(e, rows_list, n):
    """mergeKernel + resultKernel on the device over the parts' sparse rows (test_two_part_reads_gpu._merge_rows, on an engine kept
    for the table's lifetime)"""
    import torch
    dev = torch.device("cuda:0")
    acc = torch.from_numpy(rows_list[0].astype(np.int64)).to(dev).to(torch.int32).contiguous()
    for rows in rows_list[1:]:
        nxt = torch.from_numpy(rows.astype(np.int64)).to(dev).to(torch.int32).contiguous()
        out = torch.empty_like(acc)
        torch.cuda.synchronize()
        e.merge_rows_device(acc.data_ptr(), nxt.data_ptr(), out.data_ptr(), n)
        e.sync()
        acc = out
    results = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.result_from_rows_device(acc.data_ptr(), results.data_ptr(), n)
    e.sync()
    return acc.cpu().numpy().view(np.uint32), results.cpu().numpy().view(np.uint32)


def _query_and_resolve(e, rp, cont, n, flags=None):
    """the two calls of classify_packed apart: the crowd statistics of the query, and the reads the dense path recounted (flags: a list
    that receives the result rows' flag words as the query left them)"""
    import torch
    dev = torch.device("cuda:0")
    d_rp = torch.from_numpy(rp.view(np.int32)).to(dev)
    d_ct = torch.from_numpy(np.concatenate([cont, np.zeros(64, np.uint16)]).view(np.int16)).to(dev)
    d_res = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.query_device(d_rp.data_ptr(), d_ct.data_ptr(), n, d_res.data_ptr())
    st = e.last_crowd_stats()
    if flags is not None:
        e.sync()
        flags.append(d_res.cpu().numpy().view(np.uint32)[:, 6].copy())
    dense = e.resolve_flagged_device(d_rp.data_ptr(), d_ct.data_ptr(), d_res.data_ptr())
    return d_res.cpu().numpy().view(np.uint32), st, dense


@pytest.fixture(scope="module", params=sorted(TABLES))
def table(request):
    """the table on the direct layout, on both super-k-mer layouts and (k = 31) as two slot-range parts of each; the launches packed
    both ways; the direct layout's results and rows, computed once"""
    from cuclark_amd import MiClarkDB
    k, kw, parts = TABLES[request.param]
    spec = _synth_spec(k, **kw)
    d_sizes, d_keys, d_labels, n_el = _synth_db(spec)
    with contextlib.ExitStack() as stack:
        def engine(layout, part=None):
            e = stack.enter_context(MiClarkDB(k, T, layout=layout))
            if part is not None:
                e.set_part(part, 2)
            e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
            assert e.info()["layout"] == layout and e.info()["n_parts"] == (0 if part is None else 2)
            return e
        engines = {"direct": engine(DIRECT), "super": engine(SUPER), "super2": engine(SUPER2)}
        if parts:
            engines.update({"super parts": [engine(SUPER, 0), engine(SUPER, 1)], "super2 parts": [engine(SUPER2, 0), engine(SUPER2, 1)]})
        for layout in ("super", "super2"):
            generic = _kernel_name(engines[layout]).startswith("query_kernel_r<0, 0,")
            assert generic == (k == 28), _kernel_name(engines[layout])
        # the reads of the generator that meet a crowded minimizer: those the per-run kernel flags when it has no work area to hand their
        # runs over (only the table with repeats has any)
        g = _genome_reads(spec, 2200, 81)
        crowded = []
        if "repeats" in request.param:
            # (microsatellites are rare in the generator's genomes: a few reads in a thousand overlap one)
            cand = [s[:150] for s in _genome_reads(spec, 40_000, 82)]
            rp, cont = _pack(cand, k)
            flags = []
            _, st, _ = _query_and_resolve(engines["super"], rp, cont, len(cand))
            os.environ["MIC_CROWD_CAP"] = "0"
            try:
                _query_and_resolve(engines["super"], rp, cont, len(cand), flags)
            finally:
                del os.environ["MIC_CROWD_CAP"]
            crowded = [cand[r] for r in np.flatnonzero(flags[0])]
            print(request.param, "reads with crowded runs among the generator's:", len(crowded), "crowd statistics:", st)
            assert len(crowded) >= 8 and len(crowded) >= st["reads"], (len(crowded), st)
        packed = []
        for reads in _launches(g, k, crowded):
            packers, terminated = _pack_both(reads, k)
            want, want_rows = engines["direct"].classify_packed(*packers, extended=True)
            assert want.shape[0] == len(reads)
            packed.append((packers, terminated, want, want_rows))
        assert 1900 <= sum(p[2].shape[0] for p in packed) <= 2200       # about two thousand reads per set
        merger = stack.enter_context(MiClarkDB(k, T, row_words=packed[0][3].shape[1]))
        yield request.param, k, engines, merger, packed


@pytest.mark.parametrize("blocks", [None, "1"], ids=["full grid", "one block"])
@pytest.mark.parametrize("fmt", ["packer's", "terminated"])
def test_rows_equal_the_direct_layouts_across_every_change_of_road(fmt, blocks, table, monkeypatch):
    name, k, engines, merger, packed = table
    if blocks:
        monkeypatch.setenv("MIC_QUERY_BLOCKS", blocks)
    big = [p for p in packed if p[2].shape[0] > max(SMALL)]
    assert len(big) == len(KINDS) and sorted(p[2].shape[0] for p in packed if p[2].shape[0] <= max(SMALL)) == sorted(SMALL)
    assert sum(int((p[2][:, 0] > 0).sum()) for p in big) > sum(p[2].shape[0] for p in big) // 3      # the genome reads hit
    for li, (packers, terminated, want, want_rows) in enumerate(packed):
        rp, cont = packers if fmt == "packer's" else terminated
        n = want.shape[0]
        for layout in ("super", "super2"):
            res, rows = engines[layout].classify_packed(rp, cont, extended=True)
            assert (res == want).all(), (name, layout, li, np.flatnonzero((res != want).any(axis=1))[:10])
            assert _rows_equal(rows, want_rows), (name, layout, li)
            if layout + " parts" not in engines:
                continue
            hits, part_rows = np.zeros(n, np.int64), []
            for e in engines[layout + " parts"]:
                r, w = e.classify_packed(rp, cont, extended=True)
                hits += r[:, 0]
                part_rows.append(w)
            assert (hits == want[:, 0]).all(), (name, layout, li)            # every k-mer occurrence is counted by exactly one part
            merged, results = _merge(merger, part_rows, n)
            fits = merged[:, 0] != 0xFFFFFFFF
            assert fits.sum() >= n - n // 50 and (results[fits, :5] == want[fits, :5]).all(), (name, layout, li)
        if "repeats" not in name:
            continue
        # The crowded kind is one on this table: its runs go to the follow-up kernel from either road, pending or not; without a work
        # area (MIC_CROWD_CAP=0) their reads are flagged, the dense path recounts them, and the rows are the direct layout's.
        for layout in ("super", "super2"):
            res, st, dense = _query_and_resolve(engines[layout], rp, cont, n)
            assert (res == want).all(), (layout, li, np.flatnonzero((res != want).any(axis=1))[:10])
            if n > max(SMALL):
                assert st["runs"] >= st["reads"] >= 32 and st["reads_to_dense_path"] == 0 and dense == 0, (layout, li, st, dense)
            handed = int(st["reads"])
            monkeypatch.setenv("MIC_CROWD_CAP", "0")
            flags = []
            res, st0, dense = _query_and_resolve(engines[layout], rp, cont, n, flags)
            monkeypatch.delenv("MIC_CROWD_CAP")
            # (a read the dense path recounted says so in its flag word, word 6: its counts, labels and number of labels are the direct
            # layout's; every other read is untouched, all 8 words)
            flagged = flags[0] != 0
            assert (res[:, :6] == want[:, :6]).all(), (layout, li, "no work area", np.flatnonzero((res[:, :6] != want[:, :6]).any(axis=1))[:10])
            assert (res[~flagged] == want[~flagged]).all() and (res[flagged, 6] != 0).all(), (layout, li, "no work area")
            assert int(flagged.sum()) == dense >= handed and (dense > 0) == (handed > 0), (layout, li, st, st0, dense)
