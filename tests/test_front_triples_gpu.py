"""The three-t-mers-per-lane front half of the per-run query kernel (k = 31, m = 20; cuclark_amd/csrc/mic_front3.h, mic_kernels.hip:
sampled_positions3) through the C ABI.  Tables of the `tiny` and `tiny_repeats` synthetic workloads on the one-strand and the
two-strand super-k-mer layout, whole and as two slot-range parts each - the four instantiations that run the new form -, against
the direct layout, which has no front half: equal result rows on every read.  The read sets walk the new index arithmetic: every
chunk size and both chunks of a long part, parts of two, an N next to the edges of lanes' triples, tied t-mers, more runs than one
round stages, both strands.  Every set runs on the full grid and on two blocks (MIC_QUERY_BLOCKS), where each wavefront takes
hundreds of reads of mixed shape through the pipelined loop.  Integer work: every comparison is exact."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_strand_bits_gpu import DIRECT, SUPER, SUPER2, MANY_RUNS, _pack, _rc, _synth_db, _synth_spec
from test_table_parts import _merge_rows

pytestmark = pytest.mark.gpu

K, T = 31, 50
TABLES = {"tiny": dict(), "tiny_repeats": dict(genome_nt=3_000_000, repeat_ppm=50_000)}
LONG = 190          # 160 k-mers: a chunk of 128 and one of 32, base > 0


def _genome_reads(spec, n, seed):
    """reads of the generator: genome reads of either strand with substitutions and N, a fifth random"""
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    rec = L.mic_synth_text_record_bytes(LONG, 1)
    assert rec == LONG + 13
    d_text = torch.zeros(n * rec, dtype=torch.uint8, device=dev)
    assert L.mic_synth_reads_text_device(C.byref(spec), seed, n, LONG, 0.2, 0.01, 0.002, 1, -1, d_text.data_ptr(), d_text.numel(), None) == 0
    torch.cuda.synchronize()
    text = d_text.cpu().numpy().reshape(n, rec)
    reads = [bytes(text[r, 12:12 + LONG]) for r in range(n)]
    assert all(set(s) <= set(b"ACGTN") for s in reads)
    return reads


def _read_sets(g):
    """name -> about 2 000 reads, from 2 000 generator reads g of 190 nucleotides"""
    rng = np.random.default_rng(8)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    sets = {}
    # every number of k-mers from 1 to 160: all chunk sizes, the third t-mer of a lane's triple on either side of the part's end, a
    # second chunk of 1 .. 32 k-mers
    sets["lengths"] = [g[(12 * (n - K) + i) % len(g)][:n] for n in range(K, LONG + 1) for i in range(12)]
    # two parts in one object, of every length between them
    sets["two parts"] = [g[i][:K - 5 + i % 130] + b"N" + g[i + 1][:K + (7 * i) % 140] for i in range(0, 1998)]
    # one N at positions 3a-1 .. 3a+3 around several lanes, around k-mer 128 and around the last t-mers of the first chunk; two N
    at = [3 * a + d for a in (1, 7, 16, 33, 42, 43, 50) for d in range(-1, 4)] + list(range(125, 132)) + list(range(148, 162))
    cut = []
    for i, p in enumerate(at * 36):
        s = bytearray(g[i % len(g)])
        s[p] = ord("N")
        if i % 9 == 0:
            s[(p + 31 + i % 40) % LONG] = ord("N")
        cut.append(bytes(s[:150 + 40 * (i % 2)]))
    sets["N at the edges of triples"] = cut
    # tied t-mers: homopolymers and di- / trinucleotide repeats, alone and inside genome reads (where the table's k-mers around them hit)
    tied = []
    for i in range(2000):
        unit = rnd(1 + i % 3)
        n = 10 + (i * 7) % 60
        stretch = (unit * n)[:n]
        if i % 4 == 3:
            tied.append((unit * LONG)[:K + (i * 3) % (LONG - K + 1)])
        else:
            s, p = g[i], (i * 13) % (LONG - n)
            tied.append((s[:p] + stretch + s[p + n:])[:150 + 40 * (i % 2)])
    sets["repeats"] = tied
    # more than 32 runs in a chunk (two rounds of staged slots), between reads that take the pipelined road
    many = []
    for i in range(2000):
        if i % 8 == 0:
            many.append((MANY_RUNS, _rc(MANY_RUNS), MANY_RUNS + g[i][:40], _rc(MANY_RUNS + g[i][:40]), g[i][:32] + MANY_RUNS[32:])[(i // 8) % 5])
        else:
            many.append(g[i][:150])
    sets["many runs"] = many
    # genome reads and their reverse complements
    sets["strands"] = [s for r in g[:1000] for s in (r[:150], _rc(r[:150]))]
    assert all(1900 <= len(v) <= 2100 for v in sets.values())
    return sets


@pytest.fixture(scope="module", params=sorted(TABLES))
def table(request):
    """the table on every layout: direct, super, super2, and the two super layouts as two slot-range parts"""
    from cuclark_amd import MiClarkDB
    spec = _synth_spec(K, **TABLES[request.param])
    d_sizes, d_keys, d_labels, n_el = _synth_db(spec)
    with contextlib.ExitStack() as stack:
        def engine(layout, part=None):
            e = stack.enter_context(MiClarkDB(K, T, layout=layout))
            if part is not None:
                e.set_part(part, 2)
            e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
            assert e.info()["layout"] == layout and e.info()["n_parts"] == (0 if part is None else 2)
            return e
        engines = {"direct": engine(DIRECT), "super": engine(SUPER), "super2": engine(SUPER2),
                   "super parts": [engine(SUPER, 0), engine(SUPER, 1)], "super2 parts": [engine(SUPER2, 0), engine(SUPER2, 1)]}
        yield engines, _read_sets(_genome_reads(spec, 2000, 77))


@pytest.mark.parametrize("name", ["lengths", "two parts", "N at the edges of triples", "repeats", "many runs", "strands"])
def test_rows_equal_the_direct_layouts(name, table, monkeypatch):
    engines, sets = table
    rp, cont = _pack(sets[name], K)
    n = rp.size - 1
    want = engines["direct"].classify_packed(rp, cont)
    assert (want[:, 0] > 0).sum() > n // 3                       # the genome reads hit
    for blocks in (None, "2"):
        if blocks:
            monkeypatch.setenv("MIC_QUERY_BLOCKS", blocks)
        for layout in ("super", "super2"):
            res = engines[layout].classify_packed(rp, cont)
            assert (res[:, :5] == want[:, :5]).all(), (layout, blocks, np.flatnonzero((res[:, :5] != want[:, :5]).any(axis=1))[:10])
            if name == "strands":
                assert (res[0::2] == res[1::2]).all()             # a read and its reverse complement
            hits, rows = np.zeros(n, np.int64), []
            for e in engines[layout + " parts"]:
                r, w = e.classify_packed(rp, cont, extended=True)
                hits += r[:, 0]
                rows.append(w)
            assert (hits == want[:, 0]).all(), (layout, blocks)   # every k-mer occurrence is counted by exactly one part
            merged, results = _merge_rows(K, T, rows[0].shape[1], rows, n)
            fits = merged[:, 0] != 0xFFFFFFFF
            assert fits.sum() >= n - n // 100 and (results[fits, :5] == want[fits, :5]).all(), (layout, blocks)
        if blocks:
            monkeypatch.delenv("MIC_QUERY_BLOCKS")
