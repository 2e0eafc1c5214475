"""Reads of two parts on the pipelined road of the per-run query kernel (cuclark_amd/csrc/mic_join2.h, mic_kernels.hip: step, front,
setup) through the C ABI.  Tables of the `tiny` and `tiny_repeats` synthetic workloads for k = 31 on the one-strand and the
two-strand super-k-mer layout, whole and as two slot-range parts each, and `tiny` for k = 27 and k = 32 (the other front half with
constant k and m), against the direct layout, which knows neither windows nor runs: all 8 result words equal on every read.  The
read sets walk the join: one N at every position of a 150-bp read of either strand, two N (three parts, a middle part shorter than
k, adjacent N), joined lengths of 127, 128 and 129 k-mer positions, more runs than one round stages, tandem repeats with an N in
them (crowded runs), and two-part reads between one-part reads, long reads and reads without k-mers.  Every set runs in the
packer's format (reads back to back) and in the terminated one (a 0 behind every read, then whatever the caller left there), the
latter with the parts shorter than k kept, on the full grid and on two blocks (MIC_QUERY_BLOCKS), where one wavefront changes
roads hundreds of times.  Integer work: every comparison is exact."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_strand_bits_gpu import DIRECT, SUPER, SUPER2, MANY_RUNS, _pack, _rc, _synth_db, _synth_spec

pytestmark = pytest.mark.gpu


def _merge_rows(k, T, row_words, rows_list, n):
    """mergeKernel + resultKernel on the device (mic_merge_rows_device / mic_result_from_rows_device) over the parts' sparse rows.
    The engine's stream does not wait for torch's: every buffer torch fills is complete before a kernel of the engine touches it."""
    import torch
    from cuclark_amd import MiClarkDB
    dev = torch.device("cuda:0")
    with MiClarkDB(k, T, row_words=row_words) as e:
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

T = 50
LONG = 190
TABLES = {"k31 tiny": (31, dict(), True), "k31 tiny_repeats": (31, dict(genome_nt=3_000_000, repeat_ppm=50_000), True),
          "k27 tiny": (27, dict(), False), "k32 tiny": (32, dict(), False)}
SETS = ["one N", "two N", "joined lengths", "many runs", "repeats", "interleaved"]


def _genome_reads(spec, n, seed):
    """reads of the generator, 190 nucleotides: genome reads of either strand with substitutions, a fifth random; no N"""
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    rec = L.mic_synth_text_record_bytes(LONG, 1)
    d_text = torch.zeros(n * rec, dtype=torch.uint8, device=dev)
    assert L.mic_synth_reads_text_device(C.byref(spec), seed, n, LONG, 0.2, 0.01, 0.0, 1, -1, d_text.data_ptr(), d_text.numel(), None) == 0
    torch.cuda.synchronize()
    text = d_text.cpu().numpy().reshape(n, rec)
    reads = [bytes(text[r, 12:12 + LONG]) for r in range(n)]
    assert all(set(s) <= set(b"ACGT") for s in reads)
    return reads


def _with_n(s, *at):
    b = bytearray(s)
    for p in at:
        b[p] = ord("N")
    return bytes(b)


def _read_sets(g, k):
    """name -> reads, from 2 000 generator reads g of 190 nucleotides"""
    rng = np.random.default_rng(9)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    sets = {}
    # one N at every position of a 150-bp read, the read and its reverse complement: no part, one part and two parts of every length
    one = []
    for p in range(150):
        for i in range(3):
            s = _with_n(g[(3 * p + i) % len(g)][:150], p)
            one += [s, _rc(s)]
    sets["one N"] = one
    # two N: three parts of at least k, a middle part shorter than k (the read is two parts again, not next to each other), adjacent N,
    # a short first and a short last part
    two = []
    for i in range(600):
        s = g[i][:150]
        a = k + (i * 5) % (150 - 3 * k - 2)
        cuts = ((a, a + k + 1 + (i * 3) % (150 - a - 2 * k - 2)), (a, a + 1 + i % (k - 1)), (a, a + 1), (i % k, a + k), (a, 149 - i % k))[i % 5]
        two.append(_with_n(s, *cuts))
    sets["two N"] = two
    # 127, 128 and 129 k-mer positions joined (len1 + len2 = n + k - 1), the N at every position that leaves two parts with k-mers: the
    # longest ones no longer fit the read-ahead entry
    edges = []
    for n in (127, 128, 129):
        total = n + k - 1
        for p in range(k, total + 1 - k):
            edges.append(_with_n(g[(7 * p + n) % len(g)][:total + 1], p))
    sets["joined lengths"] = edges
    # more than 32 runs: the joined read would need two rounds, it takes the plain road (k = 31: MANY_RUNS was searched for it)
    many = []
    for i in range(900):
        if i % 3 == 0:
            m = (MANY_RUNS, _rc(MANY_RUNS), g[i][:32] + MANY_RUNS[32:])[(i // 3) % 3]
            many.append(_with_n(m, 40 + (i * 7) % 80))
        else:
            many.append(_with_n(g[i][:150], k + i % (150 - 2 * k)) if i % 3 == 1 else g[i][:150])
    sets["many runs"] = many
    # tandem repeats (crowded minimizers on the table with repeats, tied t-mers everywhere) with an N inside and next to the stretch
    tied = []
    for i in range(900):
        unit = rnd(1 + i % 3)
        n = 20 + (i * 7) % 60
        s, p = g[i], 35 + (i * 13) % (150 - n - 70)
        s = (s[:p] + (unit * n)[:n] + s[p + n:])[:150]
        tied.append(_with_n(s, (p + n // 2, p - 1, p + n, p + 3)[i % 4]))
    sets["repeats"] = tied
    # two-part reads between one-part reads, long reads (two chunks), reads without k-mers and reads of three parts
    mixed = []
    for i in range(1200):
        s = g[i]
        mixed.append((_with_n(s[:150], k + (i * 11) % (150 - 2 * k)), s[:150], _with_n(s[:150], 40 + i % 70), s, _with_n(s[:150], 75 + i % 9), s[:k - 1 - i % 7],
                      _with_n(s[:150], 3 + i % 5), b"N" * 40, _with_n(s[:150], 60 + i % 30), _with_n(s, 50, 120), _with_n(s[:120], 60 - i % 30), s[:k])[i % 12])
    sets["interleaved"] = mixed
    assert sorted(sets) == sorted(SETS)
    return sets


def _pack_terminated(reads, k):
    """The same reads with every part kept, those shorter than k too (the kernels skip them), a 0 behind every read and one to three
    containers of anything behind that: the terminated format (include/mi_clark.h: a length slot of 0 ends a read early)."""
    rp, cont = [0], []
    for r, s in enumerate(reads):
        if len(s) >= k:
            for part in s.split(b"N"):
                if not part:
                    continue
                codes = [b"TGCA".index(c) for c in part] + [0] * (-len(part) % 8)
                cont.append(len(part))
                for i in range(0, len(codes), 8):
                    v = 0
                    for c in codes[i:i + 8]:
                        v = v << 2 | c
                    cont.append(v)
        cont.append(0)
        cont += [0x5555 + r % 7] * (1 + r % 3)
        rp.append(len(cont))
    return np.array(rp, np.uint32), np.array(cont, np.uint16)


@pytest.fixture(scope="module", params=sorted(TABLES))
def table(request):
    """the table on the direct layout, on both super-k-mer layouts and (k = 31) as two slot-range parts of each; the read sets packed
    both ways; the direct layout's rows"""
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
        packed = {}
        for name, reads in _read_sets(_genome_reads(spec, 2000, 78), k).items():
            rp, cont = _pack(reads, k)
            packed[name] = ((rp, cont), _pack_terminated(reads, k), engines["direct"].classify_packed(rp, cont))
        yield k, engines, packed


@pytest.mark.parametrize("name", SETS)
def test_rows_equal_the_direct_layouts(name, table, monkeypatch):
    k, engines, packed = table
    packers, terminated, want = packed[name]
    n = want.shape[0]
    assert (want[:, 0] > 0).sum() > n // 4                       # the genome reads hit
    for blocks in (None, "2"):
        if blocks:
            monkeypatch.setenv("MIC_QUERY_BLOCKS", blocks)
        for fmt, (rp, cont) in (("packer's", packers), ("terminated", terminated)):
            for layout in ("super", "super2"):
                res = engines[layout].classify_packed(rp, cont)
                assert (res == want).all(), (layout, fmt, blocks, np.flatnonzero((res != want).any(axis=1))[:10])
                if layout + " parts" not in engines:
                    continue
                hits, rows = np.zeros(n, np.int64), []
                for e in engines[layout + " parts"]:
                    r, w = e.classify_packed(rp, cont, extended=True)
                    hits += r[:, 0]
                    rows.append(w)
                assert (hits == want[:, 0]).all(), (layout, fmt, blocks)     # every k-mer occurrence is counted by exactly one part
                merged, results = _merge_rows(k, T, rows[0].shape[1], rows, n)
                fits = merged[:, 0] != 0xFFFFFFFF
                assert fits.sum() >= n - n // 100 and (results[fits, :5] == want[fits, :5]).all(), (layout, fmt, blocks)
        if blocks:
            monkeypatch.delenv("MIC_QUERY_BLOCKS")
