"""Every k from 12 to 32 with the default minimizer length, and the (k, MIC_MINIMIZER_LEN) of tests/test_k_sweep.py that reach the
remaining branches of the query kernels' front half, against the oracle through the C ABI: a table of every k-mer of a random genome
with planted tandem repeats (tied t-mers in k-mers that hit), reads of every length around the chunk edge, one N at every position,
substitutions, several chunks and the repeats - on the minimizer layout and both super-k-mer layouts, on the full grid and on two
blocks, whole and (where the launcher routes parts elsewhere) as two slot-range parts.  mic_db_kernel_name must name the
instantiation that test_k_sweep.py's restatement of the launcher predicts.  Integer work: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import golden_util as gu
import test_k_sweep as ks
from test_k_sweep import DIRECT, MINIMIZER, SUPER, SUPER2
from test_strand_bits_gpu import _rc
from test_table_parts import _db_of_codes, _merge_rows, _oracle_part, _reads_from

pytestmark = pytest.mark.gpu

T, ROW_WORDS, HTSIZE = 24, 32, 262147          # 24 targets in rows of 31 pairs: every sparse row fits, no read is left out
ASCII_OF = np.frombuffer(b"TGCA", np.uint8)


def _genome(rng, k):
    """~300 000 random nucleotides with 30 tandem repeats of units of 1 - 3 nucleotides, 20 - 80 nucleotides long.  Below k = 16
    fewer, so that neither the k-mer space (4^k / 3) nor the super-k-mer layouts' minimizer space (m = k - 4: 4^m / 8) saturates: a
    table whose minimizers are all crowded is answered by the side table and the dense fallback, not by the kernels' front half -
    and a repeat every ~9 000 nucleotides, three at least."""
    G = min(300_000, (1 << (2 * k)) // 3)
    if 12 <= k < 16:
        G = min(G, (1 << (2 * (k - 4))) // 8)
    codes = rng.integers(0, 4, G, dtype=np.uint8)
    n_sites = min(30, max(3, G // 9000))
    sites = []
    for i in range(n_sites):
        n = 20 + (i * 7) % 61
        p = (i + 1) * (G // (n_sites + 2)) + int(rng.integers(0, 50))
        codes[p:p + n] = np.resize(rng.integers(0, 4, 1 + i % 3, dtype=np.uint8), n)
        sites.append((p, n))
    return codes, sites


def _reads(rng, codes, sites, k):
    G = codes.size

    def cut(p, n, strand, *n_at):
        s = bytearray(ASCII_OF[codes[p:p + n]].tobytes())
        for a in n_at:
            s[a] = ord("N")
        return _rc(bytes(s)) if strand else bytes(s)
    at = lambda n: int(rng.integers(0, G - n))
    reads = []
    # every length from k - 1 to k + 135, either strand: no k-mer, one chunk, the edge of the 128-position chunk and the `past`
    # threshold n_act + k - t >= 129 (t >= 7) from both sides
    for n in range(k - 1, k + 136):
        reads += [cut(at(n), n, 0), cut(at(n), n, 1)]
    # one N at every position of a 150-nt read, strands alternating: parts of every length, joined (mic_join2.h) or on the plain road
    for p in range(150):
        reads.append(cut(at(150), 150, p & 1, p))
    # several chunks
    for i in range(30):
        reads.append(cut(at(320), 320, i & 1, *([100 + i] if i % 3 == 0 else [])))
    for i in range(12):
        reads.append(cut(at(1000), 1000, i & 1, *([300 + 17 * i] if i % 3 == 0 else [])))
    # over the planted repeats, with and without an N inside, at their edges and next to them.  (Four reads per site: every run of
    # a crowded minimizer is an item of the follow-up kernel's work area, which holds one per read of the batch and 4 096 more; what
    # does not fit is recounted by the dense path and says so in its flags - exact, but not the kernel's own answer.)
    for j, (p, n) in enumerate(sites):
        for q, shift in enumerate((-40, 40)):
            a = min(max(p + n // 2 - 75 + shift, 0), G - 150)
            reads.append(cut(a, 150, (j + q) & 1))
            reads.append(cut(a, 150, (j + q + 1) & 1, min(max((p + n // 2, p - 1, p + n, p + 3)[(2 * j + q) % 4] - a, 0), 149)))
    data = b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(reads))
    # 150-nt reads of either strand with substitutions and N, a fifth random
    return data + _reads_from(rng, codes, 800, 150)


def _sparse_rows(counts):
    """the oracle's sparse rows in the engine's form: [n, target | count << 16 ...], ascending targets"""
    o = gu.oracle()
    rows = np.zeros((counts.shape[0], ROW_WORDS), np.uint32)
    for r in range(counts.shape[0]):
        n, row = o.sparse_row(counts[r], ROW_WORDS - 1)
        assert n <= ROW_WORDS - 1
        rows[r, 0] = n
        rows[r, 1:1 + n] = row[1:1 + 2 * n:2].astype(np.uint32) | (row[2:2 + 2 * n:2].astype(np.uint32) << 16)
    return rows


def _used(rows):
    """the words of sparse rows that mean something: the count and that many entries"""
    return np.where(np.arange(rows.shape[1])[None, :] <= rows[:, :1], rows, 0)


def _kernel_name(e):
    buf = C.create_string_buffer(256)
    assert e.L.mic_db_kernel_name(e.h, buf, 256) > 0
    return buf.value.decode()


def _engine(k, layout=0):
    from cuclark_amd import MiClarkDB
    return MiClarkDB(k, T, row_words=ROW_WORDS, layout=layout)


@functools.lru_cache(maxsize=None)
def _case(k):
    """the table, the packed reads, what the oracle answers and what the direct layout does: computed once per k, never changed"""
    from cuclark_amd import host
    rng = np.random.default_rng(7000 + k)
    codes, sites = _genome(rng, k)
    _, sizes, keys, lab = _db_of_codes(codes, k, HTSIZE, T, stride=max(codes.size // 33, 1))
    data = _reads(rng, codes, sites, k)
    idx = host.index_reads(data)
    rp, cont = host.pack_reads(data, idx["seq_s"], idx["seq_e"], idx["length"], k)
    odb = gu.oracle().db_from_arrays(sizes, keys, lab)
    counts, bad = odb.query_batch(k, rp, cont, T)
    assert bad == 0
    expect = gu.oracle().result_from_counts(counts)
    n = rp.size - 1
    assert n > 1200 and (expect[:, 0] > 0).sum() >= n // 4        # a table that answers nothing does not pass
    with _engine(k, DIRECT) as e:
        e.read_arrays(sizes, keys, lab)
        assert e.info()["layout"] == DIRECT and _kernel_name(e) == ks.kernel_name(k, 0, DIRECT)
        direct, direct_rows = e.classify_packed(rp, cont, extended=True)
    want_rows = _sparse_rows(counts)
    assert (direct[:, :5] == expect).all() and (_used(direct_rows) == want_rows).all()
    return dict(codes=codes, sites=sites, sizes=sizes, keys=keys, lab=lab, rp=rp, cont=cont, odb=odb, expect=expect, rows=want_rows, direct=direct)


def _mismatch(a, b):
    """for the assertion's message: how many reads differ, the first of them and their rows on both sides"""
    bad = np.flatnonzero((a != b).any(axis=1))
    return bad.size, bad[:10], a[bad[:3], -3:].tolist(), b[bad[:3], -3:].tolist()


def _check(k, m, layouts, monkeypatch):
    c = _case(k)
    rp, cont, expect, direct = c["rp"], c["cont"], c["expect"], c["direct"]
    for layout in layouts:
        with _engine(k, layout) as e:
            e.read_arrays(c["sizes"], c["keys"], c["lab"])
            info = e.info()
            assert (info["layout"], info["minimizer_len"]) == (layout, m if layout != MINIMIZER else ks.decide_layout(k, MINIMIZER)[1])
            assert _kernel_name(e) == ks.kernel_name(k, info["minimizer_len"], layout), (k, m, layout)
            res, rows = e.classify_packed(rp, cont, extended=True)
            assert (res[:, :5] == expect).all(), (k, m, layout, _mismatch(res[:, :5], expect))
            assert (_used(rows) == c["rows"]).all(), (k, m, layout, _mismatch(_used(rows), c["rows"]))
            assert (res == direct).all(), (k, m, layout, _mismatch(res, direct))
            if layout in (SUPER, SUPER2):
                # two blocks: each wavefront runs hundreds of these reads back to back and changes between its roads as often
                monkeypatch.setenv("MIC_QUERY_BLOCKS", "2")
                res2, rows2 = e.classify_packed(rp, cont, extended=True)
                monkeypatch.delenv("MIC_QUERY_BLOCKS")
                assert (res2 == res).all() and (_used(rows2) == _used(rows)).all(), (k, m, layout, _mismatch(res2, res))


@pytest.mark.parametrize("k", ks.DEFAULT_K)
def test_every_k_with_the_default_m(k, monkeypatch):
    monkeypatch.delenv("MIC_MINIMIZER_LEN", raising=False)
    assert ks.SWEEP[k - ks.K_MIN][0] == k
    _check(k, ks.SWEEP[k - ks.K_MIN][1], (MINIMIZER, SUPER, SUPER2), monkeypatch)


@pytest.mark.parametrize("k,m", ks.OTHER_M)
def test_other_minimizer_lengths(k, m, monkeypatch):
    """MIC_MINIMIZER_LEN is read at every table load and the kernels take m from the table: t = 16, t > 16, W = w and the other
    combinations no k reaches with m = 20"""
    monkeypatch.setenv("MIC_MINIMIZER_LEN", str(m))
    _check(k, m, (SUPER, SUPER2), monkeypatch)


@functools.lru_cache(maxsize=None)
def _tied_case(k):
    """Two-part reads whose SECOND part holds a planted repeat, a batch of their own (their crowded runs get a work area of their
    own): the t-mers of a repeat tie, the tie is broken by the position bits, and on the joined road (mic_join2.h) those are the
    position in the part, not in the joined chunk - which only shows where the tied positions hash to different parts of the table.
    Part 1 has k .. k + 31 nucleotides, so the two numberings differ by every residue mod 32; either strand."""
    from cuclark_amd import host
    c = _case(k)
    codes, G = c["codes"], c["codes"].size
    reads = []
    for j, (p, n) in enumerate(c["sites"]):
        for q in range(8):
            at_n = k + (5 * j + 4 * q) % 32                   # the N: part 1 = [0, at_n), part 2 = [at_n + 1, 150)
            a = min(max(p - at_n - 1 - (j + q) % 7, 0), G - 150)
            s = bytearray(ASCII_OF[codes[a:a + 150]].tobytes())
            s[at_n] = ord("N")
            reads.append(bytes(s))
            a = min(max(p + n + (j + q) % 7 - (149 - at_n), 0), G - 150)       # the repeat in front of the N, the read reversed
            s = bytearray(ASCII_OF[codes[a:a + 150]].tobytes())
            s[149 - at_n] = ord("N")
            reads.append(_rc(bytes(s)))
    data = b"".join(b">t%d\n%s\n" % (i, s) for i, s in enumerate(reads))
    idx = host.index_reads(data)
    rp, cont = host.pack_reads(data, idx["seq_s"], idx["seq_e"], idx["length"], k)
    counts, bad = c["odb"].query_batch(k, rp, cont, T)
    assert bad == 0
    expect = gu.oracle().result_from_counts(counts)
    assert (expect[:, 0] > 0).sum() >= (rp.size - 1) // 4
    return dict(rp=rp, cont=cont, expect=expect, rows=_sparse_rows(counts))


@pytest.mark.parametrize("k,layout", [(26, SUPER), (29, SUPER), (29, SUPER2), (24, SUPER2), (27, SUPER), (27, SUPER2), (32, SUPER), (32, SUPER2)])
def test_two_slot_range_parts(k, layout, monkeypatch):
    """k = 26 one-strand: query_kernel_s in its sharded instantiation; k = 29 and k = 24 two-strand: query_kernel_r with k and m from the
    table and the part's compare per run.  Every part answers what the oracle's restatement of the partition says, the parts' hits add
    up to the whole table's, and the rows merged on the device are the whole table's - for the sweep's reads and for the two-part
    reads over the repeats.
    k = 27 and k = 32: the instantiations with constant k and m are the only ones with the pipelined road (query_kernel_r: PIPE = KK
    != 0; with k and m from the table every read takes the plain road), so sampled_positions<CANON, GAP = true> - a joined read's
    position bits from j2_part_offset - runs for these two k and no other, and only a part of the table tells which tied position
    the front half chose.  (k = 31 joins in sampled_positions3: tests/test_two_part_reads_gpu.py has its parts.)"""
    import contextlib
    monkeypatch.delenv("MIC_MINIMIZER_LEN", raising=False)
    c = _case(k)
    with contextlib.ExitStack() as stack:
        engines = []
        for p in range(2):
            e = stack.enter_context(_engine(k, layout))
            e.set_part(p, 2)
            e.read_arrays(c["sizes"], c["keys"], c["lab"])
            info = e.info()
            assert (info["layout"], info["minimizer_len"], info["part"], info["n_parts"]) == (layout, 20, p, 2)
            assert _kernel_name(e) == ks.kernel_name(k, 20, layout, parted=True)
            engines.append((e, info))
        for name, rs in (("sweep", c), ("tied", _tied_case(k))):
            rp, cont, expect = rs["rp"], rs["cont"], rs["expect"]
            n = rp.size - 1
            want = [_oracle_part(c["odb"], info, k, rp, cont, T) for e, info in engines]
            assert all((w[:, 0] > 0).sum() > n // 8 for w in want)           # both parts have their share
            for blocks in (None, "2"):
                if blocks:
                    monkeypatch.setenv("MIC_QUERY_BLOCKS", blocks)
                hits, parts = np.zeros(n, np.int64), []
                for p, (e, info) in enumerate(engines):
                    res, rows = e.classify_packed(rp, cont, extended=True)
                    assert (res[:, :5] == want[p]).all(), (name, p, blocks, _mismatch(res[:, :5], want[p]))
                    hits += res[:, 0]
                    parts.append(rows)
                if blocks:
                    monkeypatch.delenv("MIC_QUERY_BLOCKS")
                assert (hits == expect[:, 0]).all(), (name, blocks)              # every k-mer occurrence is counted by exactly one part
                merged, results = _merge_rows(k, T, ROW_WORDS, parts, n)
                assert (_used(merged) == rs["rows"]).all() and (results[:, :5] == expect).all(), (name, blocks)


@pytest.mark.parametrize("k", [11, 8])
def test_below_k_12_the_super_layout_falls_back_to_the_direct_one(k, monkeypatch):
    monkeypatch.delenv("MIC_MINIMIZER_LEN", raising=False)
    monkeypatch.setenv("MIC_LAYOUT", "super")
    assert ks.decide_layout(k, SUPER) == (DIRECT, 0)
    c = _case(k)
    with _engine(k) as e:
        e.read_arrays(c["sizes"], c["keys"], c["lab"])
        info = e.info()
        assert (info["layout"], info["minimizer_len"]) == (DIRECT, 0) and _kernel_name(e) == ks.kernel_name(k, 0, DIRECT)
        res, rows = e.classify_packed(c["rp"], c["cont"], extended=True)
    assert (res[:, :5] == c["expect"]).all() and (_used(rows) == c["rows"]).all() and (res == c["direct"]).all()
