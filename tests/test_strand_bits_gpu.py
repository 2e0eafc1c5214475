"""The strand handling of the one-strand super-k-mer table (canonical t-mers in the front half, the reverse-complemented region of a
run in the per-run kernel's set-up) through the C ABI: a read and its reverse complement give the same rows, hand-built reads at
the edges of that code give the oracle's rows on every layout, and the tables of the toy workloads keep their shape.  Integer
work: every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

DIRECT, SUPER, SUPER2 = 1, 3, 4
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(seq):
    return seq[::-1].translate(_COMP)          # N stays N


def _synth_spec(k, **kw):
    from cuclark_amd import _lib
    w = dict(seed=4, htsize=999983, genome_nt=1_500_000, n_targets=50, n_genomes=64, k=k, key_bytes=8)      # bench.py: `tiny`
    w.update(kw)
    return _lib.MicSynthSpec(**w)


def _synth_db(spec):
    import torch
    from cuclark_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    cap = int(spec.genome_nt) + 1024
    d_sizes = torch.zeros(spec.htsize, dtype=torch.uint8, device=dev)
    d_keys = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_labels = torch.zeros(cap, dtype=torch.int16, device=dev)
    n_el = C.c_uint64(0)
    torch.cuda.synchronize()
    assert L.mic_synth_db_device(C.byref(spec), d_sizes.data_ptr(), d_keys.data_ptr(), d_labels.data_ptr(), cap, C.byref(n_el), None) == 0
    torch.cuda.synchronize()
    return d_sizes, d_keys, d_labels, n_el.value


def _pack(reads, k):
    from cuclark_amd import host
    data = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads))
    idx = host.index_reads(data)
    return host.pack_reads(data, idx["seq_s"], idx["seq_e"], idx["length"], k)


# ------------------------------------------------------------------ a read and its reverse complement

@pytest.mark.parametrize("k", [31, 27, 32, 25])
def test_a_read_and_its_reverse_complement_give_the_same_rows(k):
    """2 000 reads of the generator (genome reads of either strand with substitutions and N, random reads) against a 50-target table
    of the `tiny` workload's shape on the one-strand layout, and the reverse complements of the same reads: equal rows pairwise, and
    both the oracle's.  k = 31 / 27 / 32 with m = 20 are the instantiations with constant k and m (t = 8 / 12 / 7), k = 25 the generic
    one."""
    import torch
    from cuclark_amd import _lib, MiClarkDB
    L = _lib.load()
    dev = torch.device("cuda:0")
    spec = _synth_spec(k)
    T = 50
    d_sizes, d_keys, d_labels, n_el = _synth_db(spec)
    n_reads, read_len = 2000, 150
    rec = L.mic_synth_text_record_bytes(read_len, 1)
    assert rec == read_len + 13
    d_text = torch.zeros(n_reads * rec, dtype=torch.uint8, device=dev)
    assert L.mic_synth_reads_text_device(C.byref(spec), 99, n_reads, read_len, 0.2, 0.01, 0.002, 1, -1, d_text.data_ptr(), d_text.numel(), None) == 0
    torch.cuda.synchronize()
    text = d_text.cpu().numpy().reshape(n_reads, rec)
    fwd = [bytes(text[r, 12:12 + read_len]) for r in range(n_reads)]
    assert all(set(s) <= set(b"ACGTN") for s in fwd) and sum(b"N" in s for s in fwd) > 100
    rev = [_rc(s) for s in fwd]
    odb = gu.oracle().db_from_arrays(d_sizes.cpu().numpy(), d_keys[:n_el].cpu().numpy().view(np.uint64),
                                     d_labels[:n_el].cpu().numpy().view(np.uint16))
    rows = []
    with MiClarkDB(k, T, layout=SUPER) as e:
        e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        assert e.info()["layout"] == SUPER and e.info()["minimizer_len"] == 20
        for reads in (fwd, rev):
            rp, cont = _pack(reads, k)
            counts, bad = odb.query_batch(k, rp, cont, T)
            assert bad == 0
            expect = gu.oracle().result_from_counts(counts)
            res = e.classify_packed(rp, cont)
            assert (res[:, :5] == expect).all()
            rows.append(res)
    assert (rows[0] == rows[1]).all()
    assert (rows[0][:, 0] > 0).sum() > 1200          # the genome reads hit


# ------------------------------------------------------------------ hand-built reads

K, M = 31, 20
W_, T_, WIN = K - M + 1, 8, K - 8 + 1            # w = 12 m-mers per k-mer, t-mers of 8 nucleotides, 24 of them per k-mer


def _codes(seq):
    return [b"TGCA".index(c) for c in seq]


def _value(codes):
    v = 0
    for c in codes:
        v = v << 2 | c
    return v


def _rc_value(v, n):
    r = 0
    for _ in range(n):
        r = r << 2 | (3 - (v & 3))
        v >>= 2
    return r


def _order(tv):
    tv = min(tv, _rc_value(tv, T_))
    return ((tv * 0x9E3779 + 0x27D4EB2F) & 0xFFFFFFFF) >> 5


def _sampled(seq):
    """What the query does with a part without N (mic_device.h: mod-sampling; mic_kernels.hip: sampled_positions), restated: for
    every k-mer the part position of its sampled m-mer.  Order of a t-mer: the top 27 bits of a 24-bit multiply-add of its canonical
    value; ties go to the smaller position mod 32."""
    c = _codes(seq)
    keys = []
    for p in range(len(c) - T_ + 1):
        keys.append(_order(_value(c[p:p + T_])) << 5 | (p & 31))
    out = []
    for j in range(len(c) - K + 1):
        i = min(range(WIN), key=lambda i_: keys[j + i_])
        out.append(j + i % W_)
    return out


def _mmer(seq, p):
    return _value(_codes(seq[p:p + M]))


# 158 nucleotides = one chunk of 128 k-mers whose sampled m-mer changes more than 32 times (found by a seeded search over
# substitutions with _sampled; a random read has ~15 runs)
MANY_RUNS = (b"CGCATGCTTGCCGCAAAGATGGCCAAGTGTCCCCCCGTTCACGTCGACATAAATGACCGGACCCAGCTATTATGATTCCG"
             b"GCATAACGAGGTGATCCTTATCTTCAGTGTTTCTTAAGTTTACTATTTTTCCGTTGCCTAGCAGAGCGCGATTTTTCG")


def _edge_reads():
    """name -> read; the genome the database is cut from is their concatenation (separated by N)"""
    rng = np.random.default_rng(2024)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    reads = {}
    def low(n):
        """n random nucleotides whose first t-mer has an order among the lowest 1 %: it wins its windows, the m-mer it starts (or, as its
        reverse complement, ends) is the sampled one"""
        while True:
            x = rnd(n)
            if _order(_value(_codes(x[:T_]))) < (1 << 27) // 100:
                return x
    # a sampled m-mer that is its own reverse complement, at every offset inside its k-mers, in random flanks
    own = 0
    for i in range(2 * W_):
        h = low(M // 2)
        fl = rnd(100)
        s = fl[:40 + i % W_] + h + _rc(h) + fl[60 + i % W_:]
        reads[f"palindrome {i}"] = s
        own += any(_mmer(s, p) == _rc_value(_mmer(s, p), M) for p in _sampled(s))
    assert own >= 20
    # m-mers whose first 8 nucleotides are the reverse complement of their last 8 and which differ after: both strands agree on the
    # high bits of the minimizer value, the comparison is decided in the middle
    half = 0
    for i in range(2 * W_):
        x, mid = low(8), rnd(4)
        while mid == _rc(mid):
            mid = rnd(4)
        mm = x + mid + _rc(x)
        fl = rnd(100)
        s = fl[:40 + i % W_] + mm + fl[60 + i % W_:]
        reads[f"half palindrome {i}"] = s
        half += any(s[p:p + M] == mm for p in _sampled(s))
    assert half >= 20
    # regions that reach before the first and past the last nucleotide of the read: sampled m-mers at positions 0 .. 11 and at the
    # last w positions, over reads of 100 .. 150 nucleotides
    first, last = set(), set()
    for i in range(60):
        s = rnd(100 + (i * 7) % 51)
        reads[f"ends {i}"] = s
        sp = _sampled(s)
        first |= {p for p in sp if p < W_}
        last |= {len(s) - M - p for p in sp if len(s) - M - p < W_}
    assert first == set(range(W_)) and last == set(range(W_))
    # one k-mer, two k-mers, a full chunk of 128 k-mers, a chunk and one k-mer
    for n in (K, K + 1, 128 + K - 1, 128 + K):
        reads[f"length {n}"] = rnd(n)
    # N inside the first and inside the last window of 16 nucleotides, and both
    for i, cut in enumerate(((5,), (144,), (5, 144), (0,), (149,), (15, 16), (30, 119))):
        s = bytearray(rnd(150))
        for p in cut:
            s[p] = ord("N")
        reads[f"N {i}"] = bytes(s)
    # more than 32 runs in one chunk: more than one round of staged slots
    sp = _sampled(MANY_RUNS)
    assert len(MANY_RUNS) == 128 + K - 1 and 1 + sum(a != b for a, b in zip(sp, sp[1:])) > 32
    reads["many runs"] = MANY_RUNS
    reads["many runs + tail"] = MANY_RUNS + rnd(40)
    return reads


def _edge_case():
    reads = _edge_reads()
    o = gu.oracle()
    rng = np.random.default_rng(7)
    htsize, T = 100003, 9
    kmers = set()
    for name, s in reads.items():
        for part in s.split(b"N"):
            c = _codes(part)
            for j in range(len(c) - K + 1):
                v = o.canonical(_value(c[j:j + K]), K)
                if name.startswith("length") or (v * 0x9E3779B97F4A7C15 >> 40) % 5:      # gaps in the presence masks
                    kmers.add(v)
    kmers |= {o.canonical(int(v), K) for v in rng.integers(0, 1 << 62, 3000, dtype=np.uint64)}
    canon = sorted(kmers, key=lambda c: (c % htsize, c // htsize))
    sizes = np.zeros(htsize, np.int64)
    for c in canon:
        sizes[c % htsize] += 1
    assert sizes.max() < 255
    sizes = sizes.astype(np.uint8)
    keys = np.array([c // htsize for c in canon], dtype=np.uint64)
    labels = np.array([(c >> 9) % T for c in canon], dtype=np.uint16)
    both = [s for r in reads.values() for s in (r, _rc(r))]
    rp, cont = _pack(both, K)
    counts, bad = o.db_from_arrays(sizes, keys, labels).query_batch(K, rp, cont, T)
    assert bad == 0
    expect = o.result_from_counts(counts)
    assert (expect[:, 0] > 0).all()
    return sizes, keys, labels, T, rp, cont, expect


@pytest.fixture(scope="module")
def edge_case():
    """reads (each one and its reverse complement), a database of four fifths of their k-mers plus unrelated ones, the oracle's rows"""
    return _edge_case()


@pytest.mark.parametrize("layout", [SUPER, SUPER2, DIRECT])
def test_reads_at_the_edges_of_the_strand_handling(layout, edge_case):
    from cuclark_amd import MiClarkDB
    sizes, keys, labels, T, rp, cont, expect = edge_case
    with MiClarkDB(K, T, layout=layout) as e:
        e.read_arrays(sizes, keys, labels)
        assert e.info()["layout"] == layout
        res = e.classify_packed(rp, cont)
    assert (res[:, :5] == expect).all()
    assert (res[0::2] == res[1::2]).all()              # a read and its reverse complement


# ------------------------------------------------------------------ the tables keep their shape

# info() of the one-strand tables of bench.py's toy workloads, recorded from runs of the commit before the change of the
# reverse-complement bit work: the canonical t-mer decides under which positions the build stores a k-mer, so a different value
# anywhere would show as other entries, chains or continuation slots.  (k-mers, main slots, entries, continuation slots, largest
# chain, k-mers in the side table.)
# The continuation slots of a table with crowded minimizers are no single number in the parent either: the one-pass build takes them
# from a pool while it writes the chains, the crowded groups among them, whose entries depend on the order in which the scatter's
# atomics staged the candidates; the groups then leave for the side table and the entries that stay are the same in every build.
# 96 builds of `tiny_repeats` with the parent's build code (48 with the parent's library, 48 with this one, identical spread) gave
# 287 (9 times), 288 (55), 289 (29), 290 (3): mean 288.3, standard deviation 0.67 - every other field was the same in all of them,
# and all fields in 12 builds each of the two tables without crowded minimizers.  The test takes six deviations either way, 284 ..
# 293: a build passes or fails on what it computes, not on the draw.
PARENT_TABLES = {
    "tiny": (dict(), (1498048, 119603, 178645, 107, 9, 0)),
    "tiny_repeats": (dict(genome_nt=3_000_000, repeat_ppm=50_000), (2869187, 220450, 342503, range(284, 294), 9, 63)),
    "tiny_homolog": (dict(htsize=9999991, genome_nt=8_000_000, n_genomes=1000, n_targets=1000, mosaic_ppm=150_000), (7970000, 651338, 1265093, 32272, 29, 0)),
}
TABLE_FIELDS = ("n_elems", "n_main", "n_entries", "n_overflow", "max_chain", "side_kmers")


def _table_fields(info):
    """info()'s n_slots counts the continuation slots too"""
    d = {f: int(info[f]) for f in ("n_elems", "n_entries", "n_overflow", "max_chain", "side_kmers")}
    d["n_main"] = int(info["n_slots"]) - d["n_overflow"]
    return tuple(d[f] for f in TABLE_FIELDS)


@pytest.mark.parametrize("workload", sorted(PARENT_TABLES))
def test_tables_of_the_toy_workloads_are_the_parents(workload):
    from cuclark_amd import MiClarkDB
    kw, want = PARENT_TABLES[workload]
    spec = _synth_spec(31, **kw)
    d_sizes, d_keys, d_labels, n_el = _synth_db(spec)
    with MiClarkDB(31, spec.n_targets, layout=SUPER) as e:
        e.read_device(d_sizes.data_ptr(), spec.htsize, d_keys.data_ptr(), 8, d_labels.data_ptr())
        got = _table_fields(e.info())
    print(workload, dict(zip(TABLE_FIELDS, got)))
    for f, g, w in zip(TABLE_FIELDS, got, want):
        assert (g in w) if isinstance(w, range) else (g == w), (f, g, w)
