"""The entry walk and the end of a read in the per-run query kernel (cuclark_amd/csrc/mic_kernels.hip: consume, tally_counts, finish)
through the C ABI.  Tables of the `tiny`, `tiny_repeats` and `tiny_homolog` synthetic workloads for k = 31 on the one-strand and the
two-strand super-k-mer layout, whole and as two slot-range parts each, `tiny` for k = 27 and k = 32 (the other instantiations with
constant k and m) and for k = 28 (the instantiations that take k and m from the table: 2k - m = 36 keeps both layouts on the per-run kernel, which
the test asserts by the kernel's name), against the direct layout, which knows
neither slots of entries nor runs: all 8 result words and the sparse rows equal on every read.  Reads of the generator, 100 .. 150
nucleotides (genome reads of either strand with substitutions, a fifth random), in the packer's format and in the terminated one,
on the full grid and on two blocks (MIC_QUERY_BLOCKS), where one wavefront meets every case in sequence.  Integer work: every
comparison is exact.

The read sets must hold the classes the walk distinguishes; a class that comes out empty fails the test.  Counted on the CPU from the
direct layout's rows: reads with no hit, with one label, with two labels (a read of at most 150 nucleotides is one round of runs:
both labels are tallied in that round) and with more than 15 labels (the mosaic segments of `tiny_homolog`).  Counted by the engine
(mic_last_crowd_stats): runs that meet the marker of a crowded minimizer (`tiny_repeats`).  Counted on the CPU from the SLOTS of the
one-strand table, read back from the device (mic_debug_fetch_slots), with the walk restated in Python over the runs of a few
hundred of the reads (`_walk_classes`; sampling: test_strand_bits_gpu._sampled): runs whose minimizer has a later entry in the same
slot that carries hits ("second entry"), runs that find hits in a continuation slot after they left the slot before it at entry 5
("across a slot's end"), and runs that keep k-mers behind an entry of theirs whose neighbour in the slot has another key - the pass
that is no longer made ("foreign next entry").  The restated walk's hits per read must be the direct layout's: the model is
checked by the same rows it classifies.
Counts above 65 535 are out of reach at this size (a read of 150 nucleotides has 120 k-mers)."""
import contextlib

import numpy as np
import pytest

from test_strand_bits_gpu import DIRECT, SUPER, SUPER2, _codes, _pack, _rc_value, _sampled, _synth_db, _synth_spec, _value
from test_two_part_reads_gpu import _genome_reads, _merge_rows, _pack_terminated

pytestmark = pytest.mark.gpu

HOMOLOG = dict(htsize=9999991, genome_nt=8_000_000, n_genomes=1000, n_targets=1000, mosaic_ppm=150_000)
# name -> k, generator settings, slot-range parts too, classes the table's reads must hold (every class is held by one table at least)
TABLES = {
    "k31 tiny": (31, dict(), True, ("no hit", "one label", "foreign next entry")),       # (64 random genomes: no read of it meets two targets)
    "k31 tiny_repeats": (31, dict(genome_nt=3_000_000, repeat_ppm=50_000), True, ("no hit", "one label", "crowded")),
    "k31 tiny_homolog": (31, HOMOLOG, True, ("no hit", "one label", "two labels", "more than 15 labels", "second entry", "across a slot's end",
                                        "foreign next entry")),
    "k27 tiny": (27, dict(), False, ("no hit", "one label")),
    "k32 tiny": (32, dict(), False, ("no hit", "one label")),
    "k28 tiny": (28, dict(), False, ("no hit", "one label")),        # k and m from the table
}
N_READS = 3000


def _reads(spec):
    g = _genome_reads(spec, N_READS, 311)
    return [s[:100 + (i * 7) % 51] for i, s in enumerate(g)]


def _classes(want):
    """reads per class, from the direct layout's result words (word 0: hits, word 5: labels in the row)"""
    n_lab = want[:, 5]
    return {"no hit": int((want[:, 0] == 0).sum()), "one label": int((n_lab == 1).sum()), "two labels": int((n_lab == 2).sum()),
            "more than 15 labels": int((n_lab > 15).sum())}


def _kernel_name(e):
    import ctypes as C
    buf = C.create_string_buffer(256)
    assert e.L.mic_db_kernel_name(e.h, buf, 256) > 0
    return buf.value.decode()


K31, M20, CTX, MODELLED = 31, 20, 11, 400


def _walk_classes(engine, reads, want):
    """The entry walk of query_kernel_r restated over the slots of the one-strand k = 31 table (include/mi_clark.h:
    mic_debug_fetch_slots), for the MODELLED reads with the most labels and as many of the others: runs per class, see the module's
    docstring.  A read's hits summed over its runs must be the direct layout's."""
    S = engine.fetch_slots()
    n_main = int(engine.info()["n_slots"]) - int(engine.info()["n_overflow"])
    cnt = (S[:, 30] & 0xFF).astype(np.int64)
    R01 = (S[:, 6:24:3].astype(np.uint64) << np.uint64(32)) | S[:, 7:24:3].astype(np.uint64)
    X = (R01 >> np.uint64(2)) & np.uint64((1 << 40) - 1)                     # the entries' minimizers: nucleotides 11 .. 30 of the region
    live = np.arange(6)[None, :] < cnt[:, None]
    owner = np.arange(S.shape[0])                                            # a continuation slot's main slot
    for s in np.flatnonzero((S[:n_main, 30] & 0x100) != 0):
        c = int(s)
        while int(S[c, 30]) & 0x100:
            c = int(S[c, 31])
            owner[c] = s
    xs, slot_of = X[live], np.broadcast_to(np.arange(S.shape[0])[:, None], X.shape)[live]
    order = np.argsort(xs, kind="stable")
    xs, slot_of = xs[order], slot_of[order]
    order = np.argsort(-want[:, 5].astype(np.int64), kind="stable")
    picked = list(order[:MODELLED // 2]) + list(order[MODELLED // 2:][:: max(1, (len(order) - MODELLED // 2) // (MODELLED // 2))][:MODELLED // 2])
    held = {"second entry": 0, "across a slot's end": 0, "foreign next entry": 0}
    for r in picked:
        seq = reads[r]
        c, sp = _codes(seq), _sampled(seq)
        total, crowded, i = 0, False, 0
        while i < len(sp):
            i_last = i
            while i_last + 1 < len(sp) and sp[i_last + 1] == sp[i]:
                i_last += 1
            p, n = sp[i], i_last - i + 1
            jmaxf, jminf = p - i, p - i_last
            i = i_last + 1
            xf = _value(c[p:p + M20])
            xr = _rc_value(xf, M20)
            rev = xr < xf
            x = xr if rev else xf
            win = [c[q] if 0 <= q < len(c) else 0 for q in range(p - CTX, p + M20 + CTX)]
            if rev:
                win = [3 - v for v in reversed(win)]
            jmax, jmin = (CTX - jminf, CTX - jmaxf) if rev else (jmaxf, jminf)
            at = int(np.searchsorted(xs, np.uint64(x)))
            if at >= len(xs) or int(xs[at]) != x:
                continue                                                     # nothing stored under this minimizer
            slot, key, remaining, from_five = int(owner[slot_of[at]]), x & 0xFFFFFFFF, n, False
            while True:
                keys = [int(v) for v in S[slot, :6]]
                e = sum(v < key for v in keys)
                more, first = e < 6, True
                e = min(e, 5)
                last_same_at_five = False
                while True:
                    same = more and keys[e] == key
                    hits = 0
                    if same and int(X[slot, e]) == x and e < cnt[slot]:
                        reg = (int(S[slot, 6 + 3 * e]) << 64) | (int(S[slot, 7 + 3 * e]) << 32) | int(S[slot, 8 + 3 * e])
                        ent = [(reg >> (94 - 2 * q)) & 3 for q in range(2 * CTX + M20)]
                        left = 0
                        while left < CTX and ent[CTX - 1 - left] == win[CTX - 1 - left]:
                            left += 1
                        right = 0
                        while right < CTX and ent[CTX + M20 + right] == win[CTX + M20 + right]:
                            right += 1
                        mask = int(S[slot, 24 + e]) >> 16
                        if mask == 0:
                            crowded = True
                            remaining = -16
                        hi, lo = min(left, jmax), max(CTX - right, jmin)
                        hits = sum((mask >> j) & 1 for j in range(lo, hi + 1))
                    if hits and not first:
                        held["second entry"] += 1
                    if hits and first and from_five:
                        held["across a slot's end"] += 1
                    total += hits
                    remaining -= hits
                    go = same and remaining > 0 and e < 5
                    if go and keys[e + 1] != key:
                        held["foreign next entry"] += 1
                    more = go and keys[e + 1] == key
                    last_same_at_five = same and e == 5
                    if not more:
                        break
                    e, first = e + 1, False
                if remaining > 0 and (int(S[slot, 30]) & 0x100) and keys[5] <= key:
                    slot, from_five = int(S[slot, 31]), last_same_at_five
                else:
                    break
        assert crowded or total == int(want[r, 0]), (r, total, int(want[r, 0]))
    return held


def _rows_equal(rows, want_rows):
    """sparse rows: word 0 the number of entries (or the mark of a row that did not fit), then the entries; the words behind them are
    whatever the buffer held"""
    a, b = rows.view(np.uint32), want_rows.view(np.uint32)
    n_ent = np.where(b[:, 0] == 0xFFFFFFFF, 0, b[:, 0]).astype(np.int64)
    live = np.arange(b.shape[1])[None, :] <= n_ent[:, None]
    return a.shape == b.shape and bool((a[live] == b[live]).all())


def _crowded_runs(engine, rp, cont, n):
    """runs handed to the follow-up kernel because they met the marker of a crowded minimizer (the engine's own bookkeeping)"""
    import torch
    dev = torch.device("cuda:0")
    d_rp = torch.from_numpy(rp.view(np.int32)).to(dev)
    d_ct = torch.from_numpy(np.concatenate([cont, np.zeros(64, np.uint16)]).view(np.int16)).to(dev)
    d_res = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.query_device(d_rp.data_ptr(), d_ct.data_ptr(), n, d_res.data_ptr())
    st = engine.last_crowd_stats()
    engine.resolve_flagged_device(d_rp.data_ptr(), d_ct.data_ptr(), d_res.data_ptr())
    return int(st["runs"])


@pytest.mark.parametrize("name", sorted(TABLES))
def test_rows_equal_the_direct_layouts(name, monkeypatch):
    from cuclark_amd import MiClarkDB
    k, kw, parts, must_hold = TABLES[name]
    spec = _synth_spec(k, **kw)
    T = int(spec.n_targets)
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
        reads = _reads(spec)
        assert all(100 <= len(s) <= 150 for s in reads)
        packers, terminated = _pack(reads, k), _pack_terminated(reads, k)
        want, want_rows = engines["direct"].classify_packed(*packers, extended=True)
        n = want.shape[0]
        assert n == N_READS

        # the classes this table's reads must hold
        held = _classes(want)
        if "crowded" in must_hold:
            held["crowded"] = _crowded_runs(engines["super"], packers[0], packers[1], n)
        if "foreign next entry" in must_hold:
            held.update(_walk_classes(engines["super"], reads, want))
        if k == 28:
            for layout in ("super", "super2"):
                assert _kernel_name(engines[layout]).startswith("query_kernel_r<0, 0,"), _kernel_name(engines[layout])
        print(name, held)
        for c in must_hold:
            assert held[c] > 0, (name, c, held)

        for blocks in (None, "2"):
            if blocks:
                monkeypatch.setenv("MIC_QUERY_BLOCKS", blocks)
            for fmt, (rp, cont) in (("packer's", packers), ("terminated", terminated)):
                for layout in ("super", "super2"):
                    res, rows = engines[layout].classify_packed(rp, cont, extended=True)
                    assert (res == want).all(), (layout, fmt, blocks, np.flatnonzero((res != want).any(axis=1))[:10])
                    assert _rows_equal(rows, want_rows), (layout, fmt, blocks)
                    if layout + " parts" not in engines:
                        continue
                    hits, part_rows = np.zeros(n, np.int64), []
                    for e in engines[layout + " parts"]:
                        r, w = e.classify_packed(rp, cont, extended=True)
                        hits += r[:, 0]
                        part_rows.append(w)
                    assert (hits == want[:, 0]).all(), (layout, fmt, blocks)     # every k-mer occurrence is counted by exactly one part
                    merged, results = _merge_rows(k, T, part_rows[0].shape[1], part_rows, n)
                    fits = merged[:, 0] != 0xFFFFFFFF
                    assert (results[fits, :5] == want[fits, :5]).all(), (layout, fmt, blocks)
            if blocks:
                monkeypatch.delenv("MIC_QUERY_BLOCKS")
