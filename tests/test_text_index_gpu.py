"""The line index of texts that are resident on the device (csrc/mic_text.hip: mic_text_index_device, mic_text_index_front_device,
mic_pairs_index_device) at the places where it can go wrong in a few KiB: a text that starts at a misaligned address (it counts from
the 4-KiB boundary below: the bytes in front of it are not its own), a text that ends one byte before, at and one byte after a tile
edge, a line end on either side of a tile edge, an unterminated last line, a text shorter than one 16-byte load, mates of different
tile counts.  Every expected value is made here in Python (bytes.split, test_pairs_device._merge), never by the library."""
import ctypes as C

import numpy as np
import pytest

import test_pairs_device as tp

pytestmark = pytest.mark.gpu

TILE = 4096
STARTS = [0, 1, 15, 16, 17, 4095, 4096, 4101]
ENDS = [2 * TILE - 1, 2 * TILE, 2 * TILE + 1]


@pytest.fixture(scope="module")
def eng():
    e, _ = tp._engine()
    with e:
        yield e


@pytest.fixture(scope="module")
def seqs():
    g = tp._genomes()[0]
    return [g[37 * i:37 * i + 10 + i % 11] for i in range(64)]        # 10 .. 20 nt: a FASTQ record of about 40 bytes


def _prefix(a):
    """a bytes that are not the text's: line ends and record markers among them."""
    junk = b"\n@junk>\n>\n@\n\n+\n"
    return (junk * (a // len(junk) + 1))[:a]


def _body(seqs, total, n_records=None, newline_at=None, eol=b"\n", fasta=False, tag=b"", shift=0):
    """Short records, `total` bytes in all: the description of the last record's header is padded to get there.  n_records: that many
    records (else as many as fit); newline_at: the description of one header in the middle is padded so that the line end of that
    header is byte newline_at of the body."""
    def rec(i, pad=0):
        s = seqs[(i + shift) % len(seqs)]
        head = (b">" if fasta else b"@") + b"r%d" % i + tag + b" " + b"x" * pad + eol
        return head + (s[:7] + eol + s[7:] + eol if fasta else s + eol + b"+" + eol + b"I" * len(s) + eol)

    out, n, i = [], 0, 0

    def add(r):
        nonlocal n, i
        out.append(r)
        n += len(r)
        i += 1

    if newline_at is not None:
        while n + 200 < newline_at:
            add(rec(i))
        pad = newline_at + 1 - n - len(rec(i).split(b"\n")[0]) - 1
        assert pad >= 0
        add(rec(i, pad))
        assert b"".join(out)[newline_at:newline_at + 1] == b"\n"
    while (n + 200 < total) if n_records is None else (i + 1 < n_records):
        add(rec(i))
    pad = total - n - len(rec(i))
    assert pad >= 0
    add(rec(i, pad))
    body = b"".join(out)
    assert len(body) == total and (n_records is None or i == n_records)
    return body


def _record_starts(body, fasta=False):
    """Byte offset of every record, then the size of the body."""
    lines = tp._lines(body)
    starts = np.cumsum([0] + [len(l) + 1 for l in lines])
    if fasta:
        return [int(starts[i]) for i, l in enumerate(lines) if l[:1] == b">"] + [len(body)]
    assert len(lines) % 4 == 0
    return [int(starts[i]) for i in range(0, len(lines), 4)] + [len(body)]


def _offsets(e, h):
    sp, ns, stride = C.POINTER(C.c_uint64)(), C.c_size_t(0), C.c_uint32(0)
    assert e.L.mic_text_offsets(h, C.byref(sp), C.byref(ns), C.byref(stride)) == 0
    return np.ctypeslib.as_array(sp, shape=(ns.value,)).copy(), int(stride.value)


def _check_samples(off, stride, first, rec_start):
    n = len(rec_start) - 1
    assert off.size == n // stride + 2 and int(off[0]) == first
    for i in range(off.size):
        assert int(off[i]) - first == rec_start[min(i * stride, n)], i


def _check_whole(e, a, body, fasta=False, at_address=None):
    """prefix(a) + body inflated on the device, the body indexed where it starts."""
    text = _prefix(a) + body
    d, nb, _ = e.gunzip_device(tp._gz(text))
    try:
        assert nb == len(text)
        if at_address is not None:
            at_address.append((d + a) & (TILE - 1))
        h, n_rec, off, stride = e.text_index(d + a, len(body))
        assert h is not None, n_rec
        try:
            rec_start = _record_starts(body, fasta)
            assert n_rec == len(rec_start) - 1 and e.text_format(h) == (">" if fasta else "@")
            _check_samples(off, stride, (d + a) & (TILE - 1), rec_start)
            assert e.text_copy(h, 0, n_rec) == body
        finally:
            e.text_free(h)
    finally:
        e.free_text(d)


def _check_front(e, a, body, n):
    """The same, but the text is the first n bytes of the body: the front of a text that is still growing."""
    text = _prefix(a) + body
    d, nb, _ = e.gunzip_device(tp._gz(text))
    try:
        h, n_rec, used, st = e.text_index_front(d + a, n)
        whole = body[:n].count(b"\n") // 4                      # records whose four lines all end in the front
        rec_start = _record_starts(body)[:whole + 1]
        assert st == 0 and n_rec == whole and used == (rec_start[whole] if whole else 0), (n_rec, used, st)
        if whole == 0:
            assert not h
            return
        assert h
        try:
            off, stride = _offsets(e, h)
            _check_samples(off, stride, (d + a) & (TILE - 1), rec_start)
            assert e.text_copy(h, 0, n_rec) == body[:used]
        finally:
            e.text_free(h)
    finally:
        e.free_text(d)


@pytest.mark.parametrize("end", ENDS)
@pytest.mark.parametrize("a", STARTS)
def test_text_at_a_misaligned_start_ending_around_a_tile_edge(eng, seqs, a, end):
    body = _body(seqs, end - a)
    assert len(_record_starts(body)) - 1 > 64                   # (an interior stride sample exists)
    _check_whole(eng, a, body)


@pytest.mark.parametrize("variant", ["unterminated", "crlf", "fasta", "fasta_crlf"])
def test_variants_of_one_shape(eng, seqs, variant):
    a, eol, fasta = 17, b"\r\n" if variant.endswith("crlf") else b"\n", variant.startswith("fasta")
    body = _body(seqs, 2 * TILE - a, eol=eol, fasta=fasta)
    if variant == "unterminated":
        body = body[:-1]
        assert body[-1:] == b"I"
    _check_whole(eng, a, body, fasta)


@pytest.mark.parametrize("a", [0, 15, 17, 4095])
def test_text_shorter_than_one_load(eng, a):
    _check_whole(eng, a, b"@r\nA\n+\nI\n")


@pytest.mark.parametrize("at", [TILE - 1, TILE])
def test_line_end_on_either_side_of_a_tile_edge(eng, seqs, at):
    """A '\\n' that is the last byte of the text's first tile / the first byte of its second one, counted from the 4-KiB boundary below
    the text's first byte (where the device put the text is only known once it is there: the body is made for that address)."""
    a = 17
    d, _, _ = eng.gunzip_device(tp._gz(_prefix(a) + _body(seqs, 2 * TILE)))
    eng.free_text(d)
    first = (d + a) & (TILE - 1)
    body = _body(seqs, 2 * TILE, newline_at=at - first)
    aimed = []
    _check_whole(eng, a, body, at_address=aimed)
    assert aimed == [first], "the device put two texts of one size at addresses that differ modulo 4 KiB: the line end missed the tile edge"


@pytest.mark.parametrize("end", ENDS)
@pytest.mark.parametrize("a", STARTS)
def test_front_cut_inside_the_last_record(eng, seqs, a, end):
    body = _body(seqs, end - a)
    _check_front(eng, a, body, len(body) - 5)                   # (the last record's quality line is not whole)


@pytest.mark.parametrize("a", [0, 17, 4095])
def test_front_cut_inside_the_first_record(eng, seqs, a):
    body = _body(seqs, 2 * TILE - a)
    _check_front(eng, a, body, _record_starts(body)[1] - 3)


def _check_pair(e, fq1, fq2):
    tx = tp._Texts(e, fq1, fq2)
    try:
        h, n_rec, off, stride = tx.index()
        assert h is not None, n_rec
        try:
            recs = tp._merge(fq1, fq2)
            want = [int(x) for x in np.cumsum([0] + [len(r) for r in recs])]
            assert n_rec == len(recs)
            _check_samples(off, stride, 0, want)
            assert e.pairs_text(h, 0, n_rec) == b"".join(recs)
        finally:
            e.pairs_free(h)
    finally:
        tx.free()


def test_pair_of_texts_that_end_at_a_tile_edge(eng, seqs):
    _check_pair(eng, _body(seqs, 2 * TILE, n_records=130, tag=b"/1"), _body(seqs, 3 * TILE, n_records=130, tag=b"/2", shift=5))


def test_pair_of_texts_with_different_tile_counts(eng, seqs):
    fq1, fq2 = _body(seqs, 4000, n_records=70, tag=b"/1"), _body(seqs, 9000, n_records=70, tag=b"/2", shift=5)
    assert (len(fq1) + TILE - 1) // TILE == 1 and (len(fq2) + TILE - 1) // TILE == 3
    _check_pair(eng, fq1, fq2)


def test_pair_with_one_unterminated_mate(eng, seqs):
    fq1, fq2 = _body(seqs, 5000, n_records=70, tag=b"/1"), _body(seqs, 6000, n_records=70, tag=b"/2", shift=5)
    _check_pair(eng, fq1[:-1], fq2)
