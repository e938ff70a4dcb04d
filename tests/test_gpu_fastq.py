"""`api.read_fastq` on the GPU against the contract's restatement (fastq_ref.py): store bytes, offsets, pieces_cut,
statistics and names over a seeded fuzz of small files and the hand cases, files laid out across the kernels' tile edges, repeated
calls, `.gz` copies, and malformed files, which raise ValueError and leave the process able to read the next file."""
import dataclasses
import gzip

import numpy as np
import pytest

import fastq_ref as F
from test_fastq_ref import HAND, MALFORMED

pytestmark = pytest.mark.gpu
K = 7
THRESHOLDS = (0, 2, 20, 40, 93)
LENGTHS = (0, 1, K - 1, K, K + 1, 151)
ALPHABET = np.frombuffer(b"ACGTacgtNnRY", np.uint8)
ALPHABET_P = [.2, .2, .2, .2, .03, .03, .03, .03, .03, .02, .02, .01]
# Phred values on both sides of every threshold, plus 10 and 31, whose characters are `+` and `@`
PHRED = np.array([0, 1, 2, 3, 10, 19, 20, 21, 31, 39, 40, 41, 92, 93], np.uint8)


def _read(rng, name: bytes, length: int):
    """One read: a third of them are good at every threshold (quality 93 throughout), a third masked by every threshold above 0
    (quality 0 or 1) -- or, all `N`, by 0 as well --, the rest mixed."""
    bases = rng.choice(ALPHABET, length, p=ALPHABET_P)
    kind = int(rng.integers(0, 6))
    if kind < 2:
        quals = np.full(length, 93, np.uint8)
        if kind == 0:
            bases = rng.choice(ALPHABET[:8], length)
    elif kind < 4:
        quals = rng.integers(0, 2, length).astype(np.uint8)
        if kind == 2:
            bases = np.full(length, ord("N"), np.uint8)
    else:
        quals = rng.choice(PHRED, length)
    return name, bases.astype(np.uint8).tobytes(), (quals + 33).astype(np.uint8).tobytes()


def _fuzz_text(rng) -> bytes:
    reads = []
    for i in range(int(rng.integers(1, 13))):
        name = f"r{i}".encode() + (b"" if rng.random() < 0.5 else b" desc\tmore") if rng.random() < 0.9 else b""
        reads.append(_read(rng, name, int(rng.choice(LENGTHS))))
    eol = b"\r\n" if rng.random() < 0.3 else b"\n"
    text = b"".join(b"@" + n + eol + s + eol + (b"+" + n if rng.random() < 0.3 else b"+") + eol + q + eol for n, s, q in reads)
    tail = int(rng.integers(0, 4))
    if tail == 1:
        text = text[:-len(eol)]  # no final newline
    elif tail == 2:
        text += eol * int(rng.integers(1, 4))  # blank lines behind the last record
    return text


def _check(api, path, text: bytes, q: int):
    """Both modes of one file against the restatement; returns the split store's arrays (copies)."""
    store, st = api.read_fastq(str(path), q)
    data, off, want = F.split(text, q)
    d, o = store.arrays()
    assert d.tobytes() == data and o.tolist() == off
    got = dataclasses.asdict(st)
    assert got.pop("tile_bytes") > 0 and got == want and store.pieces_cut == want["pieces_cut"]
    seqs, names, nst = api.read_fastq(str(path), q, named=True)
    want_seqs, want_names, want = F.named(text, q)
    nd, no = seqs.arrays()
    assert nd.tobytes() == b"".join(want_seqs) and no.tolist() == np.cumsum([0] + [len(s) for s in want_seqs]).tolist()
    assert names == want_names
    got = dataclasses.asdict(nst)
    got.pop("tile_bytes")
    assert got == want
    return d.copy(), o.copy()


@pytest.mark.parametrize("q", THRESHOLDS)
def test_fuzz_against_the_restatement(product_lib, tmp_path, q):
    """60 files per threshold (300 in all), read lengths from {0, 1, k-1, k, k+1, 151}."""
    from matchtigs_amd import api

    rng = np.random.default_rng(1000 + q)
    entirely = untouched = 0
    for i in range(60):
        text = _fuzz_text(rng)
        for _, bases, quals in F.records_of(text):
            flags = F.good_flags(bases, quals, q)
            acgt = [b in F.ACGT for b in bases]
            entirely += bool(bases) and any(acgt) and not any(flags)   # masked entirely by the quality threshold
            untouched += bool(bases) and flags == acgt and any(acgt)   # ... and not at all
        p = tmp_path / f"f{i}.fq"
        p.write_bytes(text)
        _check(api, p, text, q)
    assert untouched > 0 and (entirely > 0 or q == 0)  # (Q = 0 masks nothing by quality: there the all-`N` reads are the empty ones)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(product_lib, tmp_path, name):
    from matchtigs_amd import api

    text, q, pieces, cut, (records, bases, other, masked), names = HAND[name]
    p = tmp_path / "hand.fq"
    p.write_bytes(text)
    d, o = _check(api, p, text, q)
    assert [d[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(o) - 1)] == pieces
    for other_q in THRESHOLDS:
        _check(api, p, text, other_q)


def _multi_tile_text(tile: int):
    """A text of a little more than four tiles. With T = tile:
      - a record boundary on the first edge: the `\\n` that ends a quality line is byte T - 1, the `@` of the next header byte T;
      - a sequence line across the second edge: its bases 0 .. 150 are bytes 2T - 40 .. 2T + 110, all good -- one piece across it;
      - a not-good run across the third edge: bases 30 .. 50 of a read are bytes 3T - 10 .. 3T + 10; 38 .. 42 are `N`, the others of
        the run have quality 5 (not good from Q = 6 on), and the qualities of this read lie in the next tile;
      - a quality line across the fourth edge: its byte 40 is byte 4T, with qualities 5 at 35 .. 45."""
    rng = np.random.default_rng(tile)
    out = bytearray()

    def add(name: bytes, bases: bytes, quals: bytes):
        out.extend(b"@" + name + b"\n" + bases + b"\n+\n" + quals + b"\n")

    def ordinary(name: bytes, length: int = 151):
        n, s, q = _read(rng, name, length)
        add(n, s, q)

    def fill_to(target: int):
        while target - len(out) > 720:
            ordinary(b"r%d" % len(out))
        gap = target - len(out)
        assert gap > 66
        ordinary(b"f" * (gap - 66), 30)  # (a record of 30 bases takes 66 bytes and its name)
        assert len(out) == target

    good = rng.choice(ALPHABET[:8], 151).astype(np.uint8).tobytes()
    high = b"I" * 151
    fill_to(tile)
    assert out[tile - 1] == 0x0A
    fill_to(2 * tile - 44)
    add(b"s2", good, high)
    assert out[2 * tile - 40:2 * tile + 111] == good
    fill_to(3 * tile - 44)
    bases = bytearray(good)
    quals = bytearray(high)
    bases[38:43] = b"NNNNN"
    quals[30:51] = b"&" * 21
    add(b"s3", bytes(bases), bytes(quals))
    assert out[3 * tile - 2:3 * tile + 3] == b"NNNNN" and len(out) - 152 > 3 * tile
    fill_to(4 * tile - 198)
    quals = bytearray(high)
    quals[35:46] = b"&" * 11
    add(b"s4", good, bytes(quals))
    assert out[4 * tile - 5:4 * tile + 6] == b"&" * 11
    for i in range(3):
        ordinary(b"t%d" % i)
    assert out[tile] == ord("@") and 4 * tile < len(out) < 2_000_000
    return bytes(out)


def test_files_across_tile_edges(product_lib, tmp_path):
    from matchtigs_amd import api

    tiny = tmp_path / "tiny.fq"
    tiny.write_bytes(b"@r\nAC\n+\nII\n")
    tile = api.read_fastq(str(tiny))[1].tile_bytes
    text = _multi_tile_text(tile)
    assert len(text) > 4 * tile  # five tiles
    p = tmp_path / "tiles.fq"
    p.write_bytes(text)
    first = {}
    for q in (0, 6, 20):
        first[q] = _check(api, p, text, q)
    # the run across the third edge cuts a piece only from Q = 6 on (its `N`s at every Q)
    assert len(first[6][1]) > len(first[0][1])
    # two calls give identical arrays
    for q, (d, o) in first.items():
        again, _ = api.read_fastq(str(p), q)
        d2, o2 = again.arrays()
        assert np.array_equal(d, d2) and np.array_equal(o, o2)
    # a .gz copy gives the same result
    with gzip.open(str(p) + ".gz", "wb") as f:
        f.write(text)
    for q in (0, 20):
        d2, o2 = _check(api, str(p) + ".gz", text, q)
        assert np.array_equal(first[q][0], d2) and np.array_equal(first[q][1], o2)
    times = api.last_fastq_times()
    assert set(times) == {"read_ms", "upload_ms", "lines_ms", "pieces_ms", "download_ms", "total_ms"} and times["total_ms"] > 0


def test_many_short_records(product_lib, tmp_path):
    """5000 reads of 0 .. 8 bases: more records than one block of the offset scan takes (2048), many line ends per thread."""
    from matchtigs_amd import api

    rng = np.random.default_rng(8)
    text = F.fastq_text([_read(rng, b"s%d" % i, int(rng.integers(0, 9))) for i in range(5000)], eol=b"\r\n")
    p = tmp_path / "short.fq"
    p.write_bytes(text)
    _check(api, p, text, 0)
    _check(api, p, text, 20)


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_files(product_lib, tmp_path, name):
    from matchtigs_amd import api

    text, record, line, reason = MALFORMED[name]
    assert F.first_error(text) == (record, line, reason)
    p = tmp_path / "bad.fq"
    p.write_bytes(text)
    for named in (False, True):
        with pytest.raises(ValueError) as e:
            api.read_fastq(str(p), 0, named=named)
        assert str(e.value) == F.error_message(p, record, line, reason)
        # a well-formed file still reads correctly in the same process
        good = tmp_path / "good.fq"
        good.write_bytes(HAND["n_at_both_ends_and_inside"][0])
        _check(api, good, HAND["n_at_both_ends_and_inside"][0], 0)


@pytest.mark.parametrize("early, late", [("quality", "header"), ("separator", "quality"), ("length", "length")])
def test_the_earlier_of_two_bad_records_is_named(product_lib, tmp_path, early, late):
    """Two bad records, one per tile -- found by different kernels (structure: one thread per record; quality: the tile kernels)."""
    from matchtigs_amd import api

    def broken(kind, i):
        n, s, q = _read(rng, b"r%d" % i, 151)
        if kind == "quality":
            return b"@" + n + b"\n" + s + b"\n+\n" + q[:70] + b" " + q[71:] + b"\n"
        if kind == "header":
            return b">" + n + b"\n" + s + b"\n+\n" + q + b"\n"
        if kind == "separator":
            return b"@" + n + b"\n" + s + b"\n-\n" + q + b"\n"
        return b"@" + n + b"\n" + s + b"\n+\n" + q[:-1] + b"\n"

    rng = np.random.default_rng(4)
    tiny = tmp_path / "tiny.fq"
    tiny.write_bytes(b"@r\nAC\n+\nII\n")
    tile = api.read_fastq(str(tiny))[1].tile_bytes
    per_tile = tile // 312 + 1
    recs = [F.fastq_text([_read(rng, b"r%d" % i, 151)]) for i in range(3 * per_tile)]
    a, b = per_tile // 2, 2 * per_tile + per_tile // 2
    recs[a], recs[b] = broken(early, a), broken(late, b)
    text = b"".join(recs)
    starts = np.cumsum([0] + [len(r) for r in recs])
    assert starts[a + 1] < tile and starts[b] > 2 * tile  # the first in tile 0, the second in tile 2 or later
    want = F.first_error(text)
    assert want[0] == a and want[2] == {"quality": F.BAD_QUALITY, "separator": F.BAD_SEPARATOR, "length": F.BAD_LENGTH}[early]
    p = tmp_path / "two.fq"
    p.write_bytes(text)
    with pytest.raises(ValueError) as e:
        api.read_fastq(str(p), 20)
    assert str(e.value) == F.error_message(p, *want)
    good = b"".join(r for i, r in enumerate(recs) if i not in (a, b))
    p.write_bytes(good)
    _check(api, p, good, 20)
