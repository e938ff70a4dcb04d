"""The counted unitig compaction on the GPU (`--min-abundance`, mtg_compact_unitigs_counted): bytes, offsets, Compaction,
every Abundance field and the per-unitig sums of the device against the restatement of the contract (abundance_ref.py); m = 1 against
the plain compaction; errors that vanish; creators taken over all windows; a closed walk that exists only after filtering; the special
shapes; the spectrum's last bin; one hot counter and many workgroups against numpy; a fuzz; determinism."""
import dataclasses

import numpy as np
import pytest

import abundance_ref as A
import compact_ref as R
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu


def _plain(seqs, k):
    from matchtigs_amd import api

    store, c = api.compact_unitigs(seqs, k)
    data, off = store.arrays()
    return data.tobytes().decode(), [int(x) for x in off], c


def _counted(seqs, k, m):
    from matchtigs_amd import api

    store, c, a = api.compact_unitigs_counted(seqs, k, m)
    data, off = store.arrays()
    return data.tobytes().decode(), [int(x) for x in off], c, a


def _abundance_dict(a):
    return {"distinct_all": a.distinct_all, "distinct_kept": a.distinct_kept, "dropped": a.dropped, "max_abundance": a.max_abundance,
            "kept_occurrences": a.kept_occurrences, "spectrum": a.spectrum.tolist(), "unitig_sums": a.unitig_sums.tolist()}


def _check(seqs, k, m):
    """Device output == restatement: bytes, offsets, Compaction, every Abundance field, the per-unitig sums."""
    unitigs, stats, closed, ab = A.compact_counted(seqs, k, m)
    data, off, c, a = _counted(seqs, k, m)
    assert dataclasses.asdict(c) == stats
    assert off == [0] + [int(x) for x in np.cumsum([len(u) for u in unitigs])]
    assert data == "".join(unitigs)
    assert a.spectrum.dtype == np.uint64 and a.spectrum.shape == (256,) and a.unitig_sums.dtype == np.uint64
    assert _abundance_dict(a) == ab
    return unitigs, stats, closed, ab


@pytest.mark.parametrize("k", [2, 3, 4, 15, 31, 32, 33, 64])
def test_m_1_equals_the_plain_compaction(product_lib, k):
    seqs = synth.random_genome(1500, seed=k, haplotypes=4, sub_rate=0.02)
    data, off, c, a = _counted(seqs, k, 1)
    assert (data, off, c) == _plain(seqs, k)
    assert int(a.spectrum.sum()) == a.distinct_all == a.distinct_kept == c.distinct_kmers and a.dropped == 0
    assert a.kept_occurrences == c.windows == int(a.unitig_sums.sum())
    if a.max_abundance < 255:
        assert int((np.arange(256, dtype=np.uint64) * a.spectrum).sum()) == c.windows
    else:
        assert k <= 4  # (only a tiny k repeats a k-mer that often in 6000 bases)
    _check(seqs, k, 1)


def _with_one_error(g):
    at = len(g) // 2
    return g[:at] + ("A" if g[at] != "A" else "C") + g[at + 1:]


@pytest.mark.parametrize("k", [11, 31, 40])
def test_errors_vanish(product_lib, k):
    g = synth.random_genome(300, seed=200 + k, haplotypes=1)[0]
    bad = _with_one_error(g)
    seqs = [g, g, g, bad]
    count = A.abundances(seqs, k)
    true_kmers = set(A.abundances([g], k))
    assert {x for x, c in count.items() if c >= 2} == true_kmers  # S_2 = kmers(G) for this seed
    data, off, c, a = _counted(seqs, k, 2)
    assert (data, off) == _plain([g], k)[:2]  # the same creators (G comes first) and the same set: the same bytes
    assert a.dropped == len(count) - len(true_kmers) > 0 and a.distinct_kept == len(true_kmers) == c.distinct_kmers
    _check(seqs, k, 2)


@pytest.mark.parametrize("k", [11, 31, 40])
def test_creators_come_from_all_windows(product_lib, k):
    """The erroneous record comes first: readings, orientation and order of the kept k-mers follow their positions in it, next to
    k-mers that are dropped."""
    g = synth.random_genome(300, seed=200 + k, haplotypes=1)[0]
    bad = _with_one_error(g)
    want = sorted(synth.canonical(x) for x in R.compact([g], k)[0])
    u, _, _, ab = _check([bad, g, g, g], k, 2)
    assert ab["dropped"] > 0 and sorted(synth.canonical(x) for x in u) == want and u[0] in g
    u, _, _, ab = _check([synth.revcomp(bad), g, g], k, 2)
    assert ab["dropped"] > 0 and sorted(synth.canonical(x) for x in u) == want
    assert synth.revcomp(u[0]) in g and u[0] not in g  # read as in revcomp(G'), the first record


@pytest.mark.parametrize("k", [4, 31, 32])
def test_a_closed_walk_appears_after_filtering(product_lib, k):
    if k == 4:
        circ, at, tail = "CGCCTGATAC", 4, "AGT"
    else:
        circ, at = synth.random_genome(3 * k + 7, seed=300 + k, haplotypes=1)[0], 5
        tail = ("A" if circ[at + k - 1] != "A" else "C") + synth.random_genome(10, seed=400 + k, haplotypes=1)[0]
    ring = circ + circ[:k - 1]
    seqs = [ring, ring, (circ + circ)[at:at + k - 1] + tail]  # the last record leaves the circle through a branch seen once
    u, stats, closed, _ = _check(seqs, k, 2)
    assert stats["closed_walks"] == 1 and closed == [True] and u == [ring]  # ... and starts at its leader, the first window
    _, stats, closed, _ = _check(seqs, k, 1)
    assert stats["closed_walks"] == 0 and not any(closed)


@pytest.mark.parametrize("k", [4, 31, 32, 40])
def test_special_shapes(product_lib, k):
    g = synth.random_genome(300, seed=100 + k, haplotypes=1)[0]
    stem = g[:k + 6]
    shapes = [
        [g[:k - 1], g, "", g[5:k + 3], "A", g[100:], g[7:k + 6]],   # records shorter than k and empty records mixed in
        [g.lower(), g[:100], g[50:200].lower()],                     # lower case
        [stem + "ACG" + synth.revcomp(stem), stem],                  # a hairpin, its stem once more
        [g[:k + 10], synth.revcomp(g[:k + 10]), g[:k]],              # k-mers seen once on each strand: abundance 2
    ]
    if k % 2 == 0:                                                   # an even-k palindromic k-mer seen twice
        half = g[:k // 2]
        pal = half + synth.revcomp(half)
        shapes.append([g[20:60] + pal + g[80:120], pal])
        assert A.abundances(shapes[-1], k)[pal] == 2 or k < 31
    if k >= 31:  # (a random piece of 41 bases repeats no 31-mer)
        assert set(A.abundances(shapes[3], k).values()) == {2, 3}
    for seqs in shapes:
        for m in (1, 2, 3):
            _check(seqs, k, m)
    # a threshold above the largest abundance: an empty store, zero unitigs, a spectrum that is still complete
    seqs = shapes[3]
    top = max(A.abundances(seqs, k).values())
    u, stats, _, ab = _check(seqs, k, top + 1)
    assert u == [] and stats["unitigs"] == 0 and stats["distinct_kmers"] == 0 and stats["windows"] > 0
    assert sum(ab["spectrum"]) == ab["distinct_all"] > 0 and ab["kept_occurrences"] == 0 and ab["max_abundance"] == top
    data, off, c, a = _counted(seqs, k, top + 1)
    assert (data, off, len(a.unitig_sums)) == ("", [0], 0)


def test_the_last_bin_of_the_spectrum(product_lib):
    data, off, c, a = _counted(["A" * 600], 5, 1)
    assert a.max_abundance == 596 and a.spectrum[255] == 1 and int(a.spectrum.sum()) == 1 and a.unitig_sums.tolist() == [596]
    assert data == "AAAAA" and c.closed_walks == 1
    _check(["A" * 600], 5, 596)
    _check(["A" * 600], 5, 597)
    # abundance exactly 254 and exactly 255 land in bins 254 and 255
    seqs = ["A" * (254 + 4), "C" * (255 + 4)]
    _, _, _, ab = _check(seqs, 5, 255)
    assert ab["spectrum"][254] == 1 and ab["spectrum"][255] == 1 and ab["distinct_kept"] == 1 and ab["unitig_sums"] == [255]
    _, _, _, ab = _check(seqs + ["G" * 5], 5, 1)  # ... and one more occurrence on the other strand moves 255 no further
    assert ab["spectrum"][254] == 1 and ab["spectrum"][255] == 1 and ab["max_abundance"] == 256


def test_one_hot_counter(product_lib):
    """2^20 windows of one k-mer: every window adds to the same counter."""
    n, k = 1 << 20, 31
    data, off, c, a = _counted((np.full(n, ord("A"), np.uint8), np.array([0, n], np.uint64)), k, 2)
    assert data == "A" * k and off == [0, k] and c.unitigs == 1 and c.closed_walks == 1 and c.windows == n - 30
    assert (a.distinct_all, a.distinct_kept, a.max_abundance, a.kept_occurrences) == (1, 1, n - 30, n - 30)
    assert a.unitig_sums.tolist() == [n - 30] and a.spectrum[255] == 1 and int(a.spectrum.sum()) == 1


_CODE = np.full(256, 255, np.uint8)
_CODE[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)


def _canonical_codes(data, off, k):
    """numpy: the canonical 2-bit code (k <= 31) of every window, in position order, and the record each window lies in."""
    base = _CODE[data].astype(np.uint64)
    n = len(base) - k + 1
    fwd = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(k):
        b = base[j:j + n]
        fwd |= b << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - b) << np.uint64(2 * j)
    start = np.arange(n, dtype=np.uint64)
    rec = np.searchsorted(off, start, side="right") - 1
    inside = start + np.uint64(k) <= off[rec + 1]
    return np.minimum(fwd, rc)[inside], rec[inside]


def test_many_workgroups_against_numpy(product_lib):
    """2^18 bases: 256 reads of 1024 bases from a 50-kb genome (5x), either strand, 1 % substitutions; k = 31, m = 2."""
    from matchtigs_amd import api

    k, m, n_reads, read_len, genome_len = 31, 2, 256, 1024, 50_000
    rng = np.random.default_rng(5)
    genome = rng.integers(0, 4, genome_len)
    reads = np.empty((n_reads, read_len), np.int64)
    for i, at in enumerate(rng.integers(0, genome_len - read_len + 1, n_reads)):
        r = genome[at:at + read_len]
        reads[i] = 3 - r[::-1] if rng.random() < 0.5 else r
    wrong = rng.random(reads.shape) < 0.01
    reads = np.where(wrong, (reads + rng.integers(1, 4, reads.shape)) % 4, reads)
    data = np.frombuffer(b"ACGT", np.uint8)[reads.reshape(-1)]
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    assert len(data) == 1 << 18
    codes, _ = _canonical_codes(data, off, k)
    distinct, counts = np.unique(codes, return_counts=True)
    kept = counts >= m
    store, c, a = api.compact_unitigs_counted((data, off), k, m)
    assert (a.distinct_all, a.distinct_kept, a.max_abundance) == (len(distinct), int(kept.sum()), int(counts.max()))
    assert a.kept_occurrences == int(counts[kept].sum()) and c.windows == len(codes) and c.distinct_kmers == a.distinct_kept
    assert a.spectrum.tolist() == np.bincount(np.minimum(counts, 255), minlength=256).tolist()
    assert 0 < a.dropped < a.distinct_all and a.max_abundance > m
    u_data, u_off = store.arrays()
    u_codes, u_rec = _canonical_codes(u_data, u_off, k)
    assert np.array_equal(np.sort(u_codes), distinct[kept])  # the unitigs' k-mers are S_m, each k-mer once
    sums = np.zeros(c.unitigs, np.int64)
    np.add.at(sums, u_rec, counts[np.searchsorted(distinct, u_codes)])
    assert a.unitig_sums.tolist() == sums.tolist()


@pytest.mark.parametrize("k", [2, 3, 5, 8, 15, 31, 32, 33])
def test_fuzz(product_lib, k):
    """25 inputs per k (200 in all) of at most 2000 bases over a reduced alphabet, so that repeats are common; m = 1, 2, 3."""
    rng = np.random.default_rng(1000 + k)
    for case in range(25):
        alphabet = ["AC", "ACG", "ACGT", "AT"][case % 4]
        total = int(2000 * rng.random() ** 3)
        seqs = []
        while total > 0:
            n = min(total, int(rng.integers(0, 3 * k + 40)))
            if seqs and rng.random() < 0.4:  # a piece of an earlier record again, on either strand
                src = seqs[int(rng.integers(0, len(seqs)))]
                lo = int(rng.integers(0, len(src) + 1))
                piece = src[lo:lo + n]
                piece = synth.revcomp(piece) if rng.random() < 0.5 else piece
            else:
                piece = "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))
            seqs.append(piece.lower() if rng.random() < 0.1 else piece)
            total -= max(n, 1)
        for m in (1, 2, 3):
            _check(seqs, k, m)


def test_determinism(product_lib):
    seqs = synth.random_genome(50_000, seed=9, haplotypes=4)
    seqs += [synth.revcomp(seqs[1][1000:30_000]), seqs[2][:20_000]]
    before = _plain(seqs, 31)
    for k, m in ((31, 2), (45, 3)):
        a, b = _counted(seqs, k, m), _counted(seqs, k, m)
        assert a[:3] == b[:3] and _abundance_dict(a[3]) == _abundance_dict(b[3])
        assert a[3].dropped > 0 and a[3].distinct_kept > 0
    assert _plain(seqs, 31) == before  # a plain compaction after counted ones returns what it returned before
