"""Colours on the GPU against the restatement (kmer_color_ref.py), as exact integers: the coloured compaction -- store,
counts, masks, per-colour counts, the matrix of shared k-mers, the occupancy -- at the k where the code takes another path (4, 31 and 32
on either side of the narrow / wide switch, 33) and m in {1, 2}, with 1, 3 and 64 colours, colour 63 in use, a colour without a
window, short records whose colours change inside a thread's run of 64 positions, a k-mer on opposite strands in two colours and a
closed walk; the statistics kernel at fewer than 64 k-mers, at a count that is no multiple of 64, where a wave takes more than one
block, and at the dense extreme; the coloured index and its query on the query set of test_gpu_kmer_abundance.py."""
import random

import numpy as np
import pytest

import kmer_abundance_ref as KA
import kmer_color_ref as R
import test_gpu_kmer_abundance as TA
from matchtigs_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
KS = [4, 31, 32, 33]
ALL = 2 ** 64 - 1
SHORT_ONLY = {1: 0, 3: 1, 64: 5}  # the colour whose records are all shorter than k (with one colour there is no such colour)
PALETTE = {1: [0] * 6, 3: [0, 2, 0, 2, 2, 0], 64: [0, 63, 17, 31, 32, 62]}  # sample -> colour


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction and the k-mer index have no CPU path")
    return torch


def _dna(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _records(k):
    """-> [(record, sample)]; sample 6 = the one whose records are all shorter than k. A 400-base genome in pieces of either strand
    from six samples, a run of sixty records of 5 .. 40 bases that walk the genome with the sample changing from record to record, the
    periodic record of kmer_abundance_ref.reads_case() (a closed walk at k > 9), a stretch forwards in one sample and as its reverse
    complement in another, and records shorter than k here and there."""
    rng = random.Random(100 + k)
    genome = _dna(rng, 400, "AACCG" if k == 4 else "ACGT")
    out = []
    for i in range(10):
        at = rng.randint(0, 400 - 120)
        s = genome[at:at + rng.randint(k + 5, 120)]
        out.append((synth.revcomp(s) if i % 2 else (s.lower() if i % 3 == 0 else s), i % 6))
    at = 0
    for i in range(60):  # about 1 300 bases: twenty threads' runs, each crossing several records
        at = (at + rng.randint(1, 9)) % (400 - 40)
        s = genome[at:at + rng.randint(5, 40)]
        out.append((synth.revcomp(s) if i % 3 == 1 else s, (i * 5 + 1) % 6))
    out.append((KA.reads_case()[1][-1], 3))
    opposite = _dna(rng, k + 3)  # nowhere else
    out += [(opposite, 1), (synth.revcomp(opposite), 4)]
    for n in (0, 1, k - 1, k // 2):
        out.insert(rng.randint(0, len(out)), (_dna(rng, n), 6))
    return out


def _case(k, C):
    """-> (records, their colours) for C colours."""
    pairs = _records(k)
    return [r for r, _ in pairs], [SHORT_ONLY[C] if s == 6 else PALETTE[C][s] for _, s in pairs]


@pytest.fixture(scope="module", params=[(k, C) for k in KS for C in (1, 3, 64)], ids=lambda p: f"k{p[0]}-C{p[1]}")
def case(request):
    k, C = request.param
    return (k, C) + _case(k, C)


def _assert_colors_equal_ref(col, want, C):
    assert col.n_colors == C and col.kmer_colors.dtype == np.uint64 and col.kmer_colors.tolist() == want["kmer_colors"]
    print("per_color", col.per_color.tolist(), want["per_color"])
    assert col.per_color.dtype == np.uint64 and col.per_color.tolist() == want["per_color"]
    assert col.shared.dtype == np.uint64 and col.shared.shape == (C, C) and col.shared.tolist() == want["shared"]
    assert col.occupancy.dtype == np.uint64 and col.occupancy.tolist() == want["occupancy"]
    assert col.core == want["occupancy"][C] and col.private == want["occupancy"][1]
    assert np.array_equal(col.shared, col.shared.T) and np.array_equal(np.diag(col.shared), col.per_color)


def test_the_cases_hold_what_they_are_for(case):
    k, C, recs, colors = case
    assert sum(1 for r in recs if len(r) < k) >= 4 and all(len(r) < k for r, c in zip(recs, colors) if C > 1 and c == SHORT_ONLY[C])
    assert (max(colors) == 63 and len(set(colors)) < 10) if C == 64 else max(colors) == C - 1
    off = np.cumsum([0] + [len(r) for r in recs])
    changes = [len({colors[i] for i in range(len(recs)) if off[i] < p + 64 and off[i + 1] > p and len(recs[i]) >= 5}) for p in range(0, off[-1], 64)]
    assert max(changes) >= (3 if C == 64 else min(C, 2))  # a thread's 64 positions see several colours (C = 3: two have windows)
    masks = R.kmer_masks(recs, colors, k)
    if C > 1:
        assert sum(1 for m in masks.values() if bin(m).count("1") >= 2) > 20 and sum(1 for m in masks.values() if bin(m).count("1") == 1) >= 3
    if C == 64:  # the two records of opposite strands (samples 1 and 4): colours 63 and 32, a 64-bit shift
        assert any(m == (1 << 63) | (1 << 32) for m in masks.values())


@pytest.mark.parametrize("m", [1, 2])
def test_compaction_equals_the_restatement(gpu, case, m):
    k, C, recs, colors = case
    unitigs, stats, closed, ab, want = R.compact_colored(recs, colors, C, k, m)
    assert stats["distinct_kmers"] > 0 and (k < 10 or any(closed))
    store, c, a, col = api.compact_unitigs_colored(recs, k, colors, C, min_abundance=m)
    assert store.sequences() == unitigs and c == api.Compaction(**stats)
    _assert_colors_equal_ref(col, want, C)
    # everything but the colours is the counted call that hands out the counts
    store2, c2, a2 = api.compact_unitigs_counted(recs, k, m, kmer_counts=True)
    assert store.sequences() == store2.sequences() and np.array_equal(store.arrays()[1], store2.arrays()[1]) and c == c2
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == getattr(a2, f) == ab[f], f
    assert np.array_equal(a.spectrum, a2.spectrum) and np.array_equal(a.unitig_sums, a2.unitig_sums) and a.unitig_sums.tolist() == ab["unitig_sums"]
    assert a.kmer_counts.dtype == np.uint32 and np.array_equal(a.kmer_counts, a2.kmer_counts)
    # per unitig: the union of its k-mers' masks is that of the records that show them
    cuts = np.concatenate([[0], np.cumsum([len(u) - k + 1 for u in unitigs])])
    masks = R.kmer_masks(recs, colors, k)
    for u, lo, hi in zip(unitigs, cuts[:-1], cuts[1:]):
        union = 0
        for i in range(len(u) - k + 1):
            union |= masks[synth.canonical(u[i:i + k])]
        assert int(np.bitwise_or.reduce(col.kmer_colors[lo:hi])) == union
    # twice the same; as arrays; and the older calls answer as before
    cat = np.frombuffer("".join(recs).encode(), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in recs])]).astype(np.uint64)
    for again in (api.compact_unitigs_colored(recs, k, colors, C, m), api.compact_unitigs_colored((cat, off), k, np.array(colors, np.int64), C, m)):
        assert again[0].sequences() == unitigs and again[1] == c
        for f in ("kmer_colors", "per_color", "shared", "occupancy"):
            assert np.array_equal(getattr(again[3], f), getattr(col, f)), f
        assert np.array_equal(again[2].kmer_counts, a.kmer_counts)
    store3, c3, a3 = api.compact_unitigs_counted(recs, k, m, kmer_counts=True)
    assert store3.sequences() == store2.sequences() and c3 == c2 and np.array_equal(a3.kmer_counts, a2.kmer_counts)
    if m == 1:
        plain, cp = api.compact_unitigs(recs, k)
        assert plain.sequences() == unitigs and cp == c
    t, tc = api.last_compact_times(), api.last_kmer_color_times()
    assert t["insert_ms"] > 0 and set(tc) == {"stats_ms", "upload_ms", "pack_ms", "probe_ms", "download_ms"} and tc["stats_ms"] > 0


def test_a_store_goes_in_as_well(gpu):
    recs, colors = _case(31, 3)
    store = api.compact_unitigs(recs, 31)[0]  # its records: the unitigs; colour them by their number
    cols = [i % 3 for i in range(len(store))]
    want = R.compact_colored(store.sequences(), cols, 3, 31)[4]
    out, _, _, col = api.compact_unitigs_colored(store, 31, cols, 3)
    assert out.sequences() == store.sequences()
    _assert_colors_equal_ref(col, want, 3)


@pytest.mark.parametrize("k", KS)
def test_empties(gpu, k):
    rng = random.Random(k)
    for recs in ([], [""], [_dna(rng, n) for n in (k - 1, 0, k // 2)], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        n = len(recs) if isinstance(recs, list) else 0
        store, c, a, col = api.compact_unitigs_colored(recs, k, [2] * n, 3)
        assert len(store) == 0 and c.distinct_kmers == 0 and len(a.kmer_counts) == 0 and a.kmer_counts.dtype == np.uint32
        assert col.n_colors == 3 and len(col.kmer_colors) == 0 and col.kmer_colors.dtype == np.uint64
        assert not col.per_color.any() and not col.shared.any() and not col.occupancy.any() and col.shared.shape == (3, 3)
        assert np.isnan(col.jaccard()).all()
    recs = [_dna(rng, 3 * k), _dna(rng, 2 * k)]
    store, c, a, col = api.compact_unitigs_colored(recs, k, [0, 1], 2, min_abundance=10 ** 6)  # nothing reaches the threshold
    assert len(store) == 0 and a.distinct_kept == 0 and a.distinct_all > 0 and len(col.kmer_colors) == 0 and not col.occupancy.any()


@pytest.mark.parametrize("bases", [31 + 19, 31 + 69, 31 + 63, 31 + 64])
def test_statistics_of_a_core_of_64_colours(gpu, bases):
    """Every k-mer in every colour: all ones everywhere, the dense extreme; 20 k-mers (fewer than a wave), 70 (no multiple of 64), 64
    and 65 (one block exactly, and one k-mer more)."""
    rec = _dna(random.Random(bases), bases)
    recs, colors = [rec if c % 2 else synth.revcomp(rec) for c in range(64)], list(range(64))
    store, c, a, col = api.compact_unitigs_colored(recs, 31, colors, 64)
    n = bases - 30
    assert c.distinct_kmers == n == len(KA.windows([rec], 31)) == len(set(map(synth.canonical, KA.windows([rec], 31))))
    assert col.kmer_colors.tolist() == [ALL] * n and col.per_color.tolist() == [n] * 64 and (col.shared == n).all()
    assert col.occupancy.tolist() == [0] * 64 + [n] and col.core == n and col.private == 0 and (col.jaccard() == 1.0).all()
    _assert_colors_equal_ref(col, R.compact_colored(recs, colors, 64, 31)[4], 64)


def test_statistics_where_a_wave_takes_more_than_one_block(gpu):
    """About 2 * 10^5 bases in three colours: a genome, a copy with 3 % substitutions, and the reverse complement of a part of it plus
    foreign sequence. More k-mers than the statistics kernel's 512 workgroups take in one block per wave (131 072)."""
    k = 25
    rng = np.random.default_rng(5)
    genome = synth.random_genome(80_000, seed=11, haplotypes=1)[0]
    copy = list(genome)
    for j in np.flatnonzero(rng.random(len(copy)) < 0.03):
        copy[j] = "ACGT"[("ACGT".index(copy[j]) + int(rng.integers(1, 4))) % 4]
    third = synth.revcomp(genome[10_000:40_000]) + synth.random_genome(30_000, seed=12, haplotypes=1)[0]
    recs, colors = [genome, "".join(copy), third], [0, 1, 2]
    masks = R.kmer_masks(recs, colors, k)
    assert len(masks) > 131_072 + 64 and len(masks) % 64
    per_color, shared, occupancy = R.statistics(masks.values(), 3)
    store, c, a, col = api.compact_unitigs_colored(recs, k, colors, 3)
    assert c.distinct_kmers == len(masks)
    print(col.per_color.tolist(), per_color, col.shared.tolist(), shared)
    assert col.per_color.tolist() == per_color and col.shared.tolist() == shared and col.occupancy.tolist() == occupancy
    assert min(occupancy[1:4]) > 1000  # private, shared by two, core: all three kinds are there
    want = [masks[synth.canonical(w)] for w in KA.windows(store.sequences(), k)]
    assert col.kmer_colors.tolist() == want


# ---- the coloured index ----
def _index_case(k, C):
    """test_gpu_kmer_abundance.py's index, weights and query set, plus one mask per window: 0, all C bits and random ones, and over
    record 0 -- which the query's 5 000-base record begins with -- two masks that alternate from window to window."""
    index, weights, query, want_abundance = TA._case(k)
    rng = random.Random(70 + k)
    full = (1 << C) - 1
    n = sum(max(0, len(s) - k + 1) for s in index)
    masks = [rng.choice([0, full, rng.getrandbits(C), rng.getrandbits(C) & rng.getrandbits(C), 1]) for _ in range(n)]
    first = len(index[0]) - k + 1
    masks[:first] = [(full, 0)[i % 2] if C == 1 else (full, 0b101 << 61)[i % 2] for i in range(first)]
    return index, weights, masks, query, want_abundance


@pytest.fixture(scope="module", params=[(k, C) for k in KS for C in (1, 64)], ids=lambda p: f"k{p[0]}-C{p[1]}")
def index_case(request):
    k, C = request.param
    index, weights, masks, query, want_abundance = _index_case(k, C)
    return k, C, index, weights, masks, query, want_abundance, R.color_hits(index, masks, C, query, k)


def _assert_hits_equal_ref(got, want, C, per_window):
    for f in ("kmers", "valid", "found"):
        assert getattr(got, f).dtype == np.uint64 and getattr(got, f).tolist() == want[f], f
    assert got.per_color.dtype == np.uint32 and got.per_color.shape == (len(want["kmers"]), C)
    print(got.per_color.tolist()[:8], want["per_color"][:8])
    assert got.per_color.tolist() == want["per_color"]
    if per_window:
        assert got.per_window.dtype == np.uint64 and got.per_window.tolist() == want["per_window"]
    else:
        assert got.per_window is None


def test_the_index_cases_hold_what_they_are_for(index_case):
    k, C, index, weights, masks, query, _, want = index_case
    long = max(range(len(query)), key=lambda i: len(query[i]))
    base = sum(len(s) for s in query[:long])
    pw = want["per_window"][base:base + len(index[0]) - k + 1]
    print(sum(a != b for a, b in zip(pw, pw[1:])), len(pw))
    assert sum(a != b for a, b in zip(pw, pw[1:])) >= (len(pw) - 1 if k > 4 else 15) and len(pw) > 30  # a flush per window (k = 4: k-mers repeat)
    assert 0 in masks and (1 << C) - 1 in masks and 0 < sum(want["found"]) < sum(want["valid"])
    assert sum(want["found"]) > sum(1 for m in want["per_window"] if m) > 0  # found windows whose mask is 0
    if C == 64:
        assert any(m >> 63 for m in masks) and sum(row[63] for row in want["per_color"]) > 0


def test_color_hits_equal_the_restatement(gpu, index_case):
    k, C, index, weights, masks, query, _, want = index_case
    with api.KmerIndex(index, k, colors=masks, n_colors=C) as ix, api.KmerIndex(index, k) as plain:
        L = _lib.load()
        assert ix.colored and ix.n_colors == C and not ix.weighted and not ix.locating
        assert L.mtg_kmer_index_is_colored(ix._h) == 1 and L.mtg_kmer_index_n_colors(ix._h) == C
        assert L.mtg_kmer_index_is_colored(plain._h) == 0 and L.mtg_kmer_index_n_colors(plain._h) == 0
        assert ix.info.device_bytes == plain.info.device_bytes + 8 * plain.info.slots
        got = ix.color_hits(query, per_window=True)
        _assert_hits_equal_ref(got, want, C, True)
        _assert_hits_equal_ref(ix.color_hits(query), want, C, False)
        cat = np.frombuffer("".join(query).encode(), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(s) for s in query])]).astype(np.uint64)
        again = ix.color_hits((cat, off), per_window=True)
        for f in ("offsets", "kmers", "valid", "found", "per_color", "per_window"):
            assert np.array_equal(getattr(got, f), getattr(again, f)), f
        with pytest.raises(ValueError):
            plain.color_hits(query)
        with pytest.raises(ValueError):
            ix.abundance(query)
    t = api.last_kmer_color_times()
    assert all(v >= 0 for v in t.values()) and t["probe_ms"] > 0


def test_the_other_calls_answer_as_without_colours(gpu, index_case):
    k, C, index, weights, masks, query, want_abundance, want = index_case
    with api.KmerIndex(index, k) as plain, api.KmerIndex(index, k, locate=True, weights=weights) as wl, \
            api.KmerIndex(index, k, colors=masks, n_colors=C) as c, \
            api.KmerIndex(index, k, locate=True, weights=weights, colors=masks, n_colors=C) as both, \
            api.KmerIndex(index, k, weights=weights, colors=masks, n_colors=C) as wc:
        assert (both.weighted, both.colored, both.locating) == (True, True, True) and (wc.weighted, wc.colored, wc.locating) == (True, True, False)
        a = plain.query(query, bits=True)
        for x in (c, both, wc):
            b = x.query(query, bits=True)
            for f in ("kmers", "valid", "found", "valid_bits", "present_bits", "offsets"):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
        la, lb = wl.locate(query), both.locate(query)
        for f in ("kmers", "valid", "found", "offsets", "runs"):
            assert np.array_equal(getattr(la, f), getattr(lb, f)), f
        assert len(la.runs) > 0
        for x in (c, wc):
            with pytest.raises(ValueError):
                x.locate(query)
        ea = wl.abundance(query, per_window=True)
        for x in (both, wc):
            eb = x.abundance(query, per_window=True)
            for f in ("sum", "min", "max", "per_window", "found"):
                assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
            assert eb.sum.tolist() == want_abundance["sum"] and eb.per_window.tolist() == want_abundance["per_window"]
            _assert_hits_equal_ref(x.color_hits(query, per_window=True), want, C, True)
        assert both.info.device_bytes == wl.info.device_bytes + 8 * wl.info.slots
        assert wc.info.device_bytes == plain.info.device_bytes + 12 * plain.info.slots


@pytest.mark.parametrize("k", KS)
def test_empty_indexes_and_queries(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3), "N" + _dna(rng, k), ""]
    for index in ([], [""], [_dna(rng, n) for n in (k - 1, 0, k // 2)], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        for locate in (False, True):
            with api.KmerIndex(index, k, locate=locate, colors=np.zeros(0, np.uint64), n_colors=5) as ix:
                assert ix.colored and ix.info.distinct == ix.info.occurrences == 0
                r = ix.color_hits(full, per_window=True)
                assert r.kmers.tolist() == [k + 4, 2, 0] and r.valid.tolist() == [k + 4, 1, 0] and r.found.tolist() == [0, 0, 0]
                assert r.per_color.shape == (3, 5) and not r.per_color.any() and len(r.per_window) == 3 * k + 4 and not r.per_window.any()
    with api.KmerIndex(full[:1], k, colors=[0b10010] * (k + 4), n_colors=5) as ix:
        for q in ([], [""], ["", ""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
            r = ix.color_hits(q, per_window=True)
            n = len(q) if isinstance(q, list) else 0
            assert len(r.per_window) == 0 and r.per_color.shape == (n, 5) and all(len(getattr(r, f)) == n for f in ("kmers", "valid", "found"))
        r = ix.color_hits(full)
        assert r.found.tolist() == [k + 4, 0, 0] and r.per_color.tolist() == [[0, k + 4, 0, 0, k + 4], [0] * 5, [0] * 5]
    ix.close()
    with pytest.raises(ValueError):
        ix.color_hits(full)


def test_compaction_to_index_to_the_samples(gpu):
    """Compaction -> coloured index of its store -> the input records as queries: every window of a record of colour c is found with
    bit c set."""
    k = 31
    recs, colors = _case(k, 64)
    store, _, ab, col = api.compact_unitigs_colored(recs, k, colors, 64)
    with api.KmerIndex(store, k, weights=ab.kmer_counts, colors=col.kmer_colors, n_colors=64) as ix:
        r = ix.color_hits(recs)
    assert np.array_equal(r.found, r.kmers) and np.array_equal(r.valid, r.kmers)
    assert all(int(r.per_color[i, c]) == int(r.kmers[i]) for i, c in enumerate(colors))
    want = R.color_hits(store.sequences(), col.kmer_colors.tolist(), 64, recs, k)
    assert r.per_color.tolist() == want["per_color"]
