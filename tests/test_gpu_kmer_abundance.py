"""K-mer abundances on the GPU against the restatement (kmer_abundance_ref.py), as exact integers: the per-k-mer
counts of the counted compaction (compact_unitigs_counted(kmer_counts=True)), the weighted index (KmerIndex(weights=...)) and its
abundance query -- kmers / valid / found / sum / min / max / per_window --, at the k where the code takes another path (even k with
palindromes, 31 and 32 on either side of the narrow / wide switch, 33), with weights that make a 32-bit sum wrap, a record that
about 80 threads flush into, records that begin and end inside a thread's run of 64 positions, and empty inputs."""
import random

import numpy as np
import pytest

import abundance_ref as A
import kmer_abundance_ref as R
from matchtigs_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
KS = [4, 31, 32, 33]
JUNK = "NNNNnnRYKMSWBDHVxX-*.5"  # what a query may hold besides ACGT
FULL = 0xFFFFFFFF
K_READS = 21


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the k-mer index has no CPU path")
    return torch


def _dna(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _flip_case(rng, s):
    return "".join(c.lower() if rng.random() < 0.3 else c for c in s)


def _case(k):
    """-> (index, weights, query, want): about 40 index records of 20 .. 300 bases and some shorter than k, with one stretch planted
    twice in one record and, on either strand, in four others; random uint32 weights with 0 and 2^32 - 1 among them, 2^32 - 1 on the
    first five windows of record 0; and the query set the module's docstring lists. At k = 4 the index has no T, so that k-mers
    with A and T are absent."""
    rng = random.Random(9000 + k)
    letters = "AACCG" if k == 4 else "ACGT"
    repeat = _dna(rng, k + 10, letters)
    half = _dna(rng, k // 2, "CG" if k == 4 else "ACGT")
    palindrome = half + synth.revcomp(half)
    index = [_dna(rng, k + 40, letters)]
    for i in range(33):
        s = _dna(rng, rng.randint(20, 300), letters)
        if i % 8 == 0:
            s = s[:len(s) // 2] + (repeat if i % 16 == 0 else synth.revcomp(repeat)) + s[len(s) // 2:]
        if i == 5:
            s = repeat + s[:30] + repeat + s[30:]
        if i == 3 and k % 2 == 0:  # a k-mer that is its own reverse complement
            s = s[:10] + palindrome + s[10:]
        index.append(_flip_case(rng, s))
    for n in (0, 1, k - 1, k - 1, 2, k):
        index.insert(rng.randint(1, len(index)), _dna(rng, n, letters))
    n_windows = sum(max(0, len(s) - k + 1) for s in index)
    weights = [rng.choice([0, 1, 2, FULL, FULL - 1, rng.getrandbits(32), rng.randint(0, 1000)]) for _ in range(n_windows)]
    weights[:5] = [FULL] * 5

    def piece(n):
        s = rng.choice([x for x in index if len(x) >= k + 5]).upper()
        s = synth.revcomp(s) if rng.random() < 0.5 else s
        at = rng.randint(0, max(0, len(s) - n))
        return s[at:at + n]

    long = index[0].upper()
    while len(long) < 5000:
        x = rng.random()
        long += piece(rng.randint(k, 200)) if x < 0.6 else _dna(rng, rng.randint(1, 120)) if x < 0.9 else rng.choice(JUNK)
    long = _flip_case(rng, long)
    query = ["", "A", _dna(rng, k - 1), index[0][:k], index[0][1:k + 1].lower(), synth.revcomp(index[0][:k + 4].upper())]
    query += [_flip_case(rng, piece(rng.randint(k, k + 50))) for _ in range(20)]  # records that begin and end inside a run of 64
    query += [long]
    query += ["ACGTN"[i % 5] for i in range(70)]  # seventy records of one base
    for i in range(12):
        s = list(piece(rng.randint(k, 150)) + _dna(rng, rng.randint(0, 40)))
        if i % 3 == 0:
            s[rng.randrange(len(s))] = rng.choice(JUNK)
        query.append(_flip_case(rng, "".join(s)))
    query += [_dna(rng, 2 * k + 7, "AT" if k == 4 else "ACGT"), "N" * (k + 3), "", "ac" + palindrome.lower() + "g"]
    return index, weights, query, R.abundance(index, weights, query, k)


@pytest.fixture(scope="module", params=KS)
def case(request):
    return (request.param,) + _case(request.param)


def _assert_equals_ref(got, want, per_window):
    for f, dtype in (("kmers", np.uint64), ("valid", np.uint64), ("found", np.uint64), ("sum", np.uint64), ("min", np.uint32), ("max", np.uint32)):
        g = getattr(got, f)
        print(f, g.tolist()[:30], want[f][:30])
        assert g.dtype == dtype and g.tolist() == want[f], f
    if per_window:
        assert got.per_window.dtype == np.uint32 and got.per_window.tolist() == want["per_window"]
    else:
        assert got.per_window is None
    mean = got.mean
    assert mean.dtype == np.float64 and len(mean) == len(want["found"])
    for m, s, f in zip(mean.tolist(), want["sum"], want["found"]):
        assert (m == s / f) if f else m != m


def test_the_cases_hold_what_they_are_for(case):
    k, index, weights, query, want = case
    long = max(range(len(query)), key=lambda i: len(query[i]))
    base = sum(len(s) for s in query[:long])
    assert len(query[long]) >= 5000 and len(query[long]) // 64 >= 78
    assert want["per_window"][base:base + len(query[long])].count(FULL) >= 3 and want["sum"][long] >= 2 ** 32 and want["max"][long] == FULL
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])  # absent k-mers and invalid windows
    assert 0 in weights and FULL in weights and any(m == 0 and f for m, f in zip(want["min"], want["found"]))
    assert sum(1 for s in index if len(s) < k) >= 4 and len(R.class_weights(index, weights, k)) < len(weights)  # repeated classes
    assert any(n == 0 for n in want["kmers"]) and any(len(s) == k for s in query)
    if k % 2 == 0:  # the palindrome is in the index and the query finds it
        pal = [w for w in R.windows(index, k) if w == synth.revcomp(w)]
        mine = [w.lower() for w in pal if w.lower() in query[-1]]
        assert mine and want["found"][-1] >= 1 and want["per_window"][-len(query[-1]) + query[-1].index(mine[0])] == \
            R.class_weights(index, weights, k)[mine[0].upper()]


def test_abundance_equals_the_restatement(gpu, case):
    k, index, weights, query, want = case
    with api.KmerIndex(index, k, weights=weights) as ix:
        assert ix.weighted and not ix.locating and _lib.load().mtg_kmer_index_is_weighted(ix._h) == 1
        got = ix.abundance(query, per_window=True)
        _assert_equals_ref(got, want, True)
        _assert_equals_ref(ix.abundance(query), want, False)
        again = ix.abundance(query, per_window=True)
        for f in ("offsets", "kmers", "valid", "found", "sum", "min", "max", "per_window"):
            assert np.array_equal(getattr(got, f), getattr(again, f)), f
        # the same records as arrays
        cat = np.frombuffer("".join(query).encode(), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(s) for s in query])]).astype(np.uint64)
        _assert_equals_ref(ix.abundance((cat, off), per_window=True), want, True)
    t = api.last_kmer_abundance_times()
    assert set(t) == {"upload_ms", "pack_ms", "probe_ms", "download_ms"} and all(v >= 0 for v in t.values()) and t["probe_ms"] > 0


def test_query_and_locate_answer_as_without_weights(gpu, case):
    k, index, weights, query, _ = case
    L = _lib.load()
    with api.KmerIndex(index, k) as plain, api.KmerIndex(index, k, locate=True) as loc, \
            api.KmerIndex(index, k, weights=weights) as w, api.KmerIndex(index, k, locate=True, weights=weights) as wl:
        assert [L.mtg_kmer_index_is_weighted(x._h) for x in (plain, loc, w, wl)] == [0, 0, 1, 1]
        assert [L.mtg_kmer_index_is_locating(x._h) for x in (plain, loc, w, wl)] == [0, 1, 0, 1]
        a = plain.query(query, bits=True)
        for x in (w, wl):
            b = x.query(query, bits=True)
            for f in ("kmers", "valid", "found", "valid_bits", "present_bits", "offsets"):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
        c, d = loc.locate(query), wl.locate(query)
        for f in ("kmers", "valid", "found", "offsets", "runs"):
            assert np.array_equal(getattr(c, f), getattr(d, f)), f
        assert len(c.runs) > 0
        with pytest.raises(ValueError):
            w.locate(query)
        for x in (plain, loc):
            with pytest.raises(ValueError):
                x.abundance(query)
        # the weighted and the weighted locating index answer alike
        e, f_ = w.abundance(query, per_window=True), wl.abundance(query, per_window=True)
        for f in ("sum", "min", "max", "per_window", "found"):
            assert np.array_equal(getattr(e, f), getattr(f_, f)), f
        same = lambda i: {f: v for f, v in vars(i.info).items() if f != "device_bytes"}
        assert same(plain) == same(loc) == same(w) == same(wl)
        assert w.info.device_bytes == plain.info.device_bytes + 4 * plain.info.slots
        assert wl.info.device_bytes == loc.info.device_bytes + 4 * loc.info.slots


@pytest.mark.parametrize("k", KS)
def test_empties(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3), "N" + _dna(rng, k), ""]
    for index in ([], [""], [_dna(rng, n) for n in (k - 1, 0, k // 2)], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        for locate in (False, True):
            with api.KmerIndex(index, k, locate=locate, weights=np.zeros(0, np.uint32)) as ix:
                assert ix.weighted and ix.info.distinct == ix.info.occurrences == 0
                r = ix.abundance(full, per_window=True)
                assert r.kmers.tolist() == [k + 4, 2, 0] and r.valid.tolist() == [k + 4, 1, 0]
                assert r.found.tolist() == r.sum.tolist() == r.min.tolist() == r.max.tolist() == [0, 0, 0]
                assert len(r.per_window) == 3 * k + 4 and not r.per_window.any() and np.isnan(r.mean).all()
    with api.KmerIndex(full[:1], k, weights=[9] * (k + 4)) as ix:
        for q in ([], [""], ["", ""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
            r = ix.abundance(q, per_window=True)
            n = len(q) if isinstance(q, list) else 0
            assert len(r.per_window) == 0 and all(len(getattr(r, f)) == n for f in ("kmers", "valid", "found", "sum", "min", "max", "mean"))
        r = ix.abundance(full)
        assert r.found.tolist() == [k + 4, 0, 0] and r.sum.tolist() == [9 * (k + 4), 0, 0] and r.min.tolist() == r.max.tolist() == [9, 0, 0]
    ix.close()
    with pytest.raises(ValueError):
        ix.abundance(full)


def test_wrong_weights_length_is_refused_before_the_library_is_called(product_lib):
    """device_id 99 does not exist: a call that reached the library would abort the process."""
    index = ["ACGTACGTAC", "AC", "GGGTTTAAAC"]  # k = 4: 7 + 0 + 7 windows
    for weights in ([1] * 13, [1] * 15, [], np.ones((2, 7), np.uint32)):
        with pytest.raises(ValueError):
            api.KmerIndex(index, 4, device_id=99, weights=weights)
        with pytest.raises(ValueError):
            api.KmerIndex((np.frombuffer("".join(index).encode(), np.uint8), np.array([0, 10, 12, 22], np.uint64)), 4, device_id=99, weights=weights)


@pytest.fixture(scope="module")
def reads():
    genome, seqs = R.reads_case()
    return genome, seqs, A.abundances(seqs, K_READS)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_compaction_hands_out_the_count_of_every_kmer(gpu, reads, m):
    _, seqs, count = reads
    k = K_READS
    store, c, ab = api.compact_unitigs_counted(seqs, k, m, kmer_counts=True)
    plain_store, plain_c, plain_ab = api.compact_unitigs_counted(seqs, k, m)
    unitigs = store.sequences()
    assert ab.kmer_counts.dtype == np.uint32 and len(ab.kmer_counts) == ab.distinct_kept == c.distinct_kmers > 0
    want = [count[synth.canonical(w)] for w in R.windows(unitigs, k)]
    assert ab.kmer_counts.tolist() == want == R.window_counts(unitigs, seqs, k)
    assert int(ab.kmer_counts.sum(dtype=np.uint64)) == ab.kept_occurrences and min(want) >= m
    cuts = np.concatenate([[0], np.cumsum([len(u) - k + 1 for u in unitigs])])
    assert [int(ab.kmer_counts[a:b].sum(dtype=np.uint64)) for a, b in zip(cuts[:-1], cuts[1:])] == ab.unitig_sums.tolist()
    # everything else is the call without the counts
    assert unitigs == plain_store.sequences() and c == plain_c and plain_ab.kmer_counts is None
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(ab, f) == getattr(plain_ab, f), f
    assert np.array_equal(ab.spectrum, plain_ab.spectrum) and np.array_equal(ab.unitig_sums, plain_ab.unitig_sums)
    assert ab.dropped > 0 or m == 1


def test_nothing_reaches_the_threshold(gpu, reads):
    store, c, ab = api.compact_unitigs_counted(reads[1], K_READS, 10 ** 6, kmer_counts=True)
    assert len(store) == 0 and ab.distinct_kept == 0 and ab.kmer_counts.dtype == np.uint32 and len(ab.kmer_counts) == 0
    store, c, ab = api.compact_unitigs_counted(store, K_READS, 1, kmer_counts=True)  # (an empty store in)
    assert len(store) == 0 and len(ab.kmer_counts) == 0


@pytest.mark.parametrize("m", [1, 2])
def test_reads_to_abundances_of_the_genome(gpu, reads, m):
    """Compaction -> weighted index of its store -> the genome and its reverse complement: every window the reads show at least m
    times is found with exactly its count, every other window is absent."""
    genome, seqs, count = reads
    k = K_READS
    store, _, ab = api.compact_unitigs_counted(seqs, k, m, kmer_counts=True)
    query = [genome, synth.revcomp(genome)]
    with api.KmerIndex(store, k, weights=ab.kmer_counts) as ix:
        r = ix.abundance(query, per_window=True)
    want = [c if c >= m else 0 for s in query for c in [count.get(synth.canonical(s[i:i + k]), 0) for i in range(len(s) - k + 1)] + [0] * (k - 1)]
    assert r.per_window.tolist() == want
    kept = [sum(1 for x in want[i * 600:(i + 1) * 600] if x) for i in (0, 1)]
    assert r.found.tolist() == kept and kept[0] == kept[1] > 100 and r.sum.tolist() == [sum(want[:600]), sum(want[600:])]
    if m > 1:  # the filter dropped windows of the genome that the reads show once
        assert any(0 < count.get(synth.canonical(genome[i:i + k]), 0) < m for i in range(600 - k + 1))
