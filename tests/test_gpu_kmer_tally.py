"""The k-mer tally on the GPU against the restatement (kmer_tally_ref.py), as exact integers: add's kmers / valid /
found, the counters after one and after two adds as coverage reads them back -- covered / sum / max / per_window, over the index's
own records and over foreign ones with junk --, at the k where the code takes another path (even k with palindromes, 31 and 32 on
either side of the narrow / wide switch, 33), with a record that about 80 threads flush into, records that begin and end inside a
thread's run of 64 positions, one class that hundreds of thousands of windows of a dozen blocks add to, two classes that alternate
window by window, reset, two tallies on one index, the arena's bytes, empty inputs and the command line end to end."""
import gc
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_query_ref as Q
import kmer_tally_ref as T
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [4, 31, 32, 33]
JUNK = "NNNNnnRYKMSWBDHVxX-*.5"  # what a query may hold besides ACGT
FIELDS = ("kmers", "valid", "found", "covered", "sum", "max")


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
    """-> dict(index, first, second, foreign, want...): about 40 index records of 20 .. 300 bases and some shorter than k, with one
    stretch planted twice in one record and, on either strand, in four others; the query set `first` (empty, one-base and (k - 1)-base records, twenty records inside one run of 64, one of 5000 bases, seventy of one
    base, junk, flipped case, both strands), a different set `second`, and a foreign set with junk to ask the coverage of. At k = 4
    the index has no T, so that k-mers with A and T are absent. The restatement's answers are computed here, once."""
    rng = random.Random(2900 + k)
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

    def piece(n):
        s = rng.choice([x for x in index if len(x) >= k + 5]).upper()
        s = synth.revcomp(s) if rng.random() < 0.5 else s
        at = rng.randint(0, max(0, len(s) - n))
        return s[at:at + n]

    def mixed(n_records):
        out = []
        for i in range(n_records):
            s = list(piece(rng.randint(k, 150)) + _dna(rng, rng.randint(0, 40)))
            if i % 3 == 0:
                s[rng.randrange(len(s))] = rng.choice(JUNK)
            out.append(_flip_case(rng, "".join(s)))
        return out

    long = index[0].upper()
    while len(long) < 5000:
        x = rng.random()
        long += piece(rng.randint(k, 200)) if x < 0.6 else _dna(rng, rng.randint(1, 120)) if x < 0.9 else rng.choice(JUNK)
    long = _flip_case(rng, long)
    first = ["", "A", _dna(rng, k - 1), index[0][:k], index[0][1:k + 1].lower(), synth.revcomp(index[0][:k + 4].upper())]
    first += [_flip_case(rng, piece(rng.randint(k, k + 50))) for _ in range(20)]  # records that begin and end inside a run of 64
    first += [long]
    first += ["ACGTN"[i % 5] for i in range(70)]  # seventy records of one base
    first += mixed(12)
    first += [_dna(rng, 2 * k + 7, "AT" if k == 4 else "ACGT"), "N" * (k + 3), "", "ac" + palindrome.lower() + "g", repeat, synth.revcomp(repeat)]
    second = mixed(15) + [synth.revcomp(long.upper())[:1500], "", repeat.lower()]
    foreign = mixed(10) + ["", "N" * k, _dna(rng, 300), long[100:900], "a", palindrome]
    ix = Q.index_set(index, k)
    once, twice = T.tally(ix, [first], k), T.tally(ix, [first, second], k)
    return dict(k=k, index=index, first=first, second=second, foreign=foreign, kmers=ix, once=once, twice=twice,
                add_first=Q.query(ix, first, k), add_second=Q.query(ix, second, k),
                own_once=T.coverage(ix, once, index, k), own_twice=T.coverage(ix, twice, index, k),
                foreign_twice=T.coverage(ix, twice, foreign, k))


@pytest.fixture(scope="module", params=KS, ids=lambda k: f"k{k}")
def case(request):
    return _case(request.param)


def _assert_query(got, want):
    for f in ("kmers", "valid", "found"):
        g = getattr(got, f)
        assert g.dtype == np.uint64 and g.tolist() == want[f], f
    assert got.valid_bits is None and got.present_bits is None


def _assert_coverage(got, want, per_window):
    for f in FIELDS:
        g = getattr(got, f)
        print(f, g.tolist()[:30], want[f][:30])
        assert g.dtype == np.uint64 and g.tolist() == want[f], f
    if per_window:
        assert got.per_window.dtype == np.uint64 and got.per_window.tolist() == want["per_window"]
    else:
        assert got.per_window is None


def test_the_cases_hold_what_they_are_for(case):
    k, first, want = case["k"], case["first"], case["add_first"]
    long = max(range(len(first)), key=lambda i: len(first[i]))
    assert len(first[long]) >= 5000 and len(first[long]) // 64 >= 78
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])  # absent k-mers and invalid windows
    assert sum(1 for s in case["index"] if len(s) < k) >= 4 and any(n == 0 for n in want["kmers"])
    assert sum(1 for s in first if len(s) == 1) >= 70 and any(len(s) == k - 1 for s in first)
    assert max(case["once"].values()) >= 4  # repeats: one class added to from several windows, records and strands
    assert any(case["twice"][x] > case["once"][x] > 0 for x in case["twice"])
    assert k == 4 or set(case["twice"]) - set(case["once"])  # (at k = 4 the first set already shows every k-mer there is)
    own, foreign = case["own_once"], case["foreign_twice"]
    assert 0 < sum(own["covered"]) <= sum(own["found"]) == sum(own["kmers"])  # the index's own records: all found ...
    assert k == 4 or (sum(own["covered"]) < sum(own["found"]) and any(f and not c for f, c in zip(own["found"], own["covered"])))  # ... not all seen
    assert 0 < sum(foreign["covered"]) <= sum(foreign["found"]) < sum(foreign["valid"]) < sum(foreign["kmers"])
    assert any(m > 1 for m in own["max"])
    if k % 2 == 0:  # the palindrome is in the index, the reads show it, and it is counted once per window
        mine = [x for x in case["kmers"] if x == synth.revcomp(x) and x.lower() in first[-3]]
        assert mine and all(case["once"][x] >= 1 for x in mine)


def test_add_and_coverage_equal_the_restatement(gpu, case):
    k, index, first, second, foreign = (case[f] for f in ("k", "index", "first", "second", "foreign"))
    with api.KmerIndex(index, k) as ix, api.KmerTally(ix) as tally:
        assert tally.device_bytes == 8 * ix.info.slots and tally.index is ix
        before = ix.query(first, bits=True)
        zero = tally.coverage(index, per_window=True)
        assert zero.found.tolist() == case["own_once"]["found"] and not zero.covered.any() and not zero.sum.any() and not zero.max.any()
        assert not zero.per_window.any()
        added = tally.add(first)
        _assert_query(added, case["add_first"])
        plain = ix.query(first)
        for f in ("offsets", "kmers", "valid", "found"):  # add answers what query answers
            assert np.array_equal(getattr(added, f), getattr(plain, f)), f
        t = api.last_kmer_tally_times()
        assert set(t) == {"upload_ms", "pack_ms", "probe_ms", "download_ms"} and all(v >= 0 for v in t.values()) and t["probe_ms"] > 0
        _assert_coverage(tally.coverage(index, per_window=True), case["own_once"], True)
        _assert_coverage(tally.coverage(index), case["own_once"], False)
        # a second, different set: the counters accumulate
        cat = np.frombuffer("".join(second).encode(), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(s) for s in second])]).astype(np.uint64)
        _assert_query(tally.add((cat, off)), case["add_second"])  # (the same records as arrays)
        own = tally.coverage(index, per_window=True)
        _assert_coverage(own, case["own_twice"], True)
        _assert_coverage(tally.coverage(foreign, per_window=True), case["foreign_twice"], True)
        _assert_coverage(tally.coverage(foreign), case["foreign_twice"], False)
        again = tally.coverage(index, per_window=True)  # reading changes nothing
        for f in FIELDS + ("offsets", "per_window"):
            assert np.array_equal(getattr(own, f), getattr(again, f)), f
        # the index does not notice
        after = ix.query(first, bits=True)
        for f in ("kmers", "valid", "found", "valid_bits", "present_bits", "offsets"):
            assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
        # reset: all zeros again, and counting starts over
        tally.reset()
        zero = tally.coverage(index, per_window=True)
        assert not zero.covered.any() and not zero.sum.any() and not zero.max.any() and not zero.per_window.any()
        assert zero.found.tolist() == case["own_once"]["found"]
        _assert_query(tally.add(first), case["add_first"])
        _assert_coverage(tally.coverage(index, per_window=True), case["own_once"], True)


def test_the_kinds_of_index_and_two_tallies(gpu):
    """A tally counts alike on a plain, a locating, a weighted and a coloured index, a store goes in like its records, and two
    tallies on one index do not see each other."""
    c = _case(31)
    k, index, first, second = c["k"], c["index"], c["first"], c["second"]
    windows = sum(max(0, len(s) - k + 1) for s in index)
    for kw in (dict(locate=True), dict(weights=[7] * windows), dict(colors=[1] * windows, n_colors=2)):
        with api.KmerIndex(index, k, **kw) as ix, api.KmerTally(ix) as tally:
            tally.add(first)
            _assert_coverage(tally.coverage(index, per_window=True), c["own_once"], True)
    store, _ = api.compact_unitigs(index, k)
    unitigs = store.sequences()
    with api.KmerIndex(store, k) as ix, api.KmerTally(ix) as a, api.KmerTally(ix) as b:
        _assert_query(a.add(first), c["add_first"])
        _assert_query(b.add(second), c["add_second"])
        _assert_query(b.add(store), Q.query(c["kmers"], unitigs, k))  # (the _store entry points)
        both = T.tally(c["kmers"], [second, unitigs], k)
        _assert_coverage(a.coverage(store, per_window=True), T.coverage(c["kmers"], c["once"], unitigs, k), True)
        _assert_coverage(b.coverage(store, per_window=True), T.coverage(c["kmers"], both, unitigs, k), True)
        a.reset()
        assert not a.coverage(store).sum.any()
        _assert_coverage(b.coverage(unitigs), T.coverage(c["kmers"], both, unitigs, k), False)


@pytest.mark.parametrize("k", [31, 32])
def test_contention_and_run_merging(gpu, k):
    """One class that 2 (200000 - k + 1) windows of about a dozen blocks add to, every thread merging its 64 hits into one atomic;
    then two classes that alternate window by window, where nothing merges."""
    rng = random.Random(k)
    n = 200_000
    index = [_dna(rng, 150), "A" * (k + 5), ("AC" * k)[:k + 7], _dna(rng, 90), "acgt"]
    kmers = Q.index_set(index, k)
    homopolymer, alternating = "A" * n + "T" * n, ("AC" * (n // 2))
    want = T.tally(kmers, [[homopolymer]], k)
    straddling = k - 1  # the windows with both A and T: absent
    assert want == {"A" * k: 2 * (n - k + 1)} and 2 * n - k + 1 - straddling == 2 * (n - k + 1)
    assert (2 * n + 63) // 64 // 256 >= 12  # blocks of 256 threads with 64 window starts each
    with api.KmerIndex(index, k) as ix, api.KmerTally(ix) as tally:
        r = tally.add([homopolymer])
        assert r.kmers.tolist() == r.valid.tolist() == [2 * n - k + 1] and r.found.tolist() == [2 * (n - k + 1)]
        _assert_coverage(tally.coverage(index, per_window=True), T.coverage(kmers, want, index, k), True)
        cov = tally.coverage(["T" * k, "A" * (k + 1), ("CA" * k)[:k]], per_window=True)
        assert cov.found.tolist() == [1, 2, 1] and cov.covered.tolist() == [1, 2, 0] and cov.max.tolist() == [2 * (n - k + 1)] * 2 + [0]
        assert cov.sum.tolist() == [2 * (n - k + 1), 4 * (n - k + 1), 0]
        tally.reset()
        r = tally.add([alternating, "", alternating.lower()])
        want = T.tally(kmers, [[alternating] * 2], k)
        each = n - k + 1  # per record, split between the window that starts with A and the one that starts with C
        assert len(want) == 2 and sorted(want.values()) == [2 * (each // 2), 2 * (each - each // 2)]
        assert r.found.tolist() == [each, 0, each]
        _assert_coverage(tally.coverage(index, per_window=True), T.coverage(kmers, want, index, k), True)


@pytest.mark.parametrize("k", [5, 34])
def test_the_arena_gets_its_bytes_back(gpu, k):
    """test_gpu_kmer_index_memory.py's method: warmed once, then the arena's live bytes before the tally and after its close."""
    rng = random.Random(4100 + k)
    index = [_dna(rng, rng.randint(90, 120)) for _ in range(5)] + [_dna(rng, k - 1)]
    reads = [index[0][10:70] + "N" + index[2][5:60], _dna(rng, 100), _dna(rng, k - 1), synth.revcomp(index[4]), index[1][20:20 + 2 * k]]
    kmers = Q.index_set(index, k)
    want = T.coverage(kmers, T.tally(kmers, [reads], k), index, k)
    assert 0 < sum(want["covered"]) < sum(want["found"])

    def run(ix, check):
        with api.KmerTally(ix) as tally:
            live = api.device_arena_stats(0)["live_bytes"]
            tally.add(reads)
            got = tally.coverage(index, per_window=True)
            tally.reset()
            tally.add([])
            assert api.device_arena_stats(0)["live_bytes"] == live  # add, coverage and reset keep nothing
            if check:
                _assert_coverage(got, want, True)
            return live, tally.device_bytes

    with api.KmerIndex(index, k) as ix:
        run(ix, False)  # (chunks taken from the driver, code objects loaded)
        gc.collect()
        before = api.device_arena_stats(0)["live_bytes"]
        live, device_bytes = run(ix, True)
        after = api.device_arena_stats(0)["live_bytes"]
        assert device_bytes == 8 * ix.info.slots and live - before >= device_bytes
        assert after == before, f"the tally left {after - before} bytes of the arena live"


@pytest.mark.parametrize("k", KS)
def test_empties(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3), "N" + _dna(rng, k), ""]
    for index in ([], [""], [_dna(rng, n) for n in (k - 1, 0, k // 2)], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        with api.KmerIndex(index, k) as ix, api.KmerTally(ix) as tally:  # an index without windows
            assert ix.info.occurrences == 0 and tally.device_bytes == 8 * ix.info.slots > 0
            r = tally.add(full)
            assert r.kmers.tolist() == [k + 4, 2, 0] and r.valid.tolist() == [k + 4, 1, 0] and r.found.tolist() == [0, 0, 0]
            c = tally.coverage(full, per_window=True)
            assert c.kmers.tolist() == [k + 4, 2, 0] and c.valid.tolist() == [k + 4, 1, 0]
            assert c.found.tolist() == c.covered.tolist() == c.sum.tolist() == c.max.tolist() == [0, 0, 0]
            assert len(c.per_window) == 3 * k + 4 and not c.per_window.any()
    with api.KmerIndex(full[:1], k) as ix, api.KmerTally(ix) as tally:
        for q in ([], [""], ["", ""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):  # an empty query
            n = len(q) if isinstance(q, list) else 0
            r = tally.add(q)
            assert all(len(getattr(r, f)) == n for f in ("kmers", "valid", "found"))
            c = tally.coverage(q, per_window=True)
            assert len(c.per_window) == 0 and all(len(getattr(c, f)) == n and not getattr(c, f).any() for f in FIELDS)
        r = tally.add(["N" * (k + 5), "ACGT"[:k - 1], "ac-" * k])  # a query with no valid window
        assert r.kmers.tolist() == [6, 0, 2 * k + 1] and not r.valid.any() and not r.found.any()
        c = tally.coverage(full)
        assert c.found.tolist() == [k + 4, 0, 0] and not c.covered.any() and not c.sum.any() and not c.max.any()
        tally.add(full)
        tally.add([synth.revcomp(full[0]).lower()])
        c = tally.coverage(full)
        assert c.covered.tolist() == [k + 4, 0, 0] and c.sum.tolist() == [2 * (k + 4), 0, 0] and c.max.tolist() == [2, 0, 0]
    with pytest.raises(ValueError, match="the tally is closed"):
        tally.add(full)
    with api.KmerIndex(full[:1], k) as ix:
        tally = api.KmerTally(ix)
    with pytest.raises(ValueError, match="the index is closed"):
        tally.coverage(full)
    tally.close()


# ---- the command line ----
K_CLI = 21


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def _reads(rng, genome, n, length):
    out = []
    for _ in range(n):
        at = int(rng.integers(0, len(genome) - length + 1))
        r = genome[at:at + length]
        out.append(synth.revcomp(r) if rng.random() < 0.5 else r)
    return out


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """A synthetic genome of 20 kb in two haplotypes as the input; sample 1: FASTQ reads of haplotype 0 with low-quality bases;
    sample 2: gzipped FASTA reads of a mutated copy, with an N and lower case here and there."""
    rng = np.random.default_rng(29)
    d = tmp_path_factory.mktemp("kmer_tally_cli")
    haplotypes = synth.random_genome(20_000, seed=29, haplotypes=2)
    (d / "genome.fa").write_text("".join(f">h{i}\n{h}\n" for i, h in enumerate(haplotypes)))
    fq, masked = [], []
    for i, r in enumerate(_reads(rng, haplotypes[0], 300, 120)):
        qual = np.where(rng.random(len(r)) < 0.03, ord("#"), ord("I")).astype(np.uint8)  # Phred 2 and 40
        fq.append(f"@r{i}\n{r}\n+\n{qual.tobytes().decode()}\n")
        masked.append("".join("N" if q == ord("#") else c for c, q in zip(r, qual.tolist())))
    (d / "s1.fq").write_text("".join(fq))
    mutated = list(haplotypes[1])
    for j in np.flatnonzero(rng.random(len(mutated)) < 0.01):
        mutated[j] = "ACGT"[("ACGT".index(mutated[j]) + int(rng.integers(1, 4))) % 4]
    fa = _reads(rng, "".join(mutated), 250, 150)
    fa = [(r[:40] + "N" + r[41:]) if i % 9 == 0 else r.lower() if i % 7 == 0 else r for i, r in enumerate(fa)]
    with gzip.open(d / "s2.fa.gz", "wt") as f:
        f.write("".join(f">m{i}\n{r[:70]}\n{r[70:]}\n" for i, r in enumerate(fa)))
    (d / "q.fa").write_text(f">q0\n{haplotypes[0][:500]}\n>q1\n{'ACGT' * 20}\n")
    return d, masked, fa


@pytest.fixture(scope="module")
def counted(product_lib, cli_inputs):
    """The count run alone -> (paths, the restatement's bytes of its `--count-out`)."""
    d, masked, fa = cli_inputs
    p = {n: str(d / n) for n in ("genome.fa", "s1.fq", "s2.fa.gz", "q.fa", "u.fa", "depth.tsv", "u2.fa", "depth2.tsv.gz", "r2.tsv", "p2.txt", "r0.tsv",
                                 "p0.txt")}
    p["count"] = ("--count-fa", p["s1.fq"], "--count-fa", p["s2.fa.gz"], "--count-min-base-quality", "20")
    r = _cli("--seq-in", p["genome.fa"], "-k", str(K_CLI), "--unitigs-fa-out", p["u.fa"], *p["count"], "--count-out", p["depth.tsv"])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return p, r.stderr, T.count_tsv(_fasta(p["u.fa"]), [masked, fa], [p["s1.fq"], p["s2.fa.gz"]], K_CLI)


def test_cli_count_out_equals_the_restatement(counted):
    p, stderr, want = counted
    unitigs = _fasta(p["u.fa"])
    got = Path(p["depth.tsv"]).read_bytes()
    assert got == want
    rows = [line.split("\t") for line in got.decode().splitlines()[1:]]
    assert len(rows) == len(unitigs) > 10 and any(int(x[2]) and int(x[3]) > int(x[2]) for x in rows)  # depth above 1
    assert any(int(x[4]) == 0 for x in rows) and any(0 < int(x[2]) < int(x[1]) for x in rows)
    lines = [l for l in stderr.splitlines() if l.startswith("Counting ")]
    assert len(lines) == 2 and lines[0].startswith(f"Counting {p['s1.fq']}: 300 records, ")
    assert f"of {len(unitigs)} unitigs covered, mean depth " in lines[0] and " valid, " in lines[1] and " found (" in lines[1]


def test_cli_count_beside_the_queries(counted):
    """gzip, and the count on the index the queries built: the same bytes; the queries' outputs are those of a run without the count."""
    p, _, want = counted
    r = _cli("--seq-in", p["genome.fa"], "-k", str(K_CLI), "--unitigs-fa-out", p["u2.fa"], *p["count"], "--count-out", p["depth2.tsv.gz"],
             "--compression-level", "9", "--query-fa", p["q.fa"], "--query-out", p["r2.tsv"], "--query-presence-out", p["p2.txt"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert gzip.open(p["depth2.tsv.gz"], "rb").read() == want and Path(p["u2.fa"]).read_bytes() == Path(p["u.fa"]).read_bytes()
    r = _cli("--seq-in", p["genome.fa"], "-k", str(K_CLI), "--query-fa", p["q.fa"], "--query-out", p["r0.tsv"], "--query-presence-out", p["p0.txt"])
    assert r.returncode == 0, r.stderr[-3000:]
    for a, b in (("r2.tsv", "r0.tsv"), ("p2.txt", "p0.txt")):
        assert Path(p[a]).read_bytes() == Path(p[b]).read_bytes() and Path(p[a]).stat().st_size > 0, a
