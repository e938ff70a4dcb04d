"""`locate` on the sparse minimizer index on the GPU (tig_locate_kernel, api.TigIndex.locate): the three counts and the runs
as exact tuples against the locate contract's restatement (kmer_locate_ref.py, which knows nothing about how an index is organised),
every run spelling what it covers, and on the larger cases field for field against api.KmerIndex(locate=True) on the same inputs.
Random pairs over k, m and bucket_limit, the palindromes on which the first passing candidate is not the smallest position, the hand
cases of DESIGN.md 18, low-complexity repeats down the heavy path, run ends and substitutions at every position of a thread's stretch,
awkward inputs, reuse of one index, the memory a locating index adds, and the path through the product."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_locate_ref as LR
import tig_index_cases as cases
import tig_locate_ref as TL
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 3, 5, 16, 31, 32, 33, 64, 101]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the tig index has no CPU path")
    return torch


def _runs(result):
    return [tuple(int(x) for x in row) for row in result.runs[list(LR.FIELDS)].tolist()]


def _assert_equals_ref(ix, index, query, k, what="", want=None):
    """One locate call: the three counts and the runs equal the restatement's, and every run spells. Returns the restatement's result."""
    want = LR.locate(index, query, k) if want is None else want
    got = ix.locate(query)
    assert got.runs.dtype == api.KMER_RUN_DTYPE
    for f in ("kmers", "valid", "found"):
        g = getattr(got, f)
        assert g.dtype == np.uint64 and g.tolist() == want[f], (what, k, ix.info, f, g.tolist()[:20], want[f][:20])
    assert _runs(got) == want["runs"], (what, k, ix.info, _runs(got)[:8], want["runs"][:8])
    for run in want["runs"]:
        assert LR.spells(index, query, run, k), (what, k, run)
    return want


def _assert_same_result(a, b):
    for f in ("offsets", "kmers", "valid", "found", "runs"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def _abutting(runs):
    """Two runs of one query record, the second starting at the window behind the first's last: a repeat (or a strand change) broke it."""
    return any(a[0] == b[0] and a[1] + a[2] == b[1] for a, b in zip(runs, runs[1:]))


@pytest.mark.parametrize("k", KS)
def test_random_pairs(gpu, k):
    rng = random.Random(3020 + k)  # (a seed whose pairs show every kind of run at every k, k = 1 included: the restatement alone says so)
    seen = dict.fromkeys(("minus run", "long run", "broken run", "heavy", "light"), False)
    for i in range(12):
        index, query = cases.random_pair(rng, k)
        want = LR.locate(index, query, k)
        for m in cases.random_ms(k):
            for limit in (None, 1, 2):
                with api.TigIndex(index, k, m, bucket_limit=limit, locate=True) as ix:
                    assert ix.locating
                    _assert_equals_ref(ix, index, query, k, f"pair {i} m={m} limit={limit}", want)
                    counts = ix.query(query)
                    assert (counts.kmers.tolist(), counts.valid.tolist(), counts.found.tolist()) == (want["kmers"], want["valid"], want["found"])
                    seen["heavy"] |= ix.info.heavy_windows > 0
                    seen["light"] |= ix.info.heavy_windows < ix.info.occurrences
        seen["minus run"] |= any(r[3] == 1 for r in want["runs"])
        seen["long run"] |= any(r[2] > 1 for r in want["runs"])
        seen["broken run"] |= _abutting(want["runs"])
    assert all(seen.values()), (k, seen)


@pytest.mark.parametrize("k,m", [(31, 19), (33, 19), (5, 2), (12, 4)])
def test_palindromes(gpu, k, m):
    """A reverse-complement palindrome of k + d bases between flanks: a window's mirrored occurrence lies earlier in the text while its
    anchor lies later, so a probe that returns at the first passing candidate reports the wrong position."""
    rng = random.Random(100 * k + m)
    text, hard = TL.palindrome_case(rng, k, m)
    ref = TL.TigLocateRef([text], k, m)
    assert hard and all(ref.first_is_not_minimum(x) for x in hard)
    query = [text, synth.revcomp(text)] + hard + [synth.revcomp(x) for x in hard]
    for limit in (None, 1):
        with api.TigIndex([text], k, m, bucket_limit=limit, locate=True) as ix:
            _assert_equals_ref(ix, [text], query, k, f"palindrome limit={limit}")


def test_hand_cases(gpu):
    for limit in (None, 1):
        with api.TigIndex(["AAAAAA"], 3, bucket_limit=limit, locate=True) as ix:
            want = _assert_equals_ref(ix, ["AAAAAA"], ["AAAAA"], 3, "a repeat breaks runs")
            assert want["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 0, 0), (0, 2, 1, 0, 0, 0)]
        with api.TigIndex(["A", "C"], 1, bucket_limit=limit, locate=True) as ix:
            want = _assert_equals_ref(ix, ["A", "C"], ["AC"], 1, "k = 1 looks the records up")
            assert want["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 1, 0)]


@pytest.mark.parametrize("k", [5, 31, 40])
def test_a_stretch_planted_twice(gpu, k):
    """The stretch forward in record 3 and reverse-complemented in record 1: it is located in record 1, as -."""
    rng = random.Random(k)
    x = cases.dna(rng, 3 * k)
    recs = [cases.dna(rng, 2 * k) for _ in range(5)]
    recs[1] = recs[1][:k] + synth.revcomp(x) + recs[1][k:]
    recs[3] = recs[3][:k + 2] + x + recs[3][k + 2:]
    for limit in (None, 1):
        with api.TigIndex(recs, k, bucket_limit=limit, locate=True) as ix:
            want = _assert_equals_ref(ix, recs, [x, recs[3]], k, f"planted twice limit={limit}")
        if k > 5:  # (at k = 5 the random flanks hold some of x's k-mers by chance)
            assert want["runs"][0] == (0, 0, 2 * k + 1, 1, 1, k)
            # (inside record 3 the run may reach a window further where the flanks agree by chance)
            assert any(r[0] == 1 and r[3:5] == (1, 1) and r[1] <= k + 2 and r[1] + r[2] >= 3 * k + 3 for r in want["runs"])


@pytest.mark.parametrize("k,m", [(31, None), (32, None), (32, 12)])
def test_repeats_take_the_heavy_path(gpu, k, m):
    """Poly-A and (AC)^n of 5 000 bases beside random sequence at the default limit: the two classes of (AC)^n have thousands of
    occurrences each, and at k >= 32 the slot names whichever won the claim, so only the heavy positions give locations 0 and 1."""
    n = 5000
    index, query = cases.repeats_case(n, k)
    with api.TigIndex(index, k, m, locate=True) as ix, api.TigIndex(index, k, m) as plain:
        assert ix.info.heavy_buckets >= 1 and ix.info.heavy_windows >= 2 * (n - k + 1) - 2 and ix.info.anchors > 0
        assert ix.info.device_bytes == plain.info.device_bytes + 8 * ix.info.table_slots and ix.info.table_slots > 0
        assert {f: v for f, v in ix.info.__dict__.items() if f != "device_bytes"} == {f: v for f, v in plain.info.__dict__.items() if f != "device_bytes"}
        want = _assert_equals_ref(ix, index, query, k, "repeats")
        a, b = ix.query(query, bits=True), plain.query(query, bits=True)
        for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
            assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
        with pytest.raises(ValueError):
            plain.locate(query)
    ac_at = n + n + 200  # the start of (AC)^n in the concatenation: record 3
    by_record = {r[0]: r for r in want["runs"]}
    assert by_record[0] == (0, 0, 1, 0, 1, 0)           # poly-A: the first base of record 1
    assert by_record[1] == (1, 0, 1, 0, 3, 0) and by_record[2] == (2, 0, 1, 0, 3, 1)  # ACAC.. at 0 and CACA.. at 1 of record 3
    assert ac_at == sum(map(len, index[:3]))


def _unique_dna(rng, length, k):
    """DNA in which no canonical k-mer occurs twice and none is a palindrome: every window of a copy has one place to be."""
    while True:
        s, used = cases.dna(rng, k - 1), set()
        while len(s) < length:
            for c in rng.sample("ACGT", 4):
                w = (s + c)[-k:]
                if w != synth.revcomp(w) and synth.canonical(w) not in used:
                    used.add(synth.canonical(w))
                    s += c
                    break
            else:
                break  # a dead end: start over
        if len(s) == length:
            return s


@pytest.mark.parametrize("k,m,limit", [(5, 2, None), (31, None, None), (33, 19, 1)])
def test_run_ends_against_thread_runs(gpu, k, m, limit):
    """A copy of the unique index record, which spans more than three thread stretches, behind 0 .. 69 junk bases, on both strands: one
    run of all its windows wherever its ends fall among the 64 positions a thread owns. Then the record with one substitution at each
    position in turn: two runs, or one at the ends, wherever no mutated window is in the index by chance."""
    rng = random.Random(k)
    L = 3 * 64 + k
    s = _unique_dna(rng, L, k)
    with api.TigIndex([s], k, m, bucket_limit=limit, locate=True) as ix:
        for strand, copy in ((0, s), (1, synth.revcomp(s))):
            query = [x for j in range(70) for x in ("N" * j, cases.flip_case(rng, copy))]
            want = _assert_equals_ref(ix, [s], query, k, f"strand {strand}")
            assert want["runs"] == [(2 * j + 1, 0, L - k + 1, strand, 0, 0) for j in range(70)]
        query = [s[:j] + rng.choice([c for c in "ACGT" if c != s[j]]) + s[j + 1:] for j in range(L)]
        want = _assert_equals_ref(ix, [s], query, k, "substitutions")
    clean = 0
    for j in range(L):
        covering = min(j, L - k) - max(0, j - k + 1) + 1
        if want["found"][j] != L - k + 1 - covering:
            continue  # a mutated window is in the index by chance (small k)
        clean += 1
        left, right = max(0, j - k + 1), L - k - min(j, L - k)
        expected = ([(j, 0, left, 0, 0, 0)] if left else []) + ([(j, j + 1, right, 0, 0, j + 1)] if right else [])
        assert [r for r in want["runs"] if r[0] == j] == expected, (k, j)
    assert clean == L if k > 30 else clean > 10, (k, clean)


def test_awkward_inputs(gpu):
    """tig_index_cases.engineered(): minimizers twice in a window, palindromic m-mers and k-mers, m = k and m = 1, record borders with
    empty records between, record ends, records shorter than k and than m, empty indexes and queries; then seventy one-base records, a
    query without a valid window, junk bytes and flipped case."""
    for name, index, query, k, m, limit in cases.engineered():
        want = LR.locate(index, query, k)
        for lim in (limit, 1):
            with api.TigIndex(index, k, m, bucket_limit=lim, locate=True) as ix:
                _assert_equals_ref(ix, index, query, k, name, want)
    rng = random.Random(70)
    ones = [rng.choice("ACGTacgt") for _ in range(70)]
    for k, index, query in ((1, ones, ones[::-1] + ["".join(ones)]), (1, ["A"] * 70, ["T"] * 70 + ["N", "", "at"]),
                            (2, ones, ones + ["".join(ones)]), (4, ["ACGTACGT", "", "ac", "GGGGG"], ["NNNN", "ACGNACG", "", "---", "acg"]),
                            (31, [cases.dna(rng, 100)], ["N" * 100, cases.JUNK * 3, ""])):
        for limit in (None, 1):
            with api.TigIndex(index, k, bucket_limit=limit, locate=True) as ix:
                _assert_equals_ref(ix, index, query, k, f"awkward k={k} limit={limit}")
    s = cases.dna(rng, 300)
    junk = list(cases.flip_case(rng, s))
    for at in (0, 63, 64, 65, 150, 299):
        junk[at] = rng.choice(cases.JUNK)
    with api.TigIndex([s[:100], "", s[100:]], 21, locate=True) as ix:
        _assert_equals_ref(ix, [s[:100], "", s[100:]], ["".join(junk), synth.revcomp(s).lower(), cases.flip_case(rng, s)], 21, "junk and case")


def test_reuse_and_interference(gpu):
    rng = random.Random(9)
    genome = cases.dna(rng, 3000)
    a = [genome[i:i + 400] for i in range(0, 2700, 300)]  # neighbouring records share 100 bases: their k-mers sit in the earlier one
    b = [synth.revcomp(genome[1000:2500]), cases.dna(rng, 500), "A" * 200]
    queries = [[genome[100:900], cases.dna(rng, 300), "ACGTN" * 50], [synth.revcomp(genome)[:-1] + "N", ""],
               [cases.dna(rng, 70)] * 5 + [genome[2000:2100].lower(), "a" * 100]]
    ka, kb = 21, 45
    ia = api.TigIndex(a, ka, locate=True)
    live = api.device_arena_stats(0)["live_bytes"]
    first = [ia.locate(q) for q in queries]
    assert api.device_arena_stats(0)["live_bytes"] == live  # a call gives back what it took
    for q, r in zip(queries, first):
        _assert_equals_ref(ia, a, q, ka, "first")
    ib = api.TigIndex(b, kb, 15, locate=True)  # a second index, of another k, with a heavy bucket
    assert ib.info.heavy_buckets >= 1 and ia.info.heavy_buckets == 0
    for q, r in zip(queries, first):
        _assert_same_result(ia.locate(q), r)
        _assert_equals_ref(ib, b, q, kb, "second index")
    api.release_device_memory(0)
    for q, r in zip(queries, first):
        _assert_same_result(ia.locate(q), r)
    with api.TigIndex(a, ka) as plain:  # the membership query does not see the difference
        for q in queries:
            x, y = ia.query(q, bits=True), plain.query(q, bits=True)
            for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
                assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), f
        assert plain.info == ia.info and not plain.locating  # (no bucket is heavy: not a byte more)
        with pytest.raises(ValueError) as e:
            plain.locate(queries[0])
        assert "locate=True" in str(e.value)
    t = api.last_tig_locate_times()
    assert set(t) == {"upload_ms", "pack_ms", "probe_ms", "runs_ms"} and all(v >= 0 for v in t.values()) and t["probe_ms"] > 0 and t["runs_ms"] > 0
    ia.close()
    with pytest.raises(ValueError) as e:
        ia.locate(queries[0])
    assert str(e.value) == "the index is closed"
    _assert_equals_ref(ib, b, queries[0], kb, "after the other closed")
    ib.close()


COMP = np.zeros(256, np.uint8)
for _a, _b in zip("ACGTN", "TGCAN"):
    COMP[ord(_a)] = ord(_b)


@pytest.mark.parametrize("extra_records", [0, 50])
def test_size_and_memory(gpu, extra_records):
    """A random genome of 2 * 10^5 bases with 300 reverse-complemented pieces of it as further records -- many workgroups, real buckets,
    every piece's class twice, on opposite strands --, and once more with 50 pieces appended again, so that classes repeat across
    records: the sparse index and the locating table return the same arrays. The memory cap is derived: the sparse index is held to half
    the plain table (test_gpu_tig_index.py), and a locating table is at least twice the plain one (its `where` is a second table)."""
    k, m = 31, 19
    rng = np.random.default_rng(30)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200_000)]
    pieces = [genome]
    for _ in range(300):
        at, n = int(rng.integers(0, 199_000)), int(rng.integers(1, 1000))
        pieces.append(COMP[genome[at:at + n][::-1]])
    pieces += [pieces[1 + 3 * i].copy() if i % 2 else COMP[pieces[1 + 3 * i][::-1]] for i in range(extra_records)]
    seq = np.concatenate(pieces)
    off = np.zeros(len(pieces) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    cuts = np.sort(rng.integers(0, len(seq), 2000))
    q_pieces = [seq[a:b] if rng.random() < 0.5 else COMP[seq[a:b][::-1]] for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(seq)])]
    q_seq = np.concatenate(q_pieces)
    q_off = np.zeros(len(q_pieces) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in q_pieces])
    sub = rng.random(len(q_seq)) < 0.03
    q_seq[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    q_seq[rng.random(len(q_seq)) < 1e-3] = ord("N")
    with api.TigIndex((seq, off), k, m, locate=True) as ix, api.KmerIndex((seq, off), k, locate=True) as table:
        with api.TigIndex((seq, off), k, m) as plain:
            assert ix.info.heavy_buckets == 0 and ix.info.device_bytes == plain.info.device_bytes
        assert ix.info.device_bytes <= table.info.device_bytes // 4
        got, want = ix.locate((q_seq, q_off)), table.locate((q_seq, q_off))
        _assert_same_result(got, want)
        _assert_same_result(ix.locate((q_seq, q_off)), got)
    runs = got.runs
    assert len(runs) > 2000 and set(runs["strand"].tolist()) == {0, 1} and int(runs["kmers"].max()) > 30
    assert int(runs["kmers"].sum()) == int(got.found.sum()) and 50_000 < int(got.found.sum()) < int(got.valid.sum())
    assert int(runs["t_record"].min()) == 0  # a piece's k-mers lie in the genome, where they occur first


def _fasta_records(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def test_through_the_product(gpu, tmp_path):
    """Two haplotypes of 10 kb compacted, both tig sets written. Over the input the sparse index's rows are byte for byte the table's
    --query-locate-out; over the tigs they are the restatement's over the tig file as written; --query-out never changes."""
    k = 21
    rng = random.Random(30)
    haps = synth.random_genome(10_000, seed=30, haplotypes=2)
    query = []
    for i in range(24):
        h = rng.choice(haps)
        at = rng.randrange(0, len(h) - 400)
        s = h[at:at + rng.randint(30, 400)]
        s = list(synth.revcomp(s) if rng.random() < 0.5 else s)
        for j in range(len(s)):
            if rng.random() < 0.01:
                s[j] = rng.choice("ACGTNn")
        query.append("".join(s))
    query += ["ACGT", cases.dna(rng, 100)]
    h_fa, q_fa = tmp_path / "haps.fa", tmp_path / "q.fa"
    h_fa.write_text("".join(f">h{i}\n{s}\n" for i, s in enumerate(haps)))
    q_fa.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(query)))

    def run(tag, *extra):
        out = {x: tmp_path / f"{tag}.{x}" for x in ("tsv", "g.fa", "e.fa", "u.fa")}
        r = subprocess.run([sys.executable, "-m", "matchtigs_amd", "--seq-in", str(h_fa), "-k", str(k), "--unitigs-fa-out", str(out["u.fa"]),
                            "--greedytigs-fa-out", str(out["g.fa"]), "--eulertigs-fa-out", str(out["e.fa"]), "--query-fa", str(q_fa),
                            "--query-out", str(out["tsv"]), *extra], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        return out

    def rows_of(index_seqs):
        want = LR.locate(index_seqs, query, k)
        head = "record\tqstart\tqend\tstrand\ttarget\ttstart\ttend\tkmers\n"
        return head + "".join(f"q{q}\t{qs}\t{qs + n + k - 1}\t{'-' if s else '+'}\t{t}\t{ts}\t{ts + n + k - 1}\t{n}\n" for q, qs, n, s, t, ts in want["runs"])

    table = run("table", "--query-locate-out", str(tmp_path / "table.loc"))
    bare = run("bare", "--query-index", "minimizer")
    assert bare["tsv"].read_bytes() == table["tsv"].read_bytes()
    sparse = run("sparse", "--query-index", "minimizer", "--query-index-locate-out", str(tmp_path / "sparse.loc"))
    assert (tmp_path / "sparse.loc").read_bytes() == (tmp_path / "table.loc").read_bytes()
    assert (tmp_path / "sparse.loc").read_text() == rows_of(_fasta_records(sparse["u.fa"]))
    assert sparse["tsv"].read_bytes() == table["tsv"].read_bytes()
    assert (tmp_path / "sparse.loc").read_text().count("\n") > 24
    for over, fa, loc in (("greedytigs", "g.fa", "g.loc.gz"), ("eulertigs", "e.fa", "e.loc")):
        out = run(over, "--query-index", "minimizer", "--query-index-over", over, "--query-index-locate-out", str(tmp_path / loc))
        raw = (tmp_path / loc).read_bytes()
        text = (gzip.decompress(raw) if loc.endswith(".gz") else raw).decode()
        assert text == rows_of(_fasta_records(out[fa])), over
        assert out["tsv"].read_bytes() == table["tsv"].read_bytes(), over
