"""Locating k-mers on the GPU (KmerIndex(locate=True).locate, kmer_query_device.hip) against the restatement
(kmer_locate_ref.py): every run, and kmers / valid / found, as exact integers. Random index / query pairs over many k (both strands,
repeats, palindromes), a copy of the index record behind 0 .. 69 junk bases (run ends against the threads' runs of 64 positions), a
substitution at every position, a repeat shared by two index records, thousands of tiny records at k = 1 and 2 (the same-record
rule), empty inputs, determinism, one case large enough for many workgroups, and the path through the product
(`--query-locate-out`)."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_locate_ref as R
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 3, 4, 5, 16, 31, 32, 33, 64, 65, 101]
JUNK = "NNNNnnRYKMSWBDHVxX-*. \x00\x7f5"  # what a query may hold besides ACGT


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the k-mer index has no CPU path")
    return torch


def _dna(rng, n, weights=(1, 1, 1, 1)):
    return "".join(rng.choices("ACGT", weights, k=n))


def _flip_case(rng, s):
    return "".join(c.lower() if rng.random() < 0.3 else c for c in s)


def _runs(result):
    return [tuple(int(x) for x in row) for row in result.runs[list(R.FIELDS)].tolist()]


def _assert_equals_ref(index, index_seqs, query, k, what=""):
    """One locate call: the runs and the three counts equal the restatement's. Returns the restatement's result."""
    want = R.locate(index_seqs, query, k)
    got = index.locate(query)
    assert got.runs.dtype == api.KMER_RUN_DTYPE
    for f in ("kmers", "valid", "found"):
        g = getattr(got, f)
        assert g.dtype == np.uint64 and g.tolist() == want[f], (what, k, f, g.tolist()[:20], want[f][:20])
    assert _runs(got) == want["runs"], (what, k, _runs(got)[:8], want["runs"][:8])
    return want


def _random_pair(rng, k):
    """The membership tests' generator: an index cut from one short genome and its reverse complement (k-mers repeat in both
    orientations, a palindrome planted for even k, a biased alphabet, mixed case, lengths 0 .. 3 k) and a query of copies, pieces,
    foreign records and mixtures, with junk bytes thrown in."""
    weights = rng.choice([(1, 1, 1, 1), (6, 1, 1, 2), (5, 0, 0, 5), (0, 4, 4, 0)])
    anti = tuple(int(w == 0) for w in weights) if 0 in weights else (1, 1, 1, 1)
    half = _dna(rng, k // 2, weights)
    genome = _dna(rng, 2 * k + 2, weights) + (half + synth.revcomp(half) if k % 2 == 0 else "") + _dna(rng, 2 * k + 2, weights)
    sources = (genome, synth.revcomp(genome))

    def piece(n):
        g = sources[rng.random() < 0.5]
        at = rng.randint(0, len(g) - n)
        return g[at:at + n]

    index = [_flip_case(rng, piece(rng.randint(0, 3 * k)) if rng.random() < 0.85 else _dna(rng, rng.randint(0, 3 * k), weights))
             for _ in range(rng.randint(0, 8))]
    query = []
    for _ in range(rng.randint(0, 8)):
        n = rng.randint(0, 3 * k)
        x = rng.random()
        if x < 0.3 and index:
            s = rng.choice(index)
            s = synth.revcomp(s.upper()) if rng.random() < 0.5 else s
        elif x < 0.55:
            s = piece(n)
        elif x < 0.75:
            s = _dna(rng, n, anti)
        else:
            s = piece(n // 2) + _dna(rng, n - n // 2, anti)
        s = list(_flip_case(rng, s))
        if s and rng.random() < 0.4:
            for _ in range(rng.randint(1, 3)):
                s[rng.randrange(len(s))] = rng.choice(JUNK)
        query.append("".join(s))
    return index, query


@pytest.mark.parametrize("k", KS)
def test_random_pairs(gpu, k):
    rng = random.Random(7000 + k)
    seen = dict.fromkeys(("plus", "minus", "long", "repeated_class", "palindrome_hit"), False)
    for i in range(100):
        index, query = _random_pair(rng, k)
        with api.KmerIndex(index, k, locate=True) as ix:
            assert ix.locating
            want = _assert_equals_ref(ix, index, query, k, f"pair {i}")
        occurrences = sum(max(0, len(s) - k + 1) for s in index)
        seen["repeated_class"] |= bool(want["runs"]) and occurrences > len(R.first_positions(index, k)[0])
        for qr, qs, n, strand, _, _ in want["runs"]:
            seen["minus" if strand else "plus"] = True
            seen["long"] |= n > 1
            for j in range(qs, qs + n):
                w = query[qr][j:j + k].upper()
                seen["palindrome_hit"] |= w == synth.revcomp(w)
    # the generator really produces what the cases are for
    assert seen.pop("palindrome_hit") == (k % 2 == 0), k
    assert all(seen.values()), (k, seen)


def _unique_dna(rng, length, k):
    """DNA in which no canonical k-mer occurs twice and none is a palindrome: every window of a copy has one place to be."""
    while True:
        s, used = _dna(rng, k - 1), set()
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


@pytest.mark.parametrize("k", [5, 31, 33])
def test_run_ends_against_thread_runs(gpu, k):
    """A copy of the index record, which spans more than three thread runs, behind 0 .. 69 junk bases: one run of all its windows
    wherever it starts and ends among the 64 positions a thread owns; then the same for its reverse complement."""
    rng = random.Random(k)
    L = 3 * 64 + k + 7
    s = _unique_dna(rng, L, k)
    with api.KmerIndex([s], k, locate=True) as ix:
        for strand, copy in ((0, s), (1, synth.revcomp(s))):
            query = [x for j in range(70) for x in ("N" * j, _flip_case(rng, copy))]
            want = _assert_equals_ref(ix, [s], query, k, f"strand {strand}")
            assert want["runs"] == [(2 * j + 1, 0, L - k + 1, strand, 0, 0) for j in range(70)]


@pytest.mark.parametrize("k", [5, 33])
def test_substitution_at_every_position(gpu, k):
    """The index record with position j substituted, one copy per j, all in one call: wherever none of the windows that cover j
    is in the index by chance, the copy is exactly two runs, or one at the ends."""
    rng = random.Random(50 + k)
    L = 3 * 64 + k + 7
    s = _unique_dna(rng, L, k)
    query = [s[:j] + rng.choice([c for c in "ACGT" if c != s[j]]) + s[j + 1:] for j in range(L)]
    with api.KmerIndex([s], k, locate=True) as ix:
        want = _assert_equals_ref(ix, [s], query, k)
    clean = 0
    for j in range(L):
        covering = min(j, L - k) - max(0, j - k + 1) + 1
        if want["found"][j] != L - k + 1 - covering:
            continue  # a mutated window is in the index by chance (small k)
        clean += 1
        left, right = max(0, j - k + 1), L - k - min(j, L - k)  # windows before and behind the covering ones
        expected = ([(j, 0, left, 0, 0, 0)] if left else []) + ([(j, j + 1, right, 0, 0, j + 1)] if right else [])
        assert [r for r in want["runs"] if r[0] == j] == expected, (k, j)
    assert clean == L if k == 33 else clean > 10, (k, clean)  # (at k = 5 the index holds 200 of the 512 classes)


@pytest.mark.parametrize("k", [4, 31, 40])
def test_repeat_shared_by_two_records(gpu, k):
    """Index [X + R + Y, Z + R + W]: the windows inside R are placed in record 0, where they occur first, so a copy of record 1 is
    three runs, the middle one in record 0."""
    rng = random.Random(k)
    n = k + 2  # the flanks
    while True:  # the k-mers of both records differ from each other, apart from those inside R, and none is a palindrome
        u = _unique_dna(rng, 5 * n + 5, k)
        X, Rp, Y, Z, W = u[:n], u[n:2 * n + 5], u[2 * n + 5:3 * n + 5], u[3 * n + 5:4 * n + 5], u[4 * n + 5:]
        index = [X + Rp + Y, Z + Rp + W]
        first, _ = R.first_positions(index, k)
        windows = [w for s in index for w in (s[i:i + k] for i in range(len(s) - k + 1))]
        if len(first) == len(windows) - (len(Rp) - k + 1) and all(w != synth.revcomp(w) for w in windows):
            break
    assert len(Rp) >= k + 5
    inner, outer = len(Rp) - k + 1, n  # windows inside R; windows that start in Z (or end in W)
    with api.KmerIndex(index, k, locate=True) as ix:
        want = _assert_equals_ref(ix, index, [index[1], synth.revcomp(index[1])], k)
    assert want["runs"] == [(0, 0, outer, 0, 1, 0), (0, outer, inner, 0, 0, len(X)), (0, outer + inner, outer, 0, 1, outer + inner),
                            (1, 0, outer, 1, 1, outer + inner), (1, outer, inner, 1, 0, len(X)), (1, outer + inner, outer, 1, 1, 0)]


@pytest.mark.parametrize("k", [1, 2])
def test_many_tiny_records(gpu, k):
    """300 index records and 5 000 query records of length 0 .. 3: neighbouring windows in different records on either side."""
    rng = random.Random(k)
    index = [_dna(rng, rng.randint(0, 3)) for _ in range(300)]
    query = ["".join(rng.choice("ACGTacgtN") for _ in range(rng.randint(0, 3))) for _ in range(5000)]
    with api.KmerIndex(index, k, locate=True) as ix:
        want = _assert_equals_ref(ix, index, query, k)
    assert {r[3] for r in want["runs"]} == {0, 1} and len({r[4] for r in want["runs"]}) > 1 and 0 < sum(want["found"]) < sum(want["kmers"])
    if k == 2:
        assert max(r[2] for r in want["runs"]) > 1
    if k == 1:
        # this index puts the rule to work on its own side: its two classes are first met at the neighbouring positions 0 and 1, which
        # lie in two records, so no run has two windows although thousands of query records hold both classes side by side
        assert sorted(R.first_positions(index, 1)[0].values()) == [0, 1] and len(index[0]) == 1
        assert max(r[2] for r in want["runs"]) == 1 and any(sum(1 for r in want["runs"] if r[0] == i) > 1 for i in range(50))
        # the case of the contract, and windows next to each other in the query but in two records
        with api.KmerIndex(["A", "C"], 1, locate=True) as ix:
            assert _runs(ix.locate(["AC"])) == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 1, 0)]
        with api.KmerIndex(["AC"], 1, locate=True) as ix:
            assert _runs(ix.locate(["A", "", "C", "AC"])) == [(0, 0, 1, 0, 0, 0), (2, 0, 1, 0, 0, 1), (3, 0, 2, 0, 0, 0)]


@pytest.mark.parametrize("k", [1, 4, 31, 32, 40])
def test_empties(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3), "N" + _dna(rng, k), ""]
    short = [_dna(rng, n) for n in (k - 1, 0, k // 2)]
    for index in ([], short, [""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        with api.KmerIndex(index, k, locate=True) as ix:
            assert ix.locating and ix.info.distinct == ix.info.occurrences == 0
            r = ix.locate(full)
            assert len(r.runs) == 0 and r.runs.dtype == api.KMER_RUN_DTYPE
            assert r.found.tolist() == [0, 0, 0] and r.valid.tolist() == [k + 4, 1, 0] and r.kmers.tolist() == [k + 4, 2, 0]
    with api.KmerIndex(full[:1], k, locate=True) as ix, api.KmerIndex(full[:1], k) as plain:
        for q in ([], [""], ["", ""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
            r = ix.locate(q)
            assert len(r.runs) == 0 and len(r.kmers) == len(r.valid) == len(r.found) == (len(q) if isinstance(q, list) else 0)
        assert not plain.locating
        with pytest.raises(ValueError):
            plain.locate(full)
        assert plain.info.device_bytes < ix.info.device_bytes
        assert {f: v for f, v in vars(plain.info).items() if f != "device_bytes"} == {f: v for f, v in vars(ix.info).items() if f != "device_bytes"}
        # query on a locating index = query on a plain one; locate's counts = query's
        q = short + full + [synth.revcomp(full[0]).lower()]
        a, b, c = plain.query(q, bits=True), ix.query(q, bits=True), ix.locate(q)
        for f in ("kmers", "valid", "found", "valid_bits", "present_bits", "offsets"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        for f in ("kmers", "valid", "found", "offsets"):
            assert np.array_equal(getattr(a, f), getattr(c, f)), f
        _assert_equals_ref(ix, full[:1], q, k)
    ix.close()
    with pytest.raises(ValueError):
        ix.locate(full)


LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    LUT[ord(_c)] = LUT[ord(_c.lower())] = _i
COMP = np.zeros(256, np.uint8)
for _a, _b in zip("ACGTN", "TGCAN"):
    COMP[ord(_a)] = ord(_b)


def _mutated_query(ua_seq, ua_off, seed):
    """The unitigs cut at random, half of the pieces reverse-complemented, 2 % substitutions, an N every ~10^3 bases: twice over."""
    rng = np.random.default_rng(seed)
    o = ua_off.astype(np.int64)
    pieces = []
    for _ in range(2):
        for u in range(len(o) - 1):
            at, end = int(o[u]), int(o[u + 1])
            while at < end:
                n = int(rng.integers(1, 400))
                p = ua_seq[at:min(end, at + n)]
                pieces.append(COMP[p[::-1]] if rng.random() < 0.5 else p)
                at += n
    seq = np.concatenate(pieces)
    off = np.zeros(len(pieces) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    sub = rng.random(len(seq)) < 0.02
    seq[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    seq[rng.random(len(seq)) < 1e-3] = ord("N")
    return seq, off


def _window_table(seq, off, k):
    """Per global position of a set: the window's forward and canonical code, its record, and whether a window starts there."""
    b = LUT[seq]
    bad = b > 3
    fwd, rc = synth._kmer_codes(np.where(bad, 0, b), k)
    n = len(fwd)
    o = off.astype(np.int64)
    lens = np.diff(o)
    rec = np.repeat(np.arange(len(lens)), lens)[:n]
    inside = np.arange(n) + k <= o[1:][rec]
    cb = np.concatenate([[0], np.cumsum(bad)])
    return fwd, np.minimum(fwd, rc), rec, inside & (cb[k:k + n] - cb[:n] == 0), o, lens


def _numpy_locate(t_seq, t_off, q_seq, q_off, k):
    """The restatement for k <= 31 by numpy: np.unique's first index is the smallest position of a class."""
    t_fwd, t_canon, _, t_ok, t_o, _ = _window_table(t_seq, t_off, k)
    t_pos = np.flatnonzero(t_ok)
    codes, first = np.unique(t_canon[t_pos], return_index=True)
    first = t_pos[first]
    q_fwd, q_canon, q_rec, q_ok, q_o, q_lens = _window_table(q_seq, q_off, k)
    at = np.minimum(np.searchsorted(codes, q_canon), len(codes) - 1)
    found = q_ok & (codes[at] == q_canon)
    t = np.where(found, first[at], -1)
    strand = np.where(found, q_fwd != t_fwd[np.maximum(t, 0)], False)
    t_rec = np.searchsorted(t_o, t, side="right") - 1
    cont = np.zeros(len(t), bool)
    step = np.where(strand[1:], -1, 1)
    cont[1:] = (found[1:] & found[:-1] & (strand[1:] == strand[:-1]) & (t[1:] == t[:-1] + step) & (q_rec[1:] == q_rec[:-1])
                & (t_rec[1:] == t_rec[:-1]))
    start = np.flatnonzero(found & ~cont)
    run_of = np.cumsum(found & ~cont) - 1
    kmers = np.bincount(run_of[found], minlength=len(start))
    runs = np.zeros(len(start), api.KMER_RUN_DTYPE)
    runs["q_record"], runs["q_start"], runs["kmers"], runs["strand"] = q_rec[start], start - q_o[q_rec[start]], kmers, strand[start]
    leftmost = np.where(strand[start], t[start] - (kmers - 1), t[start])
    runs["t_record"], runs["t_start"] = t_rec[start], leftmost - t_o[t_rec[start]]
    counts = {"kmers": np.maximum(q_lens - k + 1, 0), "valid": np.bincount(q_rec[q_ok], minlength=len(q_lens)),
              "found": np.bincount(q_rec[found], minlength=len(q_lens))}
    return runs, counts


def _assert_runs_spell(runs, t_seq, t_off, q_seq, q_off, k, unique_index):
    """Independent of any restatement: every run spells as the contract says; and, where every k-mer of the index occurs once and
    none is a palindrome, no run can be extended by a base on either side."""
    t_o, q_o = t_off.astype(np.int64), q_off.astype(np.int64)
    upper = np.arange(256, dtype=np.uint8)
    upper[ord("a"):ord("z") + 1] -= 32
    tu, qu = upper[t_seq], upper[q_seq]
    span = runs["kmers"].astype(np.int64) + k - 1
    qs = q_o[runs["q_record"].astype(np.int64)] + runs["q_start"].astype(np.int64)
    ts = t_o[runs["t_record"].astype(np.int64)] + runs["t_start"].astype(np.int64)
    assert (qs + span <= q_o[runs["q_record"].astype(np.int64) + 1]).all() and (ts + span <= t_o[runs["t_record"].astype(np.int64) + 1]).all()
    for a, b, n, s in zip(qs.tolist(), ts.tolist(), span.tolist(), runs["strand"].tolist()):
        tw = tu[b:b + n]
        assert np.array_equal(qu[a:a + n], COMP[tw[::-1]] if s else tw), (a, b, n, s)
    if not unique_index:
        return
    minus = runs["strand"] == 1
    q_lo, q_hi = q_o[runs["q_record"].astype(np.int64)], q_o[runs["q_record"].astype(np.int64) + 1]
    t_lo, t_hi = t_o[runs["t_record"].astype(np.int64)], t_o[runs["t_record"].astype(np.int64) + 1]
    pad_q, pad_t = np.concatenate([qu, [0]]), np.concatenate([tu, [1]])  # (a base beyond either end equals nothing)
    before_q, behind_q = np.where(qs > q_lo, pad_q[qs - 1], 0), np.where(qs + span < q_hi, pad_q[np.minimum(qs + span, len(qu))], 0)
    before_t, behind_t = np.where(ts > t_lo, pad_t[ts - 1], 1), np.where(ts + span < t_hi, pad_t[np.minimum(ts + span, len(tu))], 1)
    left_partner = np.where(minus, COMP[behind_t], before_t)   # the index base a query base before the run would have to equal
    right_partner = np.where(minus, COMP[before_t], behind_t)
    acgt = np.isin(before_q, np.frombuffer(b"ACGT", np.uint8)), np.isin(behind_q, np.frombuffer(b"ACGT", np.uint8))
    assert not (acgt[0] & (before_q == left_partner)).any() and not (acgt[1] & (behind_q == right_partner)).any()


@pytest.fixture(scope="module")
def gseq_unitigs():
    return synth.g_seq_arrays(200_000, seed=5, k=31)


@pytest.fixture(scope="module")
def gseq_query(gseq_unitigs):
    return _mutated_query(gseq_unitigs.seq, gseq_unitigs.off, 1)


def _assert_same_result(a, b):
    for f in ("kmers", "valid", "found", "offsets", "runs"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_larger_case_k31(gpu, gseq_unitigs, gseq_query):
    """~10^6 index bases, ~2 * 10^6 query bases: grids of many workgroups, real probe chains, ~10^5 runs. Two builds and two calls
    give the same arrays, also after the arena gave its free chunks back."""
    ua, k = gseq_unitigs, 31
    seq, off = gseq_query
    want, counts = _numpy_locate(ua.seq, ua.off, seq, off, k)
    with api.KmerIndex((ua.seq, ua.off), k, locate=True) as ix:
        got = ix.locate((seq, off))
        again = ix.locate((seq, off))
        plain = ix.query((seq, off))
        api.release_device_memory(0)
        with api.KmerIndex((ua.seq, ua.off), k, locate=True) as twin:
            assert twin.info == ix.info
            other = twin.locate((seq, off))
        third = ix.locate((seq, off))
    assert np.array_equal(got.runs, want)
    for f, w in counts.items():
        assert np.array_equal(getattr(got, f), w.astype(np.uint64)) and np.array_equal(getattr(plain, f), getattr(got, f)), f
    for x in (again, other, third):
        _assert_same_result(got, x)
    assert int(got.runs["kmers"].sum()) == int(got.found.sum()) > 100_000 and len(seq) > 1_900_000
    assert 10_000 < len(got.runs) and {0, 1} == set(got.runs["strand"].tolist()) and int(got.runs["kmers"].max()) > 100
    _assert_runs_spell(got.runs, ua.seq, ua.off, seq, off, k, unique_index=True)
    t = api.last_kmer_locate_times()
    assert set(t) == {"upload_ms", "pack_ms", "probe_ms", "runs_ms"} and all(v >= 0 for v in t.values()) and t["probe_ms"] > 0 and t["runs_ms"] > 0


def test_larger_case_k31_repeated_classes(gpu, gseq_unitigs, gseq_query):
    """The same with every third unitig indexed a second time, reverse-complemented, behind the others: ~10^5 classes whose
    occurrences race for the smallest position."""
    ua, k = gseq_unitigs, 31
    seq, off = gseq_query
    o = ua.off.astype(np.int64)
    extra = [COMP[ua.seq[o[u]:o[u + 1]][::-1]] for u in range(0, len(o) - 1, 3)]
    t_seq = np.concatenate([ua.seq] + extra)
    t_off = np.concatenate([ua.off, ua.off[-1] + np.cumsum([len(x) for x in extra]).astype(np.uint64)])
    want, counts = _numpy_locate(t_seq, t_off, seq, off, k)
    with api.KmerIndex((t_seq, t_off), k, locate=True) as ix:
        assert ix.info.distinct == len(ua.kmers) < ix.info.occurrences
        got = ix.locate((seq, off))
    assert np.array_equal(got.runs, want) and np.array_equal(got.found, counts["found"].astype(np.uint64))
    assert int(got.runs["t_record"].max()) < len(o) - 1  # nothing is placed in a second copy
    _assert_runs_spell(got.runs, t_seq, t_off, seq, off, k, unique_index=False)


def test_larger_case_k41(gpu, gseq_unitigs):
    """A tenth of that with the wide table form, against the Python restatement."""
    ua, k = gseq_unitigs, 41
    o = ua.off.astype(np.int64)
    n_rec = int(np.searchsorted(o, 100_000))
    sub_seq, sub_off = ua.seq[:o[n_rec]], ua.off[:n_rec + 1]
    seq, off = _mutated_query(sub_seq, sub_off, 2)
    text, qo = seq.tobytes().decode(), off.astype(np.int64)
    index = [sub_seq[o[i]:o[i + 1]].tobytes().decode() for i in range(n_rec)]
    query = [text[qo[i]:qo[i + 1]] for i in range(len(qo) - 1)]
    want = R.locate(index, query, k)
    with api.KmerIndex(index, k, locate=True) as ix:
        got = ix.locate((seq, off))
    for f in ("kmers", "valid", "found"):
        assert getattr(got, f).tolist() == want[f], f
    assert _runs(got) == want["runs"]
    assert int(got.runs["kmers"].sum()) == int(got.found.sum()) > 10_000 and {0, 1} == set(got.runs["strand"].tolist())
    unique = len(R.first_positions(index, k)[0]) == sum(max(0, len(s) - k + 1) for s in index)
    _assert_runs_spell(got.runs, sub_seq, sub_off, seq, off, k, unique_index=unique)


def test_through_the_product(gpu, tmp_path):
    k = 15
    g = synth.g_seq(3000, seed=11, k=k)
    units = g.unitigs
    u_fa, t_fa = tmp_path / "u.fa", tmp_path / "t.fa"
    u_fa.write_text("".join(f">u{i} LN:i:{len(s)}\n{s}\n" for i, s in enumerate(units)))

    def run(*a):
        return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)

    r = run("--fa-in", str(u_fa), "-k", str(k), "--eulertigs-fa-out", str(t_fa))
    assert r.returncode == 0, r.stderr[-2000:]
    tigs = [l for l in t_fa.read_text().splitlines() if not l.startswith(">")]
    tsv, loc, tsv_plain, loc_gz = tmp_path / "r.tsv", tmp_path / "l.tsv", tmp_path / "r0.tsv", tmp_path / "l.tsv.gz"
    r = run("--fa-in", str(t_fa), "-k", str(k), "--query-fa", str(u_fa), "--query-out", str(tsv), "--query-locate-out", str(loc))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split("\t") for l in loc.read_text().splitlines()]
    assert rows[0] == ["record", "qstart", "qend", "strand", "target", "tstart", "tend", "kmers"]
    # eulertigs spell every k-mer once: a unitig lies in one piece in one tig
    assert len(rows) == 1 + len(units)
    strands = set()
    for i, s in enumerate(units):
        name, qs, qe, strand, target, ts, te, n = rows[1 + i]
        assert [name, qs, qe, n] == [f"u{i}", "0", str(len(s)), str(len(s) - k + 1)] and strand in "+-" and int(te) - int(ts) == len(s)
        piece = tigs[int(target)][int(ts):int(te)]
        assert s == (piece if strand == "+" else synth.revcomp(piece)), i
        strands.add(strand)
    assert strands == {"+", "-"}
    r = run("--fa-in", str(t_fa), "-k", str(k), "--query-fa", str(u_fa), "--query-out", str(tsv_plain))
    assert r.returncode == 0, r.stderr[-2000:]
    assert tsv.read_bytes() == tsv_plain.read_bytes() and len(tsv.read_text().splitlines()) == 1 + len(units)
    r = run("--fa-in", str(t_fa), "-k", str(k), "--query-fa", str(u_fa), "--query-out", str(tsv), "--query-locate-out", str(loc_gz))
    assert r.returncode == 0, r.stderr[-2000:]
    assert gzip.decompress(loc_gz.read_bytes()) == loc.read_bytes()
