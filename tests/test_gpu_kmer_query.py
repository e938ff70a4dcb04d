"""The k-mer index on the GPU (kmer_query_device.hip) against its restatement (kmer_query_ref.py): kmers / valid / found
of every record and both bit arrays, as exact integers. Random index / query pairs over many k (both table forms, palindromes,
repeats in either orientation, `N` and other bytes anywhere), an `N` moved over every position of a record that spans several
thread runs, `N` spacings around k, thousands of tiny records per run, empty inputs, reuse of one index, one case large enough for
many workgroups and real probe chains, and the path through the product (`--query-fa`)."""
import gzip
import itertools
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_query_ref as R
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 3, 4, 5, 16, 31, 32, 33, 34, 63, 64, 65, 101]
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


def _assert_equals_ref(index, index_set, seqs, k, what=""):
    """One query with the bit arrays and one without: every output equals the restatement. Returns the restatement's result."""
    want = R.query(index_set, seqs, k)
    got = index.query(seqs, bits=True)
    for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
        g = getattr(got, f)
        assert g.dtype == np.uint64 and g.tolist() == want[f], (what, k, f, g.tolist()[:20], want[f][:20])
    assert got.offsets.tolist() == list(itertools.accumulate((len(s) for s in seqs), initial=0))
    for i in range(min(len(seqs), 12)):
        assert got.presence(i) == R.presence(want, seqs, i), (what, k, i)
    plain = index.query(seqs)
    assert plain.valid_bits is None and plain.present_bits is None
    for f in ("kmers", "valid", "found"):
        assert getattr(plain, f).tolist() == want[f], (what, k, f)
    return want


def _random_pair(rng, k):
    """An index cut from one short genome and its reverse complement (k-mers repeat in both orientations, a palindrome planted for
    even k, a biased alphabet, mixed case, lengths 0 .. 3 k) and a query of copies, pieces, foreign records (drawn from the letters the
    genome avoids where it avoids some) and mixtures, with junk bytes thrown in."""
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
    filled = [i for i, s in enumerate(query) if s]
    if filled and rng.random() < 0.3:
        query[filled[0]] = rng.choice(JUNK) + query[filled[0]][1:]
    if filled and rng.random() < 0.3:
        query[filled[-1]] = query[filled[-1]][:-1] + rng.choice(JUNK)
    return index, query


@pytest.mark.parametrize("k", KS)
def test_random_pairs(gpu, k):
    rng = random.Random(4000 + k)
    seen = dict.fromkeys(("all", "some", "none", "invalid", "first_bad", "last_bad", "palindrome"), False)
    for i in range(120):
        index, query = _random_pair(rng, k)
        iset = R.index_set(index, k)
        with api.KmerIndex(index, k) as ix:
            assert ix.info.distinct == len(iset) and ix.info.records == len(index) and ix.info.k == k
            assert ix.info.occurrences == sum(max(0, len(s) - k + 1) for s in index) and ix.info.characters == sum(map(len, index))
            want = _assert_equals_ref(ix, iset, query, k, f"pair {i}")
        for n, v, f in zip(want["kmers"], want["valid"], want["found"]):
            seen["all"] |= n > 0 and f == n
            seen["some"] |= 0 < f < n
            seen["none"] |= v > 0 and f == 0
            seen["invalid"] |= v < n
        text = "".join(query)
        seen["first_bad"] |= bool(text) and text[0] not in R.ACGT
        seen["last_bad"] |= bool(text) and text[-1] not in R.ACGT
        seen["palindrome"] |= any(x == synth.revcomp(x) for x in iset)
    # the generator really produces what the cases are for
    assert seen.pop("palindrome") == (k % 2 == 0), k
    assert all(seen.values()), (k, seen)


@pytest.mark.parametrize("k", [5, 31, 33])
def test_n_at_every_position(gpu, k):
    """A record of the index that spans more than three thread runs, one copy per position with that position replaced by N, all
    copies in one call: the N costs exactly the windows that cover it, whichever run boundary it sits at."""
    rng = random.Random(k)
    L = 3 * 64 + k + 7
    s = _dna(rng, L)
    query = [s[:j] + "N" + s[j + 1:] for j in range(L)]
    with api.KmerIndex([s], k) as ix:
        got = ix.query(query, bits=True)
        want = R.query(R.index_set([s], k), query, k)
    covering = [min(j, L - k) - max(0, j - k + 1) + 1 for j in range(L)]
    assert got.kmers.tolist() == [L - k + 1] * L
    assert got.valid.tolist() == [L - k + 1 - c for c in covering]
    assert got.found.tolist() == got.valid.tolist()
    for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
        assert getattr(got, f).tolist() == want[f], (k, f)
    j = 64 + 3
    assert got.presence(j) == "1" * max(0, j - k + 1) + "-" * covering[j] + "1" * (L - k - min(j, L - k))


@pytest.mark.parametrize("k", [1, 2, 5, 31, 32, 33, 65])
def test_n_spacing(gpu, k):
    """Two N exactly k + 1, k and k - 1 apart leave 1, 0 and 0 valid windows between them; runs of N longer than a thread's run and
    longer than k; records of nothing but N."""
    rng = random.Random(100 + k)
    flank = k + 70
    src = _dna(rng, 4 * flank + 4 * k)
    query, between = [], []
    for d in (k + 1, k, k - 1):
        if d < 1:
            continue
        query.append(src[:flank] + "N" + src[flank + 1:flank + d] + "n" + src[flank + d + 1:2 * flank + d])
        between.append((len(query) - 1, d))
    run = max(64, k) + 7
    query += [src[:k + 5] + "N" * run + src[k + 5 + run:2 * k + 10 + run], "N" * (2 * k + 70), "N" * (k - 1), "N", src[:k] + "N", "N" + src[:k]]
    iset = R.index_set([src], k)
    with api.KmerIndex([src], k) as ix:
        want = _assert_equals_ref(ix, iset, query, k)
        got = ix.query(query, bits=True)
    for i, d in between:
        lo = int(got.offsets[i]) + flank
        inside = sum((int(got.valid_bits[p >> 6]) >> (p & 63)) & 1 for p in range(lo + 1, lo + d))
        assert inside == (1 if d == k + 1 else 0), (k, d)
        assert want["found"][i] == want["valid"][i] == 2 * flank + d - k + 1 - (d + k) + inside
    n = len(query)
    assert want["valid"][n - 6] == want["found"][n - 6] == 2 * 6
    assert want["valid"][n - 5:n - 2] == [0, 0, 0] and want["kmers"][n - 5] == k + 71 and want["kmers"][n - 4] == 0
    assert want["valid"][n - 2:] == want["found"][n - 2:] == [1, 1]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_many_tiny_records(gpu, k):
    """5 000 records of length 0 .. 3: a thread's run holds dozens of records, empty ones included; the total is no multiple of 64,
    so the last word of both bit arrays has padding, which stays clear. The index is drawn from A and T alone: at k = 1 there are only
    two classes, A/T and C/G, and an index that held both would find every valid window."""
    rng = random.Random(k)
    index = [_dna(rng, rng.randint(0, 3), (3, 0, 0, 1)) for _ in range(300)]
    query = ["".join(rng.choice("ACGTacgtN") for _ in range(rng.randint(0, 3))) for _ in range(5000)]
    if sum(map(len, query)) % 64 == 0:
        query.append("A")
    total = sum(map(len, query))
    with api.KmerIndex(index, k) as ix:
        want = _assert_equals_ref(ix, R.index_set(index, k), query, k)
        got = ix.query(query, bits=True)
    assert total % 64 and len(got.valid_bits) == len(got.present_bits) == total // 64 + 1
    assert int(got.valid_bits[-1]) >> (total % 64) == 0 and int(got.present_bits[-1]) >> (total % 64) == 0
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])


@pytest.mark.parametrize("k", [1, 4, 31, 32, 40])
def test_empties(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3), "N" + _dna(rng, k), ""]
    short = [_dna(rng, n) for n in (k - 1, 0, k // 2)]
    for index in ([], short, [""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
        with api.KmerIndex(index, k) as ix:
            assert ix.info.distinct == ix.info.occurrences == 0 and ix.info.slots >= 8
            want = _assert_equals_ref(ix, set(), full, k)
            assert want["found"] == [0, 0, 0] and want["valid"] == [k + 4, 1, 0]
            for q in ([], [""], ["", ""], short):
                r = ix.query(q, bits=True)
                assert len(r.kmers) == len(r.valid) == len(r.found) == len(q) and not r.kmers.any() and not r.valid.any() and not r.found.any()
                assert len(r.valid_bits) == len(r.present_bits) == (sum(map(len, q)) + 63) // 64
                assert not r.valid_bits.any() and not r.present_bits.any()
    with api.KmerIndex(full[:1], k) as ix:  # a full index, empty queries
        for q in ([], [""], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
            r = ix.query(q, bits=True)
            assert len(r.kmers) == len(r.valid) == len(r.found) == (len(q) if isinstance(q, list) else 0)
            assert len(r.valid_bits) == len(r.present_bits) == 0 and not r.found.any()
        _assert_equals_ref(ix, R.index_set(full[:1], k), short + full, k)


def test_reuse_and_determinism(gpu):
    rng = random.Random(9)
    genome = _dna(rng, 3000)
    a = [genome[i:i + 400] for i in range(0, 2700, 300)]
    b = [synth.revcomp(genome[1000:2500]), _dna(rng, 500)]
    queries = [[genome[100:900], _dna(rng, 300), "ACGTN" * 50], [synth.revcomp(genome)[:-1] + "N", ""], [_dna(rng, 70)] * 5 + [genome[2000:2100].lower()]]
    ka, kb = 21, 45
    sa, sb = R.index_set(a, ka), R.index_set(b, kb)
    ia, ib = api.KmerIndex(a, ka), api.KmerIndex(b, kb)  # two indexes of different k alive at once
    assert ia.info.distinct == api.compare_kmer_sets(a, a, ka).distinct_a == len(sa)
    assert ib.info.distinct == api.compare_kmer_sets(b, b, kb).distinct_a == len(sb)
    assert ia.info.device_bytes >= 8 * ia.info.slots and ia.info.slots >= 2 * ia.info.occurrences
    first = ia.query(queries[0], bits=True)
    for q in queries:
        _assert_equals_ref(ia, sa, q, ka)
        _assert_equals_ref(ib, sb, q, kb)
    again = ia.query(queries[0], bits=True)
    for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
        assert np.array_equal(getattr(first, f), getattr(again, f)), f
    api.release_device_memory(0)
    other = api.KmerIndex([_dna(rng, 5000)], 33)  # another index built and closed in between
    other.close()
    other.close()
    api.release_device_memory(0)
    for q in queries:
        _assert_equals_ref(ia, sa, q, ka)
        _assert_equals_ref(ib, sb, q, kb)
    twin = api.KmerIndex(a, ka)
    assert twin.info == ia.info
    ia.close()
    with pytest.raises(ValueError):
        ia.query(queries[0])
    _assert_equals_ref(ib, sb, queries[0], kb)
    _assert_equals_ref(twin, sa, queries[0], ka)
    ib.close()
    twin.close()
    t = api.last_kmer_query_times()
    assert set(t) == {"build_upload_ms", "build_pack_ms", "build_insert_ms", "query_upload_ms", "query_pack_ms", "query_probe_ms"}
    assert all(v >= 0 for v in t.values()) and t["query_probe_ms"] > 0 and t["build_insert_ms"] > 0


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


def _numpy_query(sorted_codes, seq, off, k):
    """The restatement for k <= 31 by numpy: canonical codes of all windows, searchsorted in the sorted index codes."""
    b = LUT[seq]
    bad = b > 3
    fwd, rc = synth._kmer_codes(np.where(bad, 0, b), k)
    canon = np.minimum(fwd, rc)
    n = len(fwd)
    o = off.astype(np.int64)
    lens = np.diff(o)
    rec = np.repeat(np.arange(len(lens)), lens)[:n]
    start = np.arange(n) + k <= o[1:][rec]  # the window lies inside its record
    cb = np.concatenate([[0], np.cumsum(bad)])
    valid = start & (cb[k:k + n] - cb[:n] == 0)
    at = np.searchsorted(sorted_codes, canon)
    found = valid & (sorted_codes[np.minimum(at, len(sorted_codes) - 1)] == canon)
    words = (len(seq) + 63) // 64

    def bits(x):
        full = np.zeros(words * 64, np.uint8)
        full[:n] = x
        return np.packbits(full, bitorder="little").view(np.uint64)

    return {"kmers": np.maximum(lens - k + 1, 0).astype(np.uint64), "valid": np.bincount(rec[valid], minlength=len(lens)).astype(np.uint64),
            "found": np.bincount(rec[found], minlength=len(lens)).astype(np.uint64), "valid_bits": bits(valid), "present_bits": bits(found)}


@pytest.fixture(scope="module")
def gseq_unitigs():
    return synth.g_seq_arrays(200_000, seed=5, k=31)


def test_larger_case_k31(gpu, gseq_unitigs):
    """~10^6 index bases, ~2 * 10^6 query bases: grids of many workgroups, real probe chains."""
    ua, k = gseq_unitigs, 31
    seq, off = _mutated_query(ua.seq, ua.off, 1)
    want = _numpy_query(ua.kmers, seq, off, k)
    with api.KmerIndex((ua.seq, ua.off), k) as ix:
        assert ix.info.distinct == len(ua.kmers) == ix.info.occurrences
        got = ix.query((seq, off), bits=True)
    for f, w in want.items():
        assert np.array_equal(getattr(got, f), w), f
    total, valid, found = int(got.kmers.sum()), int(got.valid.sum()), int(got.found.sum())
    assert 100_000 < found < valid < total and len(seq) > 1_900_000


def test_larger_case_k41(gpu, gseq_unitigs):
    """A tenth of that with the wide table form, against the Python set."""
    ua, k = gseq_unitigs, 41
    o = ua.off.astype(np.int64)
    n_rec = int(np.searchsorted(o, 100_000))
    sub_seq, sub_off = ua.seq[:o[n_rec]], ua.off[:n_rec + 1]
    seq, off = _mutated_query(sub_seq, sub_off, 2)
    text, qo = seq.tobytes().decode(), off.astype(np.int64)
    index = [sub_seq[o[i]:o[i + 1]].tobytes().decode() for i in range(n_rec)]
    query = [text[qo[i]:qo[i + 1]] for i in range(len(qo) - 1)]
    iset = R.index_set(index, k)
    want = R.query(iset, query, k)
    with api.KmerIndex(index, k) as ix:
        assert ix.info.distinct == len(iset)
        got = ix.query((seq, off), bits=True)
    for f, w in want.items():
        assert getattr(got, f).tolist() == w, f
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])


def test_through_the_product(gpu, tmp_path):
    k = 15
    g = synth.g_seq(3000, seed=11, k=k)
    rng = random.Random(3)
    units = g.unitigs
    u_fa, q_fa, t_fa = tmp_path / "u.fa", tmp_path / "q.fa", tmp_path / "t.fa"
    u_fa.write_text("".join(f">u{i} LN:i:{len(s)}\n{s}\n" for i, s in enumerate(units)))
    query = []
    for i in range(40):
        s = list(rng.choice(units) if rng.random() < 0.7 else _dna(rng, rng.randint(0, 60)))
        for j in range(len(s)):
            if rng.random() < 0.03:
                s[j] = rng.choice("ACGTNn")
        query.append(_flip_case(rng, "".join(s)))
    query[5] = ""
    q_fa.write_text("".join(f">q{i}\tmutated\n" + "".join(s[j:j + 50] + "\n" for j in range(0, len(s), 50)) for i, s in enumerate(query)))

    def run(*a):
        return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)

    r = run("--fa-in", str(u_fa), "-k", str(k), "--greedytigs-fa-out", str(t_fa))
    assert r.returncode == 0, r.stderr[-2000:]
    tsv, pres, tsv_gz, pres_gz = tmp_path / "r.tsv", tmp_path / "p.txt", tmp_path / "r.tsv.gz", tmp_path / "p.txt.gz"
    r = run("--fa-in", str(t_fa), "-k", str(k), "--query-fa", str(u_fa), "--query-fa", str(q_fa), "--query-out", str(tsv),
            "--query-presence-out", str(pres))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split("\t") for l in tsv.read_text().splitlines()]
    assert rows[0] == ["record", "length", "kmers", "valid", "found"] and len(rows) == 1 + len(units) + len(query)
    lines = pres.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == len(units) + len(query) + 1
    want = R.query(g.kmers, query, k)
    for i, s in enumerate(units):  # the tigs spell the input's set: every k-mer of a unitig is found
        n = len(s) - k + 1
        assert rows[1 + i] == [f"u{i}", str(len(s)), str(n), str(n), str(n)] and lines[i] == "1" * n
    for i, s in enumerate(query):
        row, line = rows[1 + len(units) + i], lines[len(units) + i]
        assert row == [f"q{i}", str(len(s)), str(want["kmers"][i]), str(want["valid"][i]), str(want["found"][i])], (i, row)
        assert line == R.presence(want, query, i)
        assert len(line) == want["kmers"][i] and line.count("1") == want["found"][i] and line.count("-") == want["kmers"][i] - want["valid"][i]
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])
    log = [l for l in r.stderr.splitlines() if l.startswith("Querying ")]
    n_u = sum(len(s) - k + 1 for s in units)
    assert len(log) == 2 and log[0].startswith(f"Querying {u_fa}: {len(units)} records, {n_u} k-mers, {n_u} valid, {n_u} found (100.00 %) in ")
    assert log[1].startswith(f"Querying {q_fa}: {len(query)} records, {sum(want['kmers'])} k-mers, {sum(want['valid'])} valid, {sum(want['found'])} found (")
    assert log[1].endswith(" s")
    r = run("--fa-in", str(t_fa), "-k", str(k), "--query-fa", str(u_fa), "--query-fa", str(q_fa), "--query-out", str(tsv_gz),
            "--query-presence-out", str(pres_gz))
    assert r.returncode == 0, r.stderr[-2000:]
    assert gzip.decompress(tsv_gz.read_bytes()) == tsv.read_bytes() and gzip.decompress(pres_gz.read_bytes()) == pres.read_bytes()
