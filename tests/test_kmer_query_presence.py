"""KmerQueryResult.presence / presence_lines (api.py) without a GPU: a result filled from the restatement (kmer_query_ref.py) spells
the same strings, for every record and for every slice of records, and spelling all records costs one pass over the bit arrays, not
one per record."""
import itertools
import random
import time

import numpy as np
import pytest

import kmer_query_ref as R
from matchtigs_amd import api


def _result(index, query, k):
    want = R.query(R.index_set(index, k), query, k)
    off = np.array(list(itertools.accumulate((len(s) for s in query), initial=0)), np.uint64)
    u = lambda f: np.array(want[f], np.uint64)
    return want, api.KmerQueryResult(k, off, u("kmers"), u("valid"), u("found"), u("valid_bits"), u("present_bits"))


@pytest.mark.parametrize("k", [1, 3, 7])
def test_presence_lines_equal_the_restatement(k):
    rng = random.Random(k)
    index = ["".join(rng.choices("AT", k=40)) for _ in range(6)]  # (no C or G: at k = 1 those are the only other class)
    query = ["".join(rng.choice("ACGTacN") for _ in range(rng.choice((0, 0, 1, k - 1, k, k + 1, 9, 63, 64, 65, 130)))) for _ in range(60)]
    want, r = _result(index, query, k)
    lines = [R.presence(want, query, i) for i in range(len(query))]
    assert {c for l in lines for c in l} == {"0", "1", "-"} and "" in lines
    for i, line in enumerate(lines):
        assert r.presence(i) == line and len(line) == want["kmers"][i]
    assert r.presence_lines() == "".join(l + "\n" for l in lines).encode()
    for a, b in [(0, 0), (60, 60), (0, 1), (59, 60), (7, 23), (23, 41)]:  # slices that start and end inside a byte and a word
        assert r.presence_lines(a, b) == "".join(l + "\n" for l in lines[a:b]).encode()
    assert b"".join(r.presence_lines(a, a + 7) for a in range(0, 56, 7)) + r.presence_lines(56) == r.presence_lines()
    with pytest.raises(IndexError):
        r.presence_lines(3, 61)
    with pytest.raises(ValueError):
        api.KmerQueryResult(k, r.offsets, r.kmers, r.valid, r.found).presence(0)


def test_presence_cost_is_linear_in_the_bases():
    """20 000 records over 2 * 10^6 bases: every record's string one by one, and all of them at once. A pass over the whole bit arrays
    per record would unpack 4 * 10^10 bits here."""
    n_rec, length, k = 20_000, 100, 5
    rng = np.random.default_rng(0)
    words = n_rec * length // 64
    valid = rng.integers(0, 2 ** 63, words, dtype=np.uint64)
    present = valid & rng.integers(0, 2 ** 63, words, dtype=np.uint64)
    off = np.arange(n_rec + 1, dtype=np.uint64) * np.uint64(length)
    kmers = np.full(n_rec, length - k + 1, np.uint64)
    r = api.KmerQueryResult(k, off, kmers, kmers, kmers, valid, present)
    t0 = time.perf_counter()
    text = r.presence_lines()
    one_by_one = [r.presence(i) for i in range(n_rec)]
    took = time.perf_counter() - t0
    assert text == "".join(l + "\n" for l in one_by_one).encode() and len(text) == n_rec * (length - k + 2)
    assert took < 20, took
