"""Inputs for the sparse minimizer index, shared by the restatement's test (test_tig_index_ref.py, no GPU) and the
GPU test (test_gpu_tig_index.py): random index / query pairs and the engineered hazards, each the smallest that can go wrong.
A case is (name, index records, query records, k, m, bucket_limit); m / bucket_limit None: the default."""
import random

import tig_index_ref as T
from matchtigs_amd import synth

JUNK = "NNNNnnRYKMSWBDHVxX-*. \x00\x7f5"  # what a query may hold besides ACGT


def dna(rng, n, weights=(1, 1, 1, 1)):
    return "".join(rng.choices("ACGT", weights, k=n))


def flip_case(rng, s):
    return "".join(c.lower() if rng.random() < 0.3 else c for c in s)


def random_pair(rng, k):
    """An index cut from one short genome and its reverse complement (k-mers repeat in both orientations, a palindrome planted for
    even k, a biased alphabet, mixed case, lengths 0 .. 3 k) and a query of copies, pieces, foreign records and mixtures, with junk
    bytes thrown in."""
    weights = rng.choice([(1, 1, 1, 1), (6, 1, 1, 2), (5, 0, 0, 5), (0, 4, 4, 0), (3, 1, 0, 0)])
    anti = tuple(int(w == 0) for w in weights) if 0 in weights else (1, 1, 1, 1)
    half = dna(rng, k // 2, weights)
    genome = dna(rng, 2 * k + 2, weights) + (half + synth.revcomp(half) if k % 2 == 0 else "") + dna(rng, 2 * k + 2, weights)
    sources = (genome, synth.revcomp(genome))

    def piece(n):
        g = sources[rng.random() < 0.5]
        at = rng.randint(0, len(g) - n)
        return g[at:at + n]

    index = [flip_case(rng, piece(rng.randint(0, 3 * k)) if rng.random() < 0.85 else dna(rng, rng.randint(0, 3 * k), weights))
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
            s = dna(rng, n, anti)
        else:  # across a record boundary of the index's concatenation, or half foreign
            s = "".join(index).upper()[:n] if rng.random() < 0.5 and index else piece(n // 2) + dna(rng, n - n // 2, anti)
        s = list(flip_case(rng, s))
        if s and rng.random() < 0.4:
            for _ in range(rng.randint(1, 3)):
                s[rng.randrange(len(s))] = rng.choice(JUNK)
        query.append("".join(s))
    return index, query


def random_ms(k):
    """m in {1, 2, ceil(k / 2), min(k, 31), default}, those that are valid for k, once each."""
    return sorted({m for m in (1, 2, -(-k // 2), min(k, 31)) if 1 <= m <= min(k, 31)}) + [None]


def _window(rng, k, m, make):
    """A k-mer built by make(M, filler) around a random m-mer M whose class is the window's minimizer and occurs at two offsets."""
    for _ in range(100000):
        x = make(dna(rng, m), lambda n: dna(rng, n))
        if len(x) != k:
            continue
        v, j1, jl = T.minimizer(x, m)
        if j1 != jl:
            return x
    raise AssertionError("no such window")


def both_ways(x, flank_rng, k):
    """x inside a record, indexed forward and queried forward and as its reverse complement, and the other way round."""
    a, b = dna(flank_rng, k + 3), dna(flank_rng, k + 5)
    rec = a + x + b
    queries = [x, synth.revcomp(x), rec, synth.revcomp(rec), x[1:] + "A", "C" + x[:-1]]
    return [([rec], queries), ([synth.revcomp(rec)], queries), ([x], queries), ([synth.revcomp(x)], queries)]


def engineered():
    rng = random.Random(2828)
    cases = []

    def add(name, index, query, k, m=None, limit=None):
        cases.append((name, index, query, k, m, limit))

    # the minimizer's class twice in one window: twice on one strand, once per strand
    for k, m in ((11, 4), (12, 3), (33, 5)):
        gap = k - 2 * m
        same = _window(rng, k, m, lambda M, f: M + f(gap) + M)
        other = _window(rng, k, m, lambda M, f: M + f(gap) + synth.revcomp(M))
        for what, x in (("same strand", same), ("both strands", other)):
            for i, (index, query) in enumerate(both_ways(x, rng, k)):
                add(f"minimizer twice, {what}, k={k} m={m} #{i}", index, query, k, m)
    # a palindromic m-mer (even m) as the minimizer
    for k, m in ((9, 4), (20, 6)):
        def pal(M, f, k=k, m=m):
            h = M[:m // 2]
            return f(2) + h + synth.revcomp(h) + f(k - m - 2)
        for _ in range(100000):
            x = pal(dna(rng, m), lambda n: dna(rng, n))
            v, j1, _ = T.minimizer(x, m)
            if x[j1:j1 + m] == synth.revcomp(x[j1:j1 + m]):
                break
        else:
            raise AssertionError("no palindromic minimizer")
        for i, (index, query) in enumerate(both_ways(x, rng, k)):
            add(f"palindromic minimizer k={k} m={m} #{i}", index, query, k, m)
    # a palindromic k-mer
    for k, m in ((8, 3), (32, None), (10, 10)):
        h = dna(rng, k // 2)
        x = h + synth.revcomp(h)
        for i, (index, query) in enumerate(both_ways(x, rng, k)):
            add(f"palindromic k-mer k={k} #{i}", index, query, k, m)
    # m = k and m = 1
    for k in (1, 2, 7, 31, 40):
        for m in (1, min(k, 31)):
            index, query = random_pair(rng, k)
            add(f"m={m} k={k}", index + [dna(rng, 2 * k)], query + index, k, m)
    # k-mers that only the concatenation spells; the last k - 1 bases against the padding behind the text
    for k, m in ((9, 4), (31, None), (35, 12)):
        a, b, c = dna(rng, 2 * k), dna(rng, k + 1), dna(rng, k)
        across = [a[-j:] + b[:k - j] for j in range(1, k)] + [b[-j:] + c[:k - j] for j in range(1, k)]
        tail = [c[-j:] + "A" * (k - j) for j in range(1, k)]
        add(f"record borders k={k}", [a, b, c], across + tail + [a + b, b + c, a, b, c], k, m)
        add(f"record borders, empty records between, k={k}", [a, "", b, "", "", c, ""], across + tail + [a + b + c], k, m)
    # present only at the very start / the very end of a record
    for k, m in ((7, 3), (33, None)):
        s = dna(rng, 3 * k)
        ends = [s[:k], s[-k:], synth.revcomp(s[:k]), synth.revcomp(s[-k:])]
        add(f"record ends k={k}", [s], ends + ["G" + s[:k - 1], s[-k + 1:] + "G"], k, m)
        add(f"record ends, one window, k={k}", [s[:k], s[-k:]], ends + [s], k, m)
    # records shorter than k and shorter than m
    for k, m in ((12, 5), (40, None)):
        m_used = m or T.default_m(k)
        shorts = [dna(rng, n) for n in (0, 1, m_used - 1, m_used, k - 1)]
        full = dna(rng, 2 * k)
        add(f"short records k={k}", shorts[:3] + [full] + shorts[3:], shorts + [full, synth.revcomp(full)], k, m)
        add(f"only short records k={k}", shorts, shorts + [full], k, m)
    # the empty index and the empty query
    for k in (1, 5, 31, 33):
        full = dna(rng, 2 * k + 3)
        for i, index in enumerate(([], [""], ["", ""])):
            add(f"empty index k={k} #{i}", index, [full, "N" + full, ""], k)
        for i, query in enumerate(([], [""], ["", ""])):
            add(f"empty query k={k} #{i}", [full], query, k)
    return cases


def neighbours(x):
    """Every one-substitution neighbour of x."""
    return [x[:i] + c + x[i + 1:] for i in range(len(x)) for c in "ACGT" if c != x[i]]


def repeats_case(n, k, seed=5):
    """Poly-A and (AC)^(n / 2) beside random sequence: index records, and a query of the repeats' k-mers, their one-substitution
    neighbours and the index itself reverse-complemented."""
    rng = random.Random(seed)
    index = [dna(rng, n), "A" * n, dna(rng, 200), "AC" * (n // 2), dna(rng, n)]
    poly, ac, ca = "A" * k, ("AC" * k)[:k], ("CA" * k)[:k]
    query = [poly, ac, ca, synth.revcomp(ac), "T" * (2 * k), ("GT" * k)] + neighbours(poly)[::3] + neighbours(ac)[::3] + \
            [synth.revcomp(s) for s in index]
    return index, query
