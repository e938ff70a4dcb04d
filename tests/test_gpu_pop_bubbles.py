"""Bubble popping on the GPU (api.compact_unitigs_simplified) against the restatement (bubble_ref.py), as exact integers and
bytes in every field: the hand-derived cases of test_bubble_ref.py for narrow and wide k and on both sides of k - 1 = 32; the filter
and tips beside the arms; colours with and without the split; the input reversed and reverse-complemented; the fuzz whose generator
test_bubble_ref.py vouches for; an input beyond one workgroup, one wave and one scan block; and the call with nothing to pop against
the cleaned call."""
import random

import numpy as np
import pytest

import bubble_ref as B
import compact_ref as R
import tip_clip_ref as T
from matchtigs_amd import api

pytestmark = pytest.mark.gpu
KS = [4, 5, 31, 32, 33, 34, 40, 64]
HAND = ["snp_short_L", "snp_tie", "snp_variant_wins", "ratio2_even", "ratio2_3to1", "deletion_goes", "deletion_wins", "three_alleles", "long_arm",
        "hairpin", "ring_snp", "snp_and_tip", "nested_one_round", "nested_two_rounds"]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


def _call(records, k, m=1, record_colors=None, n_colors=0, **kw):
    return api.compact_unitigs_simplified(records, k, min_abundance=m, record_colors=record_colors, n_colors=n_colors, kmer_counts=True, **kw)


def _check(records, k, **kw):
    """The device's answer equals the restatement's in every field -> (the device's, the restatement's)."""
    want = B.compact_simplified(records, k, **kw)
    got = _call(records, k, **kw)
    unitigs, stats, closed, ab, col, classes, cleaning, bubbles = want
    store, c, a, co, cc, cl, bu = got
    assert store.sequences() == unitigs
    assert store.arrays()[1].tolist() == np.concatenate([[0], np.cumsum([len(u) for u in unitigs])]).astype(np.int64).tolist()
    assert c == api.Compaction(**stats) and c.closed_walks == sum(closed)
    assert cl == api.Cleaning(**cleaning)
    assert bu == api.Bubbles(**bubbles)
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == ab[f], f
    assert a.spectrum.tolist() == ab["spectrum"] and a.unitig_sums.tolist() == ab["unitig_sums"] and a.kmer_counts.tolist() == ab["kmer_counts"]
    assert int(a.unitig_sums.sum()) == a.kept_occurrences - cl.removed_occurrences - bu.removed_occurrences
    assert a.distinct_kept - c.distinct_kmers == cl.removed_kmers + bu.arm_kmers
    if col is None:
        assert co is None and cc is None
    else:
        assert co.n_colors == col["n_colors"] and co.kmer_colors.tolist() == col["kmer_colors"]
        for f in ("per_color", "shared", "occupancy"):
            assert getattr(co, f).tolist() == col[f], f
        for f in ("masks", "kmers", "runs", "first", "kmer_class"):
            assert getattr(cc, f).tolist() == classes[f], f
        assert int(cc.runs.sum()) == classes["n_runs"]
        if kw.get("split"):
            assert int(cc.runs.sum()) == c.unitigs
    return got, want


# ---- the hand-derived cases, at every k ----
@pytest.fixture(scope="module")
def hand():
    out = {}
    for k in [11] + KS:
        rng = random.Random(25 if k == 11 else 2500 + k)
        out[k] = B.hand_cases(rng, _dna(rng), k)
    return out


@pytest.mark.parametrize("k", [11] + KS)
def test_the_hand_derived_cases(gpu, hand, k):
    cases = hand[k]
    p = cases["_parts"]
    for name in HAND:
        records, _, kw = cases[name]
        try:
            got, _ = _check(records, k, **kw)
        except AssertionError:
            print("case", name, "k", k)
            raise
        if k <= 5:
            continue  # (a tiny k has other forks: the restatement alone says what comes out)
        bu, cl = got[6], got[5]
        if name in ("snp_short_L", "ratio2_even", "hairpin"):
            assert bu == api.Bubbles(0, 0, 0)
        if name in ("snp_tie", "ratio2_3to1", "deletion_goes", "three_alleles", "snp_and_tip", "nested_two_rounds"):
            assert got[0].sequences() == [p["g"]]
        if name in ("snp_tie", "snp_variant_wins", "ratio2_3to1", "deletion_wins", "long_arm", "ring_snp", "snp_and_tip", "nested_one_round"):
            assert bu == api.Bubbles(1, k, k)
        if name == "deletion_goes":
            assert bu == api.Bubbles(1, k - 1, k - 1)
        if name == "three_alleles":
            assert bu == api.Bubbles(2, 2 * k, 2 * k) and cl.rounds_run == 1
        if name == "ring_snp":
            assert got[1].closed_walks == 1 and got[0].sequences() == R.compact([p["ring_rec"]], k)[0]
        if name == "snp_and_tip":
            assert (cl.tips, cl.tip_kmers, cl.removed_occurrences) == (1, 4, 4)
        if name == "nested_two_rounds":
            assert bu == api.Bubbles(2, 3 * k - 1, k + 2 * (2 * k - 1)) and cl.rounds_run == 3


@pytest.mark.parametrize("k", [5, 31, 34])
def test_the_filter_and_tips_beside_the_arms(gpu, k):
    rng = random.Random(2600 + k)
    dna = _dna(rng)
    g = T.genome(rng, 60 * max(k, 8), max(k, 8))
    tips, _ = T.plant_tips(rng, g, k, 5, dna)
    snps, _ = B.plant_snps(rng, g, k, 6)
    records = [g] + tips + snps[1:] + tips[1:] + snps[1:4]  # every tip twice, three of the SNPs twice: m = 2 drops the other three
    _check(records, k, pop_bubbles=2 * k, clip_tips=k, m=1)
    loose, _ = _check(records, k, pop_bubbles=2 * k, clip_tips=k, m=1, rounds=3)  # (a tip's fork on an arm: the arm is one walk a round later)
    tight, _ = _check(records, k, pop_bubbles=2 * k, clip_tips=k, m=2, rounds=3)
    _check(records, k, pop_bubbles=2 * k, bubble_ratio=2, clip_tips=k, m=2, rounds=2)
    if k > 5:
        assert loose[6].arms == 6 and loose[5].tips == 5 and tight[6].arms == 3 and tight[5].tips == 5
        assert loose[0].sequences() == tight[0].sequences() == [g]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("k", [5, 31, 34])
def test_colours_with_and_without_the_split(gpu, k, split):
    rng = random.Random(2700 + k)
    g = T.genome(rng, 60 * max(k, 8), max(k, 8))
    snps, _ = B.plant_snps(rng, g, k, 6)
    records = snps + [g[:len(g) // 2]]  # g is colour 0, its first half colour 1 too, the variants 2 and 0 in turn
    colors = [0] + [2 * (i % 2) for i in range(6)] + [1]
    for rounds in (1, 3):
        got, _ = _check(records, k, pop_bubbles=2 * k, rounds=rounds, record_colors=colors, n_colors=3, split=split)
    if k > 5:
        # (variants whose site lies in g's first half: g's arm there has mean 2 and wins; the others tie and g's creators win)
        assert got[6].arms == 6 and got[1].unitigs == (2 if split else 1)
    _check(records, k, pop_bubbles=2 * k, bubble_ratio=2, clip_tips=k, rounds=2, record_colors=colors, n_colors=3, split=split)


def _kmer_set(seqs, k):
    return {R.canonical(u[i:i + k]) for u in seqs for i in range(len(u) - k + 1)}


@pytest.mark.parametrize("k", [5, 31, 33])
def test_the_other_strand_and_the_other_order_pop_the_same_arms(gpu, k):
    """Where no tie is settled by creators, reversing the input and reverse-complementing every record changes creators and readings
    only: the same k-mers stay, the counters are equal, and the unitigs are the same set up to strand. Ties (means equal) follow the
    contract's creator order on either input, which the restatement holds them to."""
    rng = random.Random(2800 + k)
    g = T.genome(rng, 60 * max(k, 8), max(k, 8))
    snps, _ = B.plant_snps(rng, g, k, 8)
    records = [g, g] + snps[1:] + snps[1:4] * 2  # 2 : 1 and 2 : 3 -- no ties
    turned = [R.revcomp(r) for r in reversed(records)]
    for kw in (dict(pop_bubbles=2 * k), dict(pop_bubbles=2 * k, bubble_ratio=2, rounds=2)):
        a, _ = _check(records, k, **kw)
        b, _ = _check(turned, k, **kw)
        if k <= 5:
            continue  # (a tiny k has other forks, and ties among them)
        assert a[6] == b[6] and a[5] == b[5] and a[1].distinct_kmers == b[1].distinct_kmers
        assert _kmer_set(a[0].sequences(), k) == _kmer_set(b[0].sequences(), k)
        assert sorted(min(u, R.revcomp(u)) for u in a[0].sequences()) == sorted(min(u, R.revcomp(u)) for u in b[0].sequences())
    tie = [g] + snps[1:]  # all ties: the restatement decides by creators on either input
    _check(tie, k, pop_bubbles=2 * k)
    _check([R.revcomp(r) for r in reversed(tie)], k, pop_bubbles=2 * k)


def test_fuzz_of_tiny_inputs(gpu):
    popped = 0
    for i, (records, k, kw) in enumerate(B.fuzz_cases()):
        try:
            got, _ = _check(records, k, **kw)
        except AssertionError:
            print("input", i, "k", k, records, kw)
            raise
        popped += got[6].arms > 0
    assert popped >= 60, popped  # (test_bubble_ref.py says so of the restatement)


def test_two_thousand_snps_cross_workgroups_and_waves(gpu):
    k = 31
    rng = random.Random(2900)
    g = "".join(rng.choices("ACGT", k=200_000))
    records, sites = B.plant_snps(rng, g, k, 2000)
    assert len(sites) == 2000
    want = api.compact_unitigs([g], k)[0]
    data, off = want.arrays()
    assert len(off) == 2  # the single unitig g
    one = api.compact_unitigs_simplified([g] + records, k, pop_bubbles=2 * k)
    two = api.compact_unitigs_simplified([g] + records, k, pop_bubbles=2 * k, rounds=2)
    for got in (one, two):
        assert got[6] == api.Bubbles(2000, 2000 * 31, 2000 * 31) and got[5].removed_kmers == 0
        assert got[0].arrays()[0].tobytes() == data.tobytes() and np.array_equal(got[0].arrays()[1], off)
        assert got[2].distinct_kept == got[1].distinct_kmers + 2000 * 31
        assert int(got[2].unitig_sums.sum()) == got[2].kept_occurrences - 2000 * 31
    assert (one[5].rounds_run, two[5].rounds_run) == (1, 2)
    assert api.compact_unitigs([g] + records, k)[1].unitigs == 1 + 3 * 2000


def test_nothing_to_pop_equals_the_cleaned_call(gpu):
    rng = random.Random(3000)
    dna = _dna(rng)
    k = 31
    g = T.genome(rng, 2000, k)
    records, _ = T.plant_tips(rng, g, k, 20, dna)
    colors = [i % 4 for i in range(len(records))]
    for kw in (dict(clip_tips=k), dict(clip_tips=k, remove_isolated=k, rounds=3, min_abundance=2), dict(),
               dict(clip_tips=k, record_colors=colors, n_colors=4, split=True)):
        cleaned = api.compact_unitigs_cleaned(records, k, kmer_counts=True, **kw)
        off = api.compact_unitigs_simplified(records, k, pop_bubbles=0, kmer_counts=True, **kw)
        assert api.last_bubble_times() == {"bubble_ms": 0.0}
        assert off[6] == api.Bubbles(0, 0, 0) and off[5] == cleaned[5] and off[1] == cleaned[1]
        assert off[0].arrays()[0].tobytes() == cleaned[0].arrays()[0].tobytes() and np.array_equal(off[0].arrays()[1], cleaned[0].arrays()[1])
        for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
            assert getattr(off[2], f) == getattr(cleaned[2], f), f
        for f in ("unitig_sums", "kmer_counts", "spectrum"):
            assert np.array_equal(getattr(off[2], f), getattr(cleaned[2], f)), f
        if "record_colors" in kw:
            for f in ("kmer_colors", "per_color", "shared", "occupancy"):
                assert np.array_equal(getattr(off[3], f), getattr(cleaned[3], f)), f
            for f in ("masks", "kmers", "runs", "first", "kmer_class"):
                assert np.array_equal(getattr(off[4], f), getattr(cleaned[4], f)), f
        else:
            assert off[3] is None and off[4] is None
    snps, _ = B.plant_snps(rng, g, k, 5)
    popped = api.compact_unitigs_simplified(snps, k, pop_bubbles=2 * k)
    assert popped[6].arms == 5 and api.last_bubble_times()["bubble_ms"] > 0 and api.last_clean_times()["rounds_run"] == 1
    assert popped[0].sequences() == [g]
    store = api.compact_unitigs(snps, k)[0]  # a store goes in as well
    a, b = api.compact_unitigs_simplified(store, k, pop_bubbles=2 * k), api.compact_unitigs_simplified(store.sequences(), k, pop_bubbles=2 * k)
    assert a[0].sequences() == b[0].sequences() and a[6] == b[6] == api.Bubbles(5, 5 * k, 5 * k) and a[1].unitigs == 1


def test_the_arguments(gpu):
    for kw in (dict(pop_bubbles=-1), dict(pop_bubbles=1.5), dict(pop_bubbles=True), dict(pop_bubbles=9, bubble_ratio=0), dict(pop_bubbles=9, bubble_ratio=256),
               dict(rounds=0), dict(rounds=65), dict(clip_tips=-1), dict(split=True), dict(min_abundance=0)):
        with pytest.raises(ValueError):
            api.compact_unitigs_simplified(["ACGTACGTTT"], 4, **kw)
