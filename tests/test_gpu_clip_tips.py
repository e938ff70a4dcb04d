"""Tip clipping and the removal of isolated unitigs on the GPU (api.compact_unitigs_cleaned) against the restatement
(tip_clip_ref.py), as exact integers and bytes: the hand-derived cases of test_tip_clip_ref.py; planted tips for narrow and wide k and
for k - 1 <= 32 against k - 1 > 32; tips at a self-mirror node, a palindromic k-mer at a tip's end, hairpins, empty and short records,
lower case; tips that exist only behind the abundance filter; colours with and without the split; the call with nothing to clean
against the older calls; a fuzz over tiny alphabets; and an input beyond one workgroup and one scan block."""
import random

import numpy as np
import pytest

import compact_ref as R
import tip_clip_ref as T
from matchtigs_amd import api

pytestmark = pytest.mark.gpu
KS = [4, 5, 31, 32, 33, 34, 40, 64]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


def _call(records, k, m=1, record_colors=None, n_colors=0, **kw):
    return api.compact_unitigs_cleaned(records, k, min_abundance=m, record_colors=record_colors, n_colors=n_colors, kmer_counts=True, **kw)


def _check(records, k, **kw):
    """The device's answer equals the restatement's in every field -> (the device's, the restatement's)."""
    want = T.compact_cleaned(records, k, **kw)
    got = _call(records, k, **kw)
    unitigs, stats, closed, ab, col, classes, cleaning = want
    store, c, a, co, cc, cl = got
    assert store.sequences() == unitigs
    assert store.arrays()[1].tolist() == np.concatenate([[0], np.cumsum([len(u) for u in unitigs])]).astype(np.int64).tolist()
    assert c == api.Compaction(**stats) and c.closed_walks == sum(closed)
    assert cl == api.Cleaning(**cleaning)
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == ab[f], f
    assert a.spectrum.tolist() == ab["spectrum"] and a.unitig_sums.tolist() == ab["unitig_sums"] and a.kmer_counts.tolist() == ab["kmer_counts"]
    assert int(a.unitig_sums.sum()) == a.kept_occurrences - cl.removed_occurrences
    assert a.distinct_kept - c.distinct_kmers == cl.removed_kmers
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


# ---- the hand-derived cases ----
@pytest.fixture(scope="module")
def cases():
    rng = random.Random(24)
    return T.hand_cases(rng, _dna(rng))


@pytest.mark.parametrize("name", ["tip6_stays", "tip6_goes", "y_one_round", "y_two_rounds", "y_many_rounds", "isolated_goes", "isolated_stays",
                                  "stem_kept", "merge_kept", "lone_palindrome", "ring_tip"])
def test_the_hand_derived_cases(gpu, cases, name):
    records, k, kw = cases[name]
    got, _ = _check(records, k, **kw)
    p = cases["_parts"]
    if name in ("tip6_goes", "y_two_rounds", "y_many_rounds", "isolated_goes"):
        assert got[0].sequences() == [p["g"]]
    if name == "ring_tip":
        assert got[0].sequences() == R.compact([p["ring_rec"]], k)[0] and got[1].closed_walks == 1


@pytest.mark.parametrize("k", [11, 21, 31, 32, 40])
def test_planted_tips_give_the_genome_back(gpu, k):
    rng = random.Random(1000 + k)
    dna = _dna(rng)
    g = T.genome(rng, 3000, k)
    records, planted = T.plant_tips(rng, g, k, 40, dna)
    got, _ = _check(records, k, clip_tips=k)
    assert got[0].sequences() == R.compact([g], k)[0] and got[5].tips == 40 and got[5].tip_kmers == planted
    again, _ = _check(records, k, clip_tips=k, rounds=2)
    assert again[0].sequences() == got[0].sequences() and again[5].rounds_run == 2 and again[5].tips == 40


# ---- special shapes ----
def _site(rng, k):
    """A genome of 10 k bases and the node in its middle."""
    g = T.genome(rng, 10 * k, max(k, 8))
    return g, 5 * k


def _off(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


@pytest.mark.parametrize("k", [k for k in KS if k % 2 == 1])
def test_tips_anchored_at_a_self_mirror_node(gpu, k):
    rng = random.Random(300 + k)
    dna = _dna(rng)
    h = dna((k - 1) // 2)
    v = h + R.revcomp(h)  # its own reverse complement: every k-mer that ends in it also leaves it, mirrored
    records = [dna(3 * k) + "A" + v, dna(3 * k) + "C" + v, dna(2) + "G" + v, "T" + v]
    got, _ = _check(records, k, clip_tips=k, rounds=3)
    if k > 5:  # (random arms: no other fork)
        assert got[5].tips == 2 and got[5].tip_kmers == 4 and got[1].unitigs == 2
    _check(records[:1] + records[2:3], k, clip_tips=k, remove_isolated=2)  # two k-mer walks meet at the node: both anchored there
    _check(records[2:3], k, clip_tips=k, remove_isolated=k)  # alone: free on both sides


@pytest.mark.parametrize("k", [k for k in KS if k % 2 == 0])
def test_a_palindromic_kmer_at_a_tips_end(gpu, k):
    rng = random.Random(400 + k)
    dna = _dna(rng)
    g, at = _site(rng, k)
    h = dna(k // 2)
    pal = h + R.revcomp(h)
    tip = g[at:at + k - 1] + _off(rng, g[at + k - 1]) + dna(2) + pal  # the twin edge of its last k-mer anchors that end
    got, _ = _check([g, tip], k, clip_tips=2 * k + 4, rounds=4)
    if k > 5:
        assert got[5].tips == 0
    _check([g, R.revcomp(tip)], k, clip_tips=2 * k + 4, remove_isolated=3, rounds=4)
    _check([pal], k, clip_tips=9, remove_isolated=9)  # the lone palindrome


@pytest.mark.parametrize("k", KS)
def test_hairpins_empty_short_and_lower_case_records(gpu, k):
    rng = random.Random(500 + k)
    dna = _dna(rng)
    x = dna(2 * k)
    hairpin = x + R.revcomp(x)
    for kw in (dict(clip_tips=k), dict(remove_isolated=10 * k), dict(clip_tips=k, remove_isolated=k + 2, rounds=5)):
        _check([hairpin], k, **kw)
    g, at = _site(rng, k)
    tip = g[at:at + k - 1] + _off(rng, g[at + k - 1]) + dna(k // 2)
    hair_tip = x[-(k - 1):] + _off(rng, R.revcomp(x)[0]) + dna(1)
    records = ["", g.lower(), "ac"[:k - 1], tip[:len(tip) // 2].lower() + tip[len(tip) // 2:], "", hairpin, hair_tip, dna(k - 1), dna(k + 1).lower()]
    got, _ = _check(records, k, clip_tips=k, remove_isolated=k, rounds=4)
    if k > 5:
        assert got[5].tips >= 1 and got[5].isolated >= 1
    _check(["", "a", ""], k, clip_tips=k)  # no window at all
    everything, _ = _check([dna(k + 1)], k, remove_isolated=3)  # the whole input is isolated: nothing is left
    if k > 5:
        assert len(everything[0]) == 0 and everything[1].distinct_kmers == 0 and everything[5].isolated_kmers == 2


@pytest.mark.parametrize("k", [5, 31, 40])
def test_tips_that_exist_only_behind_the_filter(gpu, k):
    rng = random.Random(600 + k)
    dna = _dna(rng)
    g, at = _site(rng, k)
    branch = g[at:at + k - 1] + _off(rng, g[at + k - 1]) + dna(3 * k)  # seen once, its first 4 k-mers twice
    records = [g, branch, R.revcomp(g), branch[:k + 3].lower()]
    loose, _ = _check(records, k, clip_tips=k, m=1)
    tight, _ = _check(records, k, clip_tips=k, m=2)
    if k > 5:
        assert loose[5].tips == 0 and tight[5].tips == 1 and tight[5].tip_kmers == 4 and tight[5].removed_occurrences == 8
        assert tight[0].sequences() == [g] and tight[2].dropped == 3 * k - 3


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("k", [5, 31, 34])
def test_colours_and_the_split_decide_on_unsplit_unitigs(gpu, k, split):
    rng = random.Random(700 + k)
    dna = _dna(rng)
    g = T.genome(rng, 40 * max(k, 8), max(k, 8))
    records, _ = T.plant_tips(rng, g, k, 6, dna)
    # colours: g itself 0, half of g again as 1 (g's unitig has two masks), the tips 2 and 0 in turn; one tip in two pieces of two colours
    records += [g[:len(g) // 2], records[1][:k + 1]]
    colors = [0] + [2 * (i % 2) for i in range(6)] + [1, 1]
    for rounds in (1, 3):
        got, _ = _check(records, k, clip_tips=k, remove_isolated=k, rounds=rounds, record_colors=colors, n_colors=3, split=split, m=1)
    if k > 5:
        assert got[5].tips == 6
        assert got[1].unitigs == (2 if split else 1)  # g's two halves differ in their masks
    _check(records, k, clip_tips=k, rounds=2, record_colors=colors, n_colors=3, split=split, m=2)


def test_nothing_to_clean_equals_the_older_calls(gpu):
    rng = random.Random(800)
    dna = _dna(rng)
    k = 31
    g = T.genome(rng, 2000, k)
    records, _ = T.plant_tips(rng, g, k, 20, dna)
    colors = [i % 4 for i in range(len(records))]
    for m in (1, 2):
        plain = api.compact_unitigs(records, k)
        counted = api.compact_unitigs_counted(records, k, m, kmer_counts=True)
        off = api.compact_unitigs_cleaned(records, k, min_abundance=m, kmer_counts=True)
        assert off[5] == api.Cleaning(0, 0, 0, 0, 0, 0) and off[3] is None and off[4] is None
        assert off[0].arrays()[0].tobytes() == counted[0].arrays()[0].tobytes() and np.array_equal(off[0].arrays()[1], counted[0].arrays()[1])
        assert off[1] == counted[1] and np.array_equal(off[2].unitig_sums, counted[2].unitig_sums) and np.array_equal(off[2].kmer_counts, counted[2].kmer_counts)
        if m == 1:
            assert off[0].arrays()[0].tobytes() == plain[0].arrays()[0].tobytes() and off[1] == plain[1]
        assert api.compact_unitigs_cleaned(records, k, min_abundance=m)[2].kmer_counts is None
        for split in (False, True):
            classed = api.compact_unitigs_colored_classes(records, k, colors, 4, m, split)
            same = api.compact_unitigs_cleaned(records, k, 0, 0, 7, m, colors, 4, split)
            assert same[0].arrays()[0].tobytes() == classed[0].arrays()[0].tobytes() and same[1] == classed[1]
            for f in ("unitig_sums", "kmer_counts", "spectrum"):
                assert np.array_equal(getattr(same[2], f), getattr(classed[2], f)), f
            for f in ("kmer_colors", "per_color", "shared", "occupancy"):
                assert np.array_equal(getattr(same[3], f), getattr(classed[3], f)), f
            for f in ("masks", "kmers", "runs", "first", "kmer_class"):
                assert np.array_equal(getattr(same[4], f), getattr(classed[4], f)), f
    assert api.last_clean_times() == {"clean_ms": 0.0, "rounds_run": 0}
    store = api.compact_unitigs(records, k)[0]  # a store goes in as well
    a, b = api.compact_unitigs_cleaned(store, k, clip_tips=k), api.compact_unitigs_cleaned(store.sequences(), k, clip_tips=k)
    assert a[0].sequences() == b[0].sequences() == [g] and a[5] == b[5] and a[5].tips == 20
    t = api.last_clean_times()
    assert t["clean_ms"] > 0 and t["rounds_run"] == 1 and api.last_compact_times()["nodes_ms"] > 0


def test_the_arguments(gpu):
    for kw in (dict(rounds=0), dict(rounds=65), dict(clip_tips=-1), dict(remove_isolated=1.5), dict(split=True), dict(min_abundance=0),
               dict(record_colors=[0], n_colors=0), dict(record_colors=[0, 0], n_colors=1)):
        with pytest.raises(ValueError):
            api.compact_unitigs_cleaned(["ACGTACGTTT"], 4, **kw)


def test_fuzz_over_tiny_alphabets(gpu):
    rng = random.Random(2024)
    removed = rounds_seen = 0
    for seed in range(300):
        k = rng.randrange(2, 7)
        alphabet = rng.sample("ACGT", rng.randrange(2, 5))
        records = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 31))) for _ in range(rng.randrange(1, 6))]
        kw = dict(clip_tips=rng.choice([0, 1, 2, 3, k, 2 * k, 40]), remove_isolated=rng.choice([0, 0, 2, k, 40]), rounds=rng.randrange(1, 17),
                  m=rng.choice([1, 1, 2, 3]))
        if rng.random() < 0.5:
            kw.update(record_colors=[rng.randrange(3) for _ in records], n_colors=3, split=rng.random() < 0.5)
        try:
            got, _ = _check(records, k, **kw)
        except AssertionError:
            print("seed", seed, "k", k, records, kw)
            raise
        removed += got[5].removed_kmers > 0
        rounds_seen = max(rounds_seen, got[5].rounds_run)
    assert removed >= 50 and rounds_seen >= 3, (removed, rounds_seen)  # the fuzz reaches the rounds


@pytest.mark.parametrize("k", [31, 40])
def test_beyond_one_workgroup_and_one_scan_block(gpu, k):
    rng = random.Random(900 + k)
    g = "".join(rng.choices("ACGT", k=300_000))
    records, planted = T.plant_tips(rng, g, k, 3000, _dna(rng))
    genome_store = api.compact_unitigs([g], k)[0]
    want = genome_store.arrays()  # (views: the store stays alive)
    first = api.compact_unitigs_cleaned(records, k, clip_tips=k)
    second = api.compact_unitigs_cleaned(records, k, clip_tips=k, rounds=2)
    for got in (first, second):
        data, off = got[0].arrays()
        assert data.tobytes() == want[0].tobytes() and np.array_equal(off, want[1])
        assert got[5].tips == 3000 and got[5].tip_kmers == planted and got[5].isolated == 0 and got[5].removed_occurrences == planted
        assert got[2].distinct_kept == got[1].distinct_kmers + planted
    assert (first[5].rounds_run, second[5].rounds_run) == (1, 2)
    uncleaned = api.compact_unitigs(records, k)[1]
    assert uncleaned.unitigs > 6000 and first[1].unitigs == len(want[1]) - 1
